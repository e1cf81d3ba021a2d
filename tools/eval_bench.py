#!/usr/bin/env python
"""Evaluation row: batched yv4_iou_coco / yv4_match_coco on a COCO-val-sized problem table
vs the per-problem CPU ops (the reference's compiled Cython from oracle/_ref when it travelled with the
snapshot -- kind "reference" -- else the oracle restatement -- kind "port").
Usage (GPU box):  python tools/eval_bench.py [--images 5000] [--classes 80] [--reps 10]
Prints ONE JSON line: problems/s for IoU + matching (10 thresholds x 4 breakdowns), inputs resident in HBM.

``--fast-bbox``: the whole metric instead (``evaluate_fast_bbox``: ten thresholds, 'All' + three scale ranges, the
six-number report) on a synthetic dataset of the same statistics (5 000 x 80, about 2.4 M detections and 0.6 M gts), list
path against flat path: the list leg (per-image lists, per-image annotation dicts), and the flat legs -- the table as numpy
arrays or GPU tensors, each with the ``FlexGt`` built per call or cached.  The legs alternate run by run after one warming
run; host clock around a device synchronise, median with min / max over --reps runs, phase by phase.  Also the largest
difference of the six report numbers between the two paths (their score ties are ordered differently)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd import eval_utils as EU  # noqa: E402


def table(rng, images, classes, mean_det, mean_gt):
    P = images * classes
    nd = rng.poisson(mean_det, P)
    ng = rng.poisson(mean_gt, P)
    live = (nd > 0) & (ng > 0)
    nd, ng = nd[live], ng[live]
    det_off, gt_off = EU._offsets(nd), EU._offsets(ng)

    def boxes(n):
        xy = rng.uniform(0, 600, (n, 2))
        return np.concatenate([xy, xy + rng.uniform(4, 200, (n, 2))], 1).astype(np.float32)
    gt, det = boxes(int(gt_off[-1])), boxes(int(det_off[-1]))
    crowd = rng.random(len(gt)) < 0.05
    return nd, ng, det_off, gt_off, det, gt, crowd


FAST_LEGS = ('numpy', 'numpy_cached_gt', 'gpu', 'gpu_cached_gt')
FAST_PHASES = ('gt_build', 'upload', 'rank', 'match', 'accumulate', 'download', 'results', 'total')
LIST_PHASES = ('problems', 'match', 'accumulate', 'report', 'total')


def fast_dataset(rng, images, classes, mean_det, mean_gt):
    def boxes(n):
        xy = rng.uniform(0, 600, (n, 2))
        return np.concatenate([xy, xy + np.exp(rng.uniform(np.log(4.0), np.log(300.0), (n, 2)))], 1).astype(np.float32)
    dets, annos = [], []
    for _ in range(images):
        ng, nd = rng.poisson(mean_gt, classes), rng.poisson(mean_det, classes)
        gt = boxes(int(ng.sum()))
        crowd = rng.random(len(gt)) < 0.05
        wh = gt[:, 2:] - gt[:, :2]
        per_cls, lo = [], 0
        for c in range(classes):
            d = boxes(int(nd[c]))
            k = min(int(ng[c]), int(nd[c]))
            d[:k] = gt[lo:lo + k] + rng.normal(0, 4, (k, 4)).astype(np.float32)       # some detections sit on gts
            lo += int(ng[c])
            per_cls.append(np.concatenate([d, rng.random((len(d), 1)).astype(np.float32)], 1))
        dets.append(per_cls)
        annos.append(dict(gt_bboxes=gt, gt_labels=np.repeat(np.arange(classes), ng),
                          gt_attrs=dict(ignore=crowd | (rng.random(len(gt)) < 0.05), iscrowd=crowd,
                                        area=(wh[:, 0] * wh[:, 1]).astype(np.float32))))
    return dets, annos


def _stats(xs):
    return dict(median_ms=round(float(np.median(xs)) * 1e3, 2), min_ms=round(float(np.min(xs)) * 1e3, 2),
                max_ms=round(float(np.max(xs)) * 1e3, 2))


def fast_bbox(a):
    from mmdet_yolov4_amd.coco_eval import flatten_results
    dev = torch.device('cuda', 0)
    dets, annos = fast_dataset(np.random.default_rng(0), a.images, a.classes, a.mean_det, a.mean_gt)
    classes = [str(c) for c in range(a.classes)]
    thrs = [0.5 + 0.05 * x for x in range(10)]
    bk = [dict(type='ScaleBreakdown', scale_ranges=dict(EU.FAST_BBOX_SCALE_RANGES))]
    report_cfg = [('map', lambda x: x['breakdown'] == 'All'),
                  ('map50', lambda x: x['iou_threshold'] == 0.5 and x['breakdown'] == 'All'),
                  ('map75', lambda x: x['iou_threshold'] == 0.75 and x['breakdown'] == 'All'),
                  ('s_map', lambda x: x['breakdown'] == 'Scale_S'), ('m_map', lambda x: x['breakdown'] == 'Scale_M'),
                  ('l_map', lambda x: x['breakdown'] == 'Scale_L')]

    def fse():
        return pkg.FlexibleStatisticsEval(classes, thrs, bk, dict(type='IOU2DCoCo'), dict(type='MatcherCoCo'), 0)
    t0 = time.perf_counter()
    flat_np = flatten_results(dets)
    flatten_s = time.perf_counter() - t0
    flat_gpu = tuple(torch.from_numpy(x).to(dev) for x in flat_np)
    gt_cached = pkg.FlexGt(annos, a.classes, EU.FAST_BBOX_SCALE_RANGES)

    def flat_leg(flat, cached, rec):
        ph, f = {}, fse()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gt = f._flat_gt(cached if cached is not None else annos)
        t1 = time.perf_counter()
        out = EU.flex_flat_device(flat, gt, thrs, True, phases=ph)
        t2 = time.perf_counter()
        rep = f.report(f._flat_list(out, gt), report_cfg)
        t3 = time.perf_counter()
        if rec is not None:
            for k, v in dict(ph, gt_build=t1 - t0, results=t3 - t2, total=t3 - t0).items():
                rec[k].append(v)
        return rep, out

    def list_leg(rec):
        f, ph = fse(), dict(problems=0.0, match=0.0)

        def timed(name, fn):
            def call(*args):
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = fn(*args)
                torch.cuda.synchronize()
                ph[name] += time.perf_counter() - t
                return r
            return call
        f._problems, f._match_all = timed('problems', f._problems), timed('match', f._match_all)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = f.statistics_eval(dets, annos)
        t1 = time.perf_counter()
        rep = f.report(res, report_cfg)
        t2 = time.perf_counter()
        if rec is not None:
            for k, v in dict(ph, accumulate=t1 - t0 - ph['problems'] - ph['match'], report=t2 - t1, total=t2 - t0).items():
                rec[k].append(v)
        return rep
    frec = {leg: {k: [] for k in FAST_PHASES} for leg in FAST_LEGS}
    lrec = {k: [] for k in LIST_PHASES}
    reports = {}
    for r in range(a.reps + 1):                                   # run 0 warms the shapes
        for leg in FAST_LEGS:                                     # alternating with the list leg below
            reports[leg], tables = flat_leg(flat_gpu if leg.startswith('gpu') else flat_np,
                                            gt_cached if leg.endswith('cached_gt') else None, frec[leg] if r else None)
        if r <= a.list_reps:
            reports['list'] = list_leg(lrec if r else None)
    diff = {leg: {k: abs(float(reports[leg][k]) - float(reports['list'][k])) for k in reports['list']} for leg in FAST_LEGS}
    tied = int(sum(len(s) - len(np.unique(s)) for s in (flat_np[0][flat_np[1] == c, 4] for c in range(a.classes))))
    out = dict(tool='eval_bench --fast-bbox', metric="metric='fast-bbox', seconds per dataset", unit='s',
               value=_stats(frec['gpu_cached_gt']['total'])['median_ms'] * 1e-3, images=a.images, classes=a.classes,
               problems=a.images * a.classes, thresholds=10, breakdowns=4, detections=int(tables['total_det']),
               gts=int(len(gt_cached.gt)), pairs=int(tables['pairs']), reps=a.reps, list_reps=len(lrec['total']),
               data='synthetic', flatten_results_ms=round(flatten_s * 1e3, 2),
               list={k: _stats(v) for k, v in lrec.items()}, flat={leg: {k: _stats(v) for k, v in frec[leg].items()}
                                                                    for leg in FAST_LEGS},
               report={k: {n: float(v) for n, v in rep.items()} for k, rep in reports.items()},
               max_abs_diff_to_list={leg: max(d.values()) for leg, d in diff.items()},
               detections_with_a_tied_score=tied,
               note='the list path orders equal scores as numpy argsort()[::-1] does, the flat path keeps the table order')
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fast-bbox', action='store_true')
    ap.add_argument('--list-reps', type=int, default=7, help='--fast-bbox: runs of the list leg after the warming run '
                                                            '(at most --reps; the list leg takes tens of seconds)')
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--mean-det', type=float, default=6.0)
    ap.add_argument('--mean-gt', type=float, default=1.5)
    ap.add_argument('--breakdowns', type=int, default=4)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-seconds', type=float, default=10.0)
    a = ap.parse_args()
    if a.fast_bbox:
        if '--reps' not in sys.argv:
            a.reps = 7
        return fast_bbox(a)
    rng = np.random.default_rng(0)
    dev = torch.device('cuda', 0)
    nd, ng, det_off, gt_off, det, gt, crowd = table(rng, a.images, a.classes, a.mean_det, a.mean_gt)
    P, B = len(nd), a.breakdowns
    thrs = np.array([0.5 + 0.05 * x for x in range(10)], np.float32)
    ign = rng.random((B, len(gt))) < 0.3
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_det, d_gt, d_crowd = t(det), t(gt), t(crowd)
    # matching problems = (problem, breakdown), sharing the IoU block of the problem
    q_det_off, q_gt_off = EU._offsets(np.repeat(nd, B)), EU._offsets(np.repeat(ng, B))
    q_ign = t(np.concatenate([ign[b, gt_off[k]:gt_off[k + 1]] for k in range(P) for b in range(B)]))
    q_crowd = t(np.concatenate([np.tile(crowd[gt_off[k]:gt_off[k + 1]], B) for k in range(P)]))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_iou, t_match = [], []
    for r in range(a.reps + 2):
        ev[0].record()
        iou, iou_off = EU.iou_coco_batched(d_det, d_gt, d_crowd, det_off, gt_off)
        ev[1].record()
        EU.match_coco_batched(iou, q_det_off, q_gt_off, np.repeat(iou_off[:-1], B), thrs, q_ign, q_crowd)
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 2:
            t_iou.append(ev[0].elapsed_time(ev[1]))
            t_match.append(ev[1].elapsed_time(ev[2]))
    ms_iou, ms_match = float(np.median(t_iou)), float(np.median(t_match))
    pairs = int(iou_off[-1])
    iou_bytes = 4 * pairs + 16 * (len(det) + len(gt)) + len(gt)
    # ---- CPU: per-problem ops on a bounded sample -----------------------------------------------------
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import build_ref, eval_oracle
    fns = build_ref.load_eval()
    kind = 'reference' if fns is not None else 'port'
    f_iou, f_match = fns if fns is not None else (eval_oracle.iou_coco, eval_oracle.match_coco)
    done, t0 = 0, time.perf_counter()
    while done < P and time.perf_counter() - t0 < a.cpu_seconds:
        k = done
        c = crowd[gt_off[k]:gt_off[k + 1]]
        m = f_iou(det[det_off[k]:det_off[k + 1]], gt[gt_off[k]:gt_off[k + 1]], c)
        for b in range(B):
            f_match(m, thrs, ign[b, gt_off[k]:gt_off[k + 1]], c)
        done += 1
    cpu_s = time.perf_counter() - t0
    out = dict(metric='evaluation problems (image x class) per second, IoU + matching', unit='problems/s',
               value=P / ((ms_iou + ms_match) * 1e-3), problems=P, pairs=pairs, thresholds=10, breakdowns=B,
               ms_iou=ms_iou, ms_match=ms_match, dtype='f32',
               data='synthetic (inputs resident in HBM; launch + table upload included)',
               roofline=dict(kernel='iou_coco_kernel', bound='hbm', achieved=iou_bytes / (ms_iou * 1e-3) / 1e9,
                             peak=8000.0, unit='GB/s', frac=iou_bytes / (ms_iou * 1e-3) / 1e9 / 8000.0, traffic=None),
               cpu_baseline=dict(value=done / cpu_s, unit='problems/s', cores=1, kind=kind,
                                 sample=f'first {done} of {P} problems, per-problem calls'))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
