#!/usr/bin/env python
"""COCO error analysis row: the seven precision curves on the COCO-val-sized synthetic dataset of
tools/coco_eval_bench.py (5 000 images x 80 classes, Poisson detections and gts per problem, 5 % crowd gts), its 80
categories in twelve supercategory groups, phase by phase.
Usage (GPU box):  python tools/coco_error_bench.py [--images 5000] [--classes 80] [--mean-gt 1.5] [--reps 5]
                  python tools/coco_error_bench.py --numpy-images 8          (host only: the restatement's time)
Measured (one warming run, then the median with min / max of --reps runs, the forms alternating inside a repetition):
  one_pass_gpu / one_pass_list   error_analysis from GPU tensors and from the per-image lists: host-clock phases, each
                                 closed by a device synchronise, and the device phases between device events (*_dev)
  three_round                    the same analysis through yv4_coco_rank / yv4_coco_match / yv4_coco_accumulate alone:
                                 the base round, a "Sim" round and an "Oth" round, each on a ground-truth table expanded on
                                 the host (every annotation copied into the problem of each category it is relabelled
                                 to: K-fold for Oth).  Device phases between device events; the host expansion and its
                                 upload once, outside the repetitions.  Its result must equal the one-pass result bit
                                 for bit, or the tool fails.
  numpy                          the literal restatement (tests/_coco_error_ref.py, 1 + 2 K numpy COCOeval runs) on the
                                 first --numpy-images images, with the time scaled to --images stated as scaled
Prints ONE JSON line."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = 12
DEV_PHASES = ('ordering', 'matching', 'accumulation')


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stats(xs):
    return dict(median_ms=float(np.median(xs)) * 1e3, min_ms=float(np.min(xs)) * 1e3, max_ms=float(np.max(xs)) * 1e3)


def expanded_tables(tab, which):
    """The per-problem ground-truth table of yv4_coco_match for the 'sim' / 'oth' run, from the image-major table of
    coco_error.tables: annotation g of category c goes into problem (image, k) for every k it is relabelled to (k == c:
    itself, with its own flags; else an ignored crowd).  Vectorised; annotation order inside a problem."""
    K, N = tab['K'], tab['N']
    G = len(tab['gt_cat'])
    img = np.repeat(np.arange(N), np.diff(tab['gt_img_off']))
    cat = tab['gt_cat'].astype(np.int64)
    if which == 'oth':
        g = np.repeat(np.arange(G), K)
        k = np.tile(np.arange(K), G)
    else:
        grp = tab['cat_group']
        order = np.argsort(grp, kind='stable')                      # the K positions, group by group
        start = np.searchsorted(grp[order], grp)                    # per k: where its group starts in `order`
        size = np.bincount(grp, minlength=int(grp.max()) + 1)[grp]  # per k: its group's size
        n = np.where(cat >= 0, size[np.maximum(cat, 0)], 0)
        g = np.repeat(np.arange(G), n)
        within = np.arange(len(g)) - np.repeat(np.cumsum(n) - n, n)
        k = order[start[cat[g]] + within]
    own = cat[g] == k
    prob = img[g] * K + k
    by = np.argsort(prob, kind='stable')
    g, own, prob = g[by], own[by], prob[by]
    flag = np.where(own, tab['gt_flag'][g], 3).astype(np.uint8)
    off = np.zeros(N * K + 1, np.int64)
    np.cumsum(np.bincount(prob, minlength=N * K), out=off[1:])
    return dict(gt_box=np.ascontiguousarray(tab['gt_box'][g]), gt_area=np.ascontiguousarray(tab['gt_area'][g]), gt_flag=flag,
                gt_off=off)


def base_tables(tab):
    keep = np.flatnonzero(tab['gt_cat'] >= 0)
    img = np.repeat(np.arange(tab['N']), np.diff(tab['gt_img_off']))[keep]
    prob = img * tab['K'] + tab['gt_cat'][keep]
    by = np.argsort(prob, kind='stable')
    g = keep[by]
    off = np.zeros(tab['P'] + 1, np.int64)
    np.cumsum(np.bincount(prob, minlength=tab['P']), out=off[1:])
    return dict(gt_box=np.ascontiguousarray(tab['gt_box'][g]), gt_area=np.ascontiguousarray(tab['gt_area'][g]),
                gt_flag=tab['gt_flag'][g], gt_off=off)


class ThreeRound:
    """The analysis through today's three entry points, one rank / match / accumulate round per run of the tool."""

    def __init__(self, tab, flat_gpu, area, conf_thr=0.1, max_det=100):
        import torch
        from mmdet_yolov4_amd import _lib
        from mmdet_yolov4_amd._eval_common import _dev
        self.torch, self.lib, self.tab = torch, _lib.lib(), tab
        self.dev = dev = flat_gpu[0].device
        t0 = time.perf_counter()
        host = [base_tables(tab), expanded_tables(tab, 'sim'), expanded_tables(tab, 'oth')]
        self.expand_s = time.perf_counter() - t0
        self.rows = [len(h['gt_area']) for h in host]
        t0 = time.perf_counter()
        self.gt = [{k: _dev(v.reshape(-1), v.dtype, dev) for k, v in h.items()} for h in host]
        torch.cuda.synchronize(dev)
        self.upload_s = time.perf_counter() - t0
        dets, labels, img_index = flat_gpu
        kmap, imap = _dev(tab['kmap'], np.int64, dev), _dev(tab['imap'], np.int64, dev)
        self.dets = dets.contiguous()
        self.prob = (imap[img_index] * tab['K'] + kmap[labels]).to(torch.int32)
        self.thrs = [_dev(np.array(t, np.float64), np.float64, dev) for t in ([0.75, 0.5, 0.1], [conf_thr], [conf_thr])]
        self.area = _dev(area.reshape(-1), np.float64, dev)
        self.rec = _dev(np.linspace(0, 1, 101), np.float64, dev)
        self.max_det, self.A = max_det, len(area)

    def run(self):
        """-> (precision (5, R, K, A, 1) on the host, {phase: seconds between device events, summed over the rounds})."""
        from mmdet_yolov4_amd._lib import check
        from mmdet_yolov4_amd.ops import stream_ptr
        torch, lib, dev, tab = self.torch, self.lib, self.dev, self.tab
        K, P, A, D, R = tab['K'], tab['P'], self.A, int(self.dets.shape[0]), 101
        md = np.array([self.max_det], dtype=np.int32)
        marks, out = [], []
        for gt, thr in zip(self.gt, self.thrs):
            T = int(thr.numel())
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            order = torch.empty(D, dtype=torch.int32, device=dev)
            sprob = torch.empty(D, dtype=torch.int32, device=dev)
            det_off = torch.empty(P + 1, dtype=torch.int64, device=dev)
            need = torch.zeros(1, dtype=torch.int64, device=dev)
            work = torch.empty(int(lib.yv4_coco_rank_work(D)) // 8 + 1, dtype=torch.int64, device=dev)
            flags = torch.empty(D * A * T, dtype=torch.uint8, device=dev)
            counts = torch.empty(K * A, dtype=torch.int32, device=dev)
            state = torch.zeros(2, dtype=torch.int64, device=dev)
            awork = torch.empty(int(lib.yv4_coco_accumulate_work(D, K, A * T)) // 8 + 1, dtype=torch.int64, device=dev)
            precision = torch.empty((T, R, K, A, 1), dtype=torch.float64, device=dev)
            scores, recall = torch.empty_like(precision), torch.empty((T, K, A, 1), dtype=torch.float64, device=dev)
            ev[0].record()
            check(lib.yv4_coco_rank(self.dets.data_ptr(), self.prob.data_ptr(), D, P, self.max_det, A * T,
                                    gt['gt_off'].data_ptr(), work.data_ptr(), order.data_ptr(), sprob.data_ptr(),
                                    det_off.data_ptr(), need.data_ptr(), stream_ptr()), 'yv4_coco_rank')
            ev[1].record()
            n = int(need.item())                                    # the read-back between the device calls
            mwork = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
            ev[2].record()
            check(lib.yv4_coco_match(self.dets.data_ptr(), order.data_ptr(), det_off.data_ptr(), gt['gt_box'].data_ptr(),
                                     gt['gt_area'].data_ptr(), gt['gt_flag'].data_ptr(), gt['gt_off'].data_ptr(), P, K, D,
                                     self.max_det, thr.data_ptr(), T, self.area.data_ptr(), A, mwork.data_ptr(), n,
                                     state.data_ptr(), flags.data_ptr(), counts.data_ptr(), stream_ptr()), 'yv4_coco_match')
            ev[3].record()
            check(lib.yv4_coco_accumulate(self.dets.data_ptr(), order.data_ptr(), sprob.data_ptr(), det_off.data_ptr(),
                                          flags.data_ptr(), counts.data_ptr(), P, K, D, md.ctypes.data, 1, T, A,
                                          self.rec.data_ptr(), R, awork.data_ptr(), precision.data_ptr(), recall.data_ptr(),
                                          scores.data_ptr(), stream_ptr()), 'yv4_coco_accumulate')
            ev[4].record()
            marks.append(ev)
            out.append(precision)
            if int(state.cpu()[1]):
                raise RuntimeError('yv4_coco_match ran out of workspace')
        precision = torch.cat(out, 0).cpu().numpy()
        return precision, {DEV_PHASES[i]: sum(ev[j].elapsed_time(ev[j + 1]) for ev in marks) * 1e-3 for i, j in enumerate((0, 2, 3))}


def numpy_slice(ds, results, n_img):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _coco_error_ref as E
    from mmdet_yolov4_amd.coco_eval import flatten_results
    sub = dict(images=ds['images'][:n_img], categories=ds['categories'],
               annotations=[a for a in ds['annotations'] if a['image_id'] < n_img])
    flat = flatten_results(results[:n_img])
    t0 = time.perf_counter()
    E.error_analysis(sub, *flat, [c['id'] for c in ds['categories']], list(range(n_img)))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--mean-det', type=float, default=6.0)
    ap.add_argument('--mean-gt', type=float, default=1.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--numpy-images', type=int, default=0, help='host only: time the numpy restatement on this many images')
    a = ap.parse_args()
    ds, results = _sibling('coco_eval_bench').dataset(np.random.default_rng(0), a.images, a.classes, a.mean_det, a.mean_gt)
    for c in ds['categories']:
        c['supercategory'] = f's{(c["id"] - 1) * GROUPS // a.classes}'
    base = dict(images=a.images, classes=a.classes, groups=GROUPS, problems=a.images * a.classes,
                gts=len(ds['annotations']), data='synthetic')
    if a.numpy_images:
        sec = numpy_slice(ds, results, a.numpy_images)
        print(json.dumps(dict(base, metric='COCO error analysis, numpy restatement (1 + 2 K COCOeval runs), host only',
                              numpy_images=a.numpy_images, seconds_on_the_slice=sec,
                              seconds_scaled_to_all_images=sec * a.images / a.numpy_images, scaled=True)))
        return
    import torch
    from mmdet_yolov4_amd import coco_error as CEA
    from mmdet_yolov4_amd.coco_eval import CocoGt, flatten_results
    gt = CocoGt(ds)
    flat_gpu = tuple(torch.from_numpy(x).cuda() for x in flatten_results(results))
    three = ThreeRound(CEA.tables(gt), flat_gpu, CEA.area_ranges())
    rec = {form: {} for form in ('one_pass_gpu', 'one_pass_list', 'three_round')}
    for r in range(a.reps + 1):                                    # run 0 warms the shapes
        runs = {}
        for form, res in (('one_pass_gpu', flat_gpu), ('one_pass_list', results)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = CEA.error_analysis(gt, res, timing=True)
            runs[form] = dict(out.phases, total=time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        precision, dev = three.run()
        runs['three_round'] = dict({k + '_dev': v for k, v in dev.items()}, total=time.perf_counter() - t0)
        if CEA.stack_ps(precision).tobytes() != out.ps.tobytes():
            raise SystemExit('the three-round form and the one-pass form disagree')
        if r:
            for form, ph in runs.items():
                for k, v in ph.items():
                    rec[form].setdefault(k, []).append(v)
    phases = {form: {k: stats(v) for k, v in ph.items()} for form, ph in rec.items()}
    device = {form: sum(phases[form][k + '_dev']['median_ms'] for k in DEV_PHASES) for form in ('one_pass_gpu', 'three_round')}
    print(json.dumps(dict(base, metric='COCO error analysis (C75 C50 Loc Sim Oth BG FN), seconds per dataset',
                          detections=int(flat_gpu[0].shape[0]), reps=a.reps, phases=phases,
                          three_round_host=dict(expand_s=three.expand_s, upload_s=three.upload_s, gt_rows=three.rows),
                          device_ms=device, matching_ratio=phases['three_round']['matching_dev']['median_ms']
                          / phases['one_pass_gpu']['matching_dev']['median_ms'],
                          device_ratio=device['three_round'] / device['one_pass_gpu'], equal=True,
                          aps_allclass=out.aps().tolist(), value=phases['one_pass_gpu']['total']['median_ms'] * 1e-3, unit='s')))


if __name__ == '__main__':
    main()
