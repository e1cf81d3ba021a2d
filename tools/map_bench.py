#!/usr/bin/env python
"""VOC-style mAP row: eval_map on a COCO-val-sized synthetic dataset (the problem statistics of tools/eval_bench.py:
5 000 images x 80 classes, Poisson detections and gts per problem), ten IoU thresholds, phase by phase.
Usage (GPU box):        python tools/map_bench.py [--images 5000] [--classes 80] [--reps 5]
      (build container)  python tools/map_bench.py --cpu-only     # only the CPU columns
Phases of the package (host clock around a device synchronise, shapes warmed by one full run first; median of --reps
runs with min / max): host table build, host sorts, upload, the two device calls, download, host accumulation.
Beside it, on --ref-images images of the same dataset and labelled as CPU numbers: the package's numpy restatement
(tests/_map_ref.py) on one core, and -- where the reference checkout exists -- the imported reference with nproc=4,
called once per threshold as datasets/custom.py does.
The flat legs (``flat``) score the same dataset from the flat table ``(dets, labels, img_index)`` -- ordering and
accumulation on the device too (csrc/map_flat.hip) -- as numpy arrays and as GPU tensors, each with the ground-truth
tables built per call and with a cached ``MapGt``: gt_build, upload (the tables, the thresholds, a numpy table), rank
(``yv4_map_rank`` and its one read-back), tpfp (overlaps + tpfp), accumulate, download, results (the per-class dicts and
mean_ap on the host).  The list leg and the flat legs alternate run by run.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

THRS = [0.5 + 0.05 * x for x in range(10)]


def dataset(rng, images, classes, mean_det, mean_gt):
    def boxes(n):
        xy = rng.uniform(0, 600, (n, 2))
        return np.concatenate([xy, xy + rng.uniform(4, 200, (n, 2))], 1).astype(np.float32)
    dets, annos = [], []
    for _ in range(images):
        ng = rng.poisson(mean_gt, classes)
        nd = rng.poisson(mean_det, classes)
        gt = boxes(int(ng.sum()))
        labels = np.repeat(np.arange(classes), ng)
        per_cls, lo = [], 0
        for c in range(classes):
            d = boxes(int(nd[c]))
            k = min(int(ng[c]), int(nd[c]))
            d[:k] = gt[lo:lo + k] + rng.normal(0, 8, (k, 4)).astype(np.float32)      # some detections sit on gts
            lo += int(ng[c])
            per_cls.append(np.concatenate([d, rng.random((len(d), 1)).astype(np.float32)], 1))
        dets.append(per_cls)
        annos.append(dict(bboxes=gt, labels=labels))
    return dets, annos


def stats(xs):
    return dict(median_ms=float(np.median(xs)) * 1e3, min_ms=float(np.min(xs)) * 1e3, max_ms=float(np.max(xs)) * 1e3)


FLAT_LEGS = ('numpy', 'numpy_cached_gt', 'gpu', 'gpu_cached_gt')
FLAT_PHASES = ('gt_build', 'upload', 'rank', 'tpfp', 'accumulate', 'download', 'results', 'total')


def flat_leg(ME, _lib, flat, annos, classes, cached_gt, rec):
    ph = {}
    t0 = time.perf_counter()
    gt = cached_gt if cached_gt is not None else ME.MapGt(annos, classes)
    t1 = time.perf_counter()
    out = ME.map_flat_device(flat, gt, _lib.TPFP_DEFAULT, THRS, None, 'area', False, phases=ph)
    t2 = time.perf_counter()
    res = [ME._flat_eval_results(out, t, None, False) for t in range(len(THRS))]
    t3 = time.perf_counter()
    if rec is not None:
        for k, v in dict(ph, gt_build=t1 - t0, results=t3 - t2, total=t3 - t0).items():
            rec[k].append(v)
    return [m for m, _ in res]


def gpu_phases(dets, annos, reps, classes):
    import torch
    from mmdet_yolov4_amd import _lib, map_eval as ME
    from mmdet_yolov4_amd.coco_eval import flatten_results
    rec = {k: [] for k in ('table_build', 'sorts', 'upload', 'launch', 'download', 'accumulate', 'total')}
    t0 = time.perf_counter()
    flat_np = flatten_results(dets)
    flatten_s = time.perf_counter() - t0
    flat_gpu = tuple(torch.from_numpy(a).cuda() for a in flat_np)
    gt_cached = ME.MapGt(annos, classes)
    frec = {leg: {k: [] for k in FLAT_PHASES} for leg in FLAT_LEGS}
    fmaps = {}
    for r in range(reps + 1):                                     # run 0 warms the shapes
        for leg in FLAT_LEGS:                                     # alternating with the list leg below
            fmaps[leg] = flat_leg(ME, _lib, flat_gpu if leg.startswith('gpu') else flat_np, annos, classes,
                                  gt_cached if leg.endswith('cached_gt') else None, frec[leg] if r else None)
        ph = {}
        t0 = time.perf_counter()
        tab = ME.MapTables(dets, annos)
        t1 = time.perf_counter()
        tab.sort()
        t2 = time.perf_counter()
        tp, fp = ME.tpfp_batched(tab, _lib.TPFP_DEFAULT, THRS, None, phases=ph)
        t3 = time.perf_counter()
        num_gts = ME._num_gts(tab, None)
        res = [ME.accumulate(tab, tp[t], fp[t], num_gts, None, None) for t in range(len(THRS))]
        t4 = time.perf_counter()
        if r:
            for k, v in (('table_build', t1 - t0), ('sorts', t2 - t1), ('accumulate', t4 - t3), ('total', t4 - t0)):
                rec[k].append(v)
            for k in ('upload', 'launch', 'download'):
                rec[k].append(ph[k])
    maps = [m for m, _ in res]
    flat = dict(flatten_results_ms=flatten_s * 1e3,
                max_abs_diff_to_list={leg: float(np.abs(np.array(fmaps[leg]) - np.array(maps)).max()) for leg in FLAT_LEGS},
                note='the list path orders equal scores as np.argsort does, the flat path keeps the table order')
    for leg in FLAT_LEGS:
        flat[leg] = {k: stats(v) for k, v in frec[leg].items()}
    return {k: stats(v) for k, v in rec.items()}, maps, int(len(tab.det)), int(len(tab.gt)), int(
        (tab.nd * tab.ng).sum()), flat


def cpu_columns(dets, annos, ref_images):
    import _map_ref as R
    d, a = dets[:ref_images], annos[:ref_images]
    out = {}
    t0 = time.perf_counter()
    maps = [R.eval_map(d, a, iou_thr=t)[0] for t in THRS]
    out['restatement_1core'] = dict(seconds=time.perf_counter() - t0, images=len(d), kind='CPU, numpy restatement, 1 core',
                                    mean_aps=maps)
    import _ref_import
    if _ref_import.available():
        from make_golden_map import import_reference_map
        M, _ = import_reference_map(serial_pool=False)
        t0 = time.perf_counter()
        maps = [M.eval_map(d, a, iou_thr=t, logger='silent', nproc=4)[0] for t in THRS]
        out['reference_nproc4'] = dict(seconds=time.perf_counter() - t0, images=len(d),
                                       kind='CPU, imported reference, Pool(4), one call per threshold', mean_aps=maps)
    else:
        out['reference_nproc4'] = 'not measured (no reference checkout on this machine)'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--mean-det', type=float, default=6.0)
    ap.add_argument('--mean-gt', type=float, default=1.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ref-images', type=int, default=100)
    ap.add_argument('--cpu-only', action='store_true')
    a = ap.parse_args()
    dets, annos = dataset(np.random.default_rng(0), a.images, a.classes, a.mean_det, a.mean_gt)
    out = dict(metric='eval_map, ten IoU thresholds, seconds per dataset', images=a.images, classes=a.classes,
               problems=a.images * a.classes, thresholds=len(THRS), data='synthetic')
    if not a.cpu_only:
        phases, maps, D, G, pairs, flat = gpu_phases(dets, annos, a.reps, a.classes)
        out.update(phases=phases, flat=flat, detections=D, gts=G, pairs=pairs, mean_aps=maps, reps=a.reps,
                   value=phases['total']['median_ms'] * 1e-3, unit='s')
    out['cpu'] = cpu_columns(dets, annos, min(a.ref_images, a.images))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
