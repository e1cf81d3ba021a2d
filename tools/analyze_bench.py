#!/usr/bin/env python
"""Per-image mAP row: image_maps on a COCO-val-sized synthetic set (the generator of tools/map_bench.py: 5 000 images x
80 classes, Poisson detections and gts per problem), ten IoU thresholds, phase by phase.
Usage (GPU box):   python tools/analyze_bench.py [--images 5000] [--classes 80] [--reps 5] [--loop-images 50]
Legs of image_maps (host clock around a device synchronise, shapes warmed by one full run first; median of --reps runs
with min / max), alternating run by run: from the per-image lists (flatten_results, the ground-truth tables built per
call), from flat numpy arrays with a cached MapGt, and from GPU tensors with a cached MapGt.  Phases: flatten, gt_build,
upload, rank (yv4_map_rank and its one read-back), tpfp (overlaps + tpfp), accumulate (yv4_map_image_ap +
yv4_map_image_mean), download.
The comparison is the only route the package had before: its own eval_map called per image with the ten thresholds
(one batched call per image), on the first --loop-images images and scaled to the set -- the scaling is stated in the
output, not measured.  A small set (--small-images) is scored both ways too, to show where the set-up cost of the
device pass dominates.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from map_bench import dataset, stats  # noqa: E402

PHASES = ('flatten', 'gt_build', 'upload', 'rank', 'tpfp', 'accumulate', 'download', 'total')
LEGS = ('lists', 'numpy_cached_gt', 'gpu_cached_gt')


def leg(A, ME, flatten_results, dets, annos, classes, flat, gt, rec):
    ph = {}
    t0 = time.perf_counter()
    if flat is None:
        flat = flatten_results(dets)
    t1 = time.perf_counter()
    if gt is None:
        gt = ME.MapGt(annos, classes)
    t2 = time.perf_counter()
    maps, _ = A.image_maps_device(flat, gt, phases=ph)
    t3 = time.perf_counter()
    if rec is not None:
        for k, v in dict(ph, flatten=t1 - t0, gt_build=t2 - t1, total=t3 - t0).items():
            rec[k].append(v)
    return maps


def eval_map_loop(pkg, A, dets, annos, images):
    """The package's eval_map per image, ten thresholds a call: seconds, and the per-image mAPs."""
    thrs = list(A.default_iou_thrs())
    t0 = time.perf_counter()
    maps = []
    for i in range(images):
        means = [m for m, _ in pkg.eval_map([dets[i]], [annos[i]], iou_thr=thrs, logger='silent')]
        maps.append(sum(means) / len(means))
    return time.perf_counter() - t0, np.array(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--mean-det', type=float, default=6.0)
    ap.add_argument('--mean-gt', type=float, default=1.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--loop-images', type=int, default=50)
    ap.add_argument('--small-images', type=int, default=8)
    a = ap.parse_args()
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import analysis as A, map_eval as ME
    from mmdet_yolov4_amd.coco_eval import flatten_results
    dets, annos = dataset(np.random.default_rng(0), a.images, a.classes, a.mean_det, a.mean_gt)
    flat_np = flatten_results(dets)
    flat_gpu = tuple(torch.from_numpy(x).cuda() for x in flat_np)
    gt = ME.MapGt(annos, a.classes)
    rec = {name: {k: [] for k in PHASES} for name in LEGS}
    maps = {}
    for r in range(a.reps + 1):                                   # run 0 warms the shapes
        for name in LEGS:
            maps[name] = leg(A, ME, flatten_results, dets, annos, a.classes,
                             None if name == 'lists' else flat_gpu if name == 'gpu_cached_gt' else flat_np,
                             None if name == 'lists' else gt, rec[name] if r else None)
    assert all(maps[name].tobytes() == maps['lists'].tobytes() for name in LEGS)
    n = min(a.loop_images, a.images)
    eval_map_loop(pkg, A, dets, annos, min(n, 3))                  # warm
    loop_s, loop_maps = eval_map_loop(pkg, A, dets, annos, n)
    out = dict(metric='image_maps, ten IoU thresholds, seconds per dataset', images=a.images, classes=a.classes,
               problems=a.images * a.classes, detections=int(len(flat_np[0])), gts=int(len(gt.gt)), thresholds=10,
               data='synthetic', reps=a.reps, legs={name: {k: stats(v) for k, v in rec[name].items()} for name in LEGS},
               value=stats(rec['gpu_cached_gt']['total'])['median_ms'] * 1e-3, unit='s',
               eval_map_loop=dict(images=n, seconds=loop_s, per_image_ms=loop_s / n * 1e3,
                                  scaled_to_set_s=loop_s / n * a.images,
                                  note='this package\'s eval_map per image, one call for the ten thresholds; measured on '
                                       f'{n} images and scaled linearly to {a.images}',
                                  max_abs_diff=float(np.abs(loop_maps - maps['lists'][:n]).max())))
    m = min(a.small_images, a.images)
    if m:
        small = {k: [] for k in PHASES}
        for r in range(a.reps + 1):
            leg(A, ME, flatten_results, dets[:m], annos[:m], a.classes, None, None, small if r else None)
        s_loop, _ = eval_map_loop(pkg, A, dets, annos, m)
        out['small'] = dict(images=m, image_maps_lists={k: stats(v) for k, v in small.items()}, eval_map_loop_s=s_loop)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
