#!/usr/bin/env python
"""Proposal-recall row: eval_recalls on a COCO-val-sized synthetic set -- 5 000 images, 2.4 M detections (Poisson 480 an
image), gts at COCO's density (Poisson 7.3 an image), proposal_nums (100, 300, 1000), ten IoU thresholds.
Usage (GPU box):        python tools/recall_bench.py [--images 5000] [--passes 7]
      (build container)  python tools/recall_bench.py --cpu-only     # only the CPU column
Legs, alternating pass by pass (pass 0 warms the shapes and is dropped); median and min - max over the passes:
  flat_gpu_cached_gt   the flat GPU table against a cached RecallGt: upload / rank / match / download (``phases``, each
                       closed by a device synchronise) and the host clock around the whole call
  flat_gpu_workspace   the same with lds_cap=1: every pair in the workspace form
  lists                per-image per-class lists, the RecallGt built per call: concatenation, upload and all
Beside them, as a CPU number: the numpy restatement (tests/_recall_ref.py) on --ref-images images, one core, scaled to
the whole set by the image count.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NUMS = (100, 300, 1000)
THRS = np.linspace(.5, 0.95, 10)
CLASSES = 80


def dataset(rng, images, mean_det, mean_gt):
    """Per image the gts (g, 4) and a per-class list of (n, 5) detections; the first detections of an image sit on its
    gts with three qualities of jitter, the rest is clutter."""
    def boxes(n):
        xy = rng.uniform(0, 600, (n, 2))
        return np.concatenate([xy, xy + rng.uniform(4, 200, (n, 2))], 1).astype(np.float32)
    gts, results = [], []
    for _ in range(images):
        g, n = int(rng.poisson(mean_gt)), int(rng.poisson(mean_det))
        gb = boxes(g)
        d = boxes(n)
        k = min(3 * g, n)
        if k:
            src = np.arange(k) % g
            d[:k] = gb[src] + (rng.normal(0, 1, (k, 4)) * np.array([2.0, 8.0, 20.0])[np.arange(k) // g % 3, None]).astype(np.float32)
        d = np.concatenate([d, rng.random((n, 1)).astype(np.float32)], 1)
        lab = np.sort(rng.integers(0, CLASSES, n))
        results.append(np.split(d, np.searchsorted(lab, np.arange(1, CLASSES))))
        gts.append(gb)
    return gts, results


def stats(xs):
    return dict(median_ms=float(np.median(xs)) * 1e3, min_ms=float(np.min(xs)) * 1e3, max_ms=float(np.max(xs)) * 1e3)


def gpu_legs(gts, results, passes):
    import torch
    import mmdet_yolov4_amd as pkg
    flat = tuple(torch.from_numpy(a).cuda() for a in pkg.flatten_results(results))
    gt = pkg.RecallGt(gts)
    keys = ('upload', 'rank', 'match', 'download', 'total')
    rec = {leg: {k: [] for k in keys} for leg in ('flat_gpu_cached_gt', 'flat_gpu_workspace')}
    rec['lists'] = dict(total=[])
    out = {}
    for r in range(passes + 1):
        for leg, cap in (('flat_gpu_cached_gt', 0), ('flat_gpu_workspace', 1)):
            ph = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[leg] = pkg.recall_device(flat, gt, NUMS, THRS, phases=ph, lds_cap=cap)
            ph['total'] = time.perf_counter() - t0
            if r:
                for k in keys:
                    rec[leg][k].append(ph.get(k, 0.0))
        t0 = time.perf_counter()
        out['lists'] = pkg.eval_recalls(gts, results, NUMS, THRS, logger='silent')
        if r:
            rec['lists']['total'].append(time.perf_counter() - t0)
    assert all((out[leg] == out['lists']).all() for leg in out)
    return ({leg: {k: stats(v) for k, v in d.items()} for leg, d in rec.items()}, out['lists'], int(flat[0].shape[0]),
            gt.total_gt)


def cpu_column(gts, results, ref_images):
    import _recall_ref as RR
    g, p = gts[:ref_images], RR.concat_classes(results[:ref_images])
    t0 = time.perf_counter()
    rec = RR.recalls(g, p, NUMS, THRS)
    s = time.perf_counter() - t0
    return dict(seconds=s, images=len(g), scaled_to_all_images_s=s * len(gts) / max(len(g), 1),
                kind='CPU, numpy restatement, 1 core', ar=rec.mean(axis=1).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--mean-det', type=float, default=480.0)
    ap.add_argument('--mean-gt', type=float, default=7.3)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--ref-images', type=int, default=500)
    ap.add_argument('--cpu-only', action='store_true')
    a = ap.parse_args()
    gts, results = dataset(np.random.default_rng(0), a.images, a.mean_det, a.mean_gt)
    out = dict(metric='eval_recalls, proposal_nums (100, 300, 1000), ten IoU thresholds, seconds per dataset',
               images=a.images, proposal_nums=list(NUMS), thresholds=len(THRS), data='synthetic')
    if not a.cpu_only:
        legs, rec, D, G = gpu_legs(gts, results, a.passes)
        out.update(legs=legs, detections=D, gts=G, ar=rec.mean(axis=1).tolist(), passes=a.passes,
                   value=legs['flat_gpu_cached_gt']['total']['median_ms'] * 1e-3, unit='s')
    out['cpu'] = cpu_column(gts, results, min(a.ref_images, a.images))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
