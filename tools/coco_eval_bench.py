#!/usr/bin/env python
"""COCO bbox evaluation row: COCOeval (evaluate / accumulate / summarize) on a COCO-val-sized synthetic dataset with the
problem statistics of tools/eval_bench.py and tools/map_bench.py (5 000 images x 80 classes, Poisson detections and gts
per problem, 5 % crowd gts), default parameters (ten IoU thresholds, maxDets 100 / 300 / 1000), phase by phase.
Usage (GPU box):  python tools/coco_eval_bench.py [--images 5000] [--classes 80] [--reps 5] [--form list|flat|gpu]
Phases (host clock around a device synchronise; one warming run, then the median with min / max of --reps runs): host
table build (gt tables and, for the list form, the flattening of the result lists), upload, ordering (yv4_coco_rank),
matching (yv4_coco_match), accumulation (yv4_coco_accumulate), download, summarize.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ('table_build', 'upload', 'ordering', 'matching', 'accumulation', 'download', 'summarize')


def dataset(rng, images, classes, mean_det, mean_gt):
    def boxes(n):
        xy = rng.uniform(0, 600, (n, 2))
        return np.concatenate([xy, rng.uniform(4, 200, (n, 2))], 1)
    results, anns, aid = [], [], 1
    for i in range(images):
        ng = rng.poisson(mean_gt, classes)
        nd = rng.poisson(mean_det, classes)
        gt = boxes(int(ng.sum()))
        crowd = rng.random(len(gt)) < 0.05
        labels = np.repeat(np.arange(classes), ng)
        for b, c, cr in zip(gt, labels, crowd):
            anns.append(dict(id=aid, image_id=i, category_id=int(c) + 1, bbox=[float(v) for v in b],
                             area=float(b[2] * b[3]), iscrowd=int(cr)))
            aid += 1
        per_cls, lo = [], 0
        for c in range(classes):
            d = boxes(int(nd[c]))
            k = min(int(ng[c]), int(nd[c]))
            d[:k] = gt[lo:lo + k] + rng.normal(0, 8, (k, 4))                 # some detections sit on gts
            lo += int(ng[c])
            d = np.concatenate([d[:, :2], d[:, :2] + np.maximum(d[:, 2:], 1.0), rng.random((len(d), 1))], 1)
            per_cls.append(d.astype(np.float32))
        results.append(per_cls)
    ds = dict(images=[dict(id=i) for i in range(images)], categories=[dict(id=c + 1, name=str(c)) for c in range(classes)],
              annotations=anns)
    return ds, results


def stats(xs):
    return dict(median_ms=float(np.median(xs)) * 1e3, min_ms=float(np.min(xs)) * 1e3, max_ms=float(np.max(xs)) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--mean-det', type=float, default=6.0)
    ap.add_argument('--mean-gt', type=float, default=1.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--form', choices=('list', 'flat', 'gpu'), default='list')
    a = ap.parse_args()
    import torch
    from mmdet_yolov4_amd import coco_eval as CE
    ds, results = dataset(np.random.default_rng(0), a.images, a.classes, a.mean_det, a.mean_gt)
    gt = CE.CocoGt(ds)
    if a.form != 'list':
        results = CE.flatten_results(results)
        if a.form == 'gpu':
            results = tuple(torch.from_numpy(x).cuda() for x in results)
    rec = {k: [] for k in PHASES + ('total',)}
    for r in range(a.reps + 1):                                    # run 0 warms the shapes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = CE.COCOeval(gt, results, 'bbox', timing=True)
        ev.params.maxDets = [100, 300, 1000]
        ev.evaluate()
        ev.accumulate()
        ev.summarize(out=lambda line: None)
        total = time.perf_counter() - t0
        if r:
            for k in PHASES:
                rec[k].append(ev.phases[k])
            rec['total'].append(total)
    phases = {k: stats(v) for k, v in rec.items()}
    host = sum(phases[k]['median_ms'] for k in ('table_build', 'summarize'))
    print(json.dumps(dict(metric='COCOeval bbox, ten IoU thresholds, maxDets 100/300/1000, seconds per dataset',
                          images=a.images, classes=a.classes, problems=a.images * a.classes, form=a.form,
                          detections=int(ev._state['D']), gts=len(ds['annotations']), data='synthetic', reps=a.reps,
                          phases=phases, host_share=host / phases['total']['median_ms'], stats=[float(v) for v in ev.stats],
                          value=phases['total']['median_ms'] * 1e-3, unit='s')))


if __name__ == '__main__':
    main()
