#!/usr/bin/env python
"""The validation pass of a training run, both result forms: the list loop (``single_gpu_test`` -> per-class numpy
lists -> ``evaluate_bbox``) against the flat loop (``single_gpu_test(flat=True)`` -> the result table built on the device
by ``yv4_results_append`` -> ``evaluate_bbox``).  YOLOv4-S at 416 in a 16-bit dtype, synthetic images and ground truth,
a few hundred images at batch 32; the head is calibrated like bench.py's (about ``--candidates`` scores per image pass
``score_thr``), so every image fills a good part of ``max_per_img=300``.
Usage (GPU box):  python tools/val_loop_bench.py [--images 320] [--batch 32] [--size 416] [--passes 7] [--dtype fp16]
Both loops run in the same process on the same plans, alternating, after one warming pass of each; per pass the host
clock around work that ends in a device synchronise: the loop, the scoring, and their sum.  Median with min / max over
the passes.  The two forms must give the same metrics, or the tool fails.  ``--metric mAP`` scores with a
``CustomBBoxDataset`` (``evaluate_map``) over the same ground truth instead; its two forms order equal scores differently
(map_eval.py), and 16-bit scores tie, so there the tool reports whether the metrics agree instead of failing.
``--metric fast-bbox`` scores with ``CocoBBoxDataset.evaluate(metric='fast-bbox')`` (``evaluate_fast_bbox``; its ``FlexGt`` is
built once, before the passes); the same holds for its ties, and the largest difference of the six report numbers is given.
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import mmdet_yolov4_amd as pkg  # noqa: E402


def ground_truth(rng, images, size, classes=80, mean_gt=7.0):
    anns = []
    for i in range(images):
        n = max(1, int(rng.poisson(mean_gt)))
        xy = rng.uniform(0, size * 0.8, (n, 2))
        wh = np.exp(rng.uniform(np.log(8.0), np.log(size / 2), (n, 2)))
        for (x, y), (w, h), c, crowd in zip(xy, wh, rng.integers(0, classes, n), rng.random(n) < 0.05):
            anns.append(dict(id=len(anns) + 1, image_id=i, category_id=int(c) + 1, bbox=[float(x), float(y), float(w), float(h)],
                             area=float(w * h), iscrowd=int(crowd)))
    return pkg.CocoGt(dict(images=[dict(id=i) for i in range(images)],
                           categories=[dict(id=c + 1, name=str(c)) for c in range(classes)], annotations=anns))


def stats(xs):
    return dict(median_ms=round(float(np.median(xs)) * 1e3, 2), min_ms=round(float(np.min(xs)) * 1e3, 2),
                max_ms=round(float(np.max(xs)) * 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=320)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--candidates', type=float, default=2000.0)
    ap.add_argument('--dtype', choices=('fp16', 'bf16'), default='fp16')
    ap.add_argument('--metric', choices=('bbox', 'mAP', 'fast-bbox'), default='bbox')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('val_loop_bench measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg('yolov4s'))
    det.init_weights()
    det.eval().to(dev)
    pkg.wrap_fp16_model(det, torch.float16 if a.dtype == 'fp16' else torch.bfloat16)
    nb = -(-a.images // a.batch)
    sizes = [min(a.batch, a.images - b * a.batch) for b in range(nb)]
    batches = [bench.synthetic_images(n, a.size, 100 + b, dev) for b, n in enumerate(sizes)]
    plan = det.compile(a.batch, a.size, a.size, device=dev, rescale=True, graph=False)
    per_img = bench.init_head(det, plan, batches[0], a.candidates)
    metas = [dict(scale_factor=np.ones(4, np.float32))] * a.batch
    loader = [dict(img=[img], img_metas=[metas[:img.shape[0]]]) for img in batches]
    gt = ground_truth(np.random.default_rng(1), a.images, a.size)
    if a.metric == 'mAP':
        xywh = gt.ann_box.astype(np.float32)
        xyxy = np.concatenate([xywh[:, :2], xywh[:, :2] + xywh[:, 2:]], 1)
        annos = []
        for i in range(a.images):
            mine, crowd = gt.ann_img == i, gt.ann_crowd != 0
            annos.append(dict(bboxes=xyxy[mine & ~crowd], labels=gt.ann_cat[mine & ~crowd] - 1,
                              bboxes_ignore=xyxy[mine & crowd], labels_ignore=gt.ann_cat[mine & crowd] - 1))
        ds = pkg.CustomBBoxDataset(annos, [str(c) for c in range(80)])

    if a.metric == 'fast-bbox':
        ds = pkg.CocoBBoxDataset(gt)
        ds.flex_gt()

    def score(res):
        if a.metric == 'mAP':
            return ds.evaluate(res, logger='silent')
        if a.metric == 'fast-bbox':
            return {k: float(v) for k, v in ds.evaluate(res, metric='fast-bbox', logger='silent').items()}
        return pkg.evaluate_bbox(res, gt, logger='silent')

    def run(flat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pkg.single_gpu_test(det, loader, flat=flat)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = score(res)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rows = int(res[0].shape[0]) if flat else int(sum(len(c) for r in res for c in r))
        return (t1 - t0, t2 - t1, t2 - t0), out, rows

    forms = (('list', False), ('flat', True))
    warm = {name: run(flat) for name, flat in forms}
    if (a.metric == 'bbox' and warm['list'][1] != warm['flat'][1]) or warm['list'][2] != warm['flat'][2]:
        raise SystemExit(f"the two result forms disagree: {warm['list'][1:]} != {warm['flat'][1:]}")
    rec = {name: [] for name, _ in forms}
    for _ in range(a.passes):
        for name, flat in forms:                          # alternating: both forms see the same drift of the machine
            rec[name].append(run(flat)[0])
    line = dict(tool='val_loop_bench', model='yolov4s', size=a.size, dtype=a.dtype, images=a.images, batch=a.batch,
                passes=a.passes, candidates_per_image=round(per_img, 1), rows=warm['flat'][2],
                metric=a.metric, bbox_mAP=warm['flat'][1].get('bbox_mAP'), mAP=warm['flat'][1].get('mAP'),
                metrics_equal=warm['list'][1] == warm['flat'][1])
    if a.metric == 'mAP':
        line['list_mAP'] = warm['list'][1].get('mAP')
    if a.metric == 'fast-bbox':
        line['report'] = dict(list=warm['list'][1], flat=warm['flat'][1])
        line['max_abs_diff'] = max(abs(warm['list'][1][k] - warm['flat'][1][k]) for k in warm['flat'][1])
    for name, _ in forms:
        t = np.asarray(rec[name])
        line[name] = dict(loop=stats(t[:, 0]), scoring=stats(t[:, 1]), total=stats(t[:, 2]))
    line['flat_over_list_total'] = round(line['flat']['total']['median_ms'] / line['list']['total']['median_ms'], 3)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
