"""Test-time augmentation step time of YOLOv3-DarkNet53 (80 classes): img_scale=[(608, 608), (416, 416)] with
flip=True (4 augmentations) against 4 separate ``simple_test`` plans, in one process on one GPU.

    python tools/tta_bench.py [--batches 1,8] [--dtypes fp32,bf16] [--reps 20] [--warmup 5]

Random-init detector (class logits shrunk and shifted; the number of (box, class) pairs of image 0 that pass score_thr
is reported: with random weights it is large, so the merged NMS takes the split path, which collection runs outside
the timings), a 480 x 640 source image.  Every plan is captured into a hipGraph and timed with HIP events over `reps` replays after
`warmup`.  Reported per (batch, dtype): the TTA plan's ms per step; the sum of the four simple_test plans' ms (each
with its own decode + NMS); their ratio; and the post-network part of the TTA plan (decode, top-k, slot tables,
merge, NMS) timed by launching those ops alone on the same buffers.  Prints one JSON line per configuration.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mmdet_yolov4_amd as pkg  # noqa: E402

SCALES = [(608, 608), (416, 416)]
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
POST_KINDS = ('decode', 'topk', 'slots', 'merge', 'nms')


def detector(dev):
    torch.manual_seed(0)
    det = pkg.build_detector(dict(
        type='YOLOV3', backbone=dict(type='Darknet', depth=53, out_indices=(3, 4, 5)),
        neck=dict(type='YOLOV3Neck', num_scales=3, in_channels=[1024, 512, 256], out_channels=[512, 256, 128]),
        bbox_head=dict(type='YOLOV3Head', num_classes=80, in_channels=[512, 256, 128], out_channels=[1024, 512, 256]),
        test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, conf_thr=0.005,
                      nms=dict(type='nms', iou_threshold=0.45), max_per_img=100)))
    with torch.no_grad():
        for conv in det.bbox_head.convs_pred:          # class logits shrunk and shifted
            conv.weight.view(3, 85, -1)[:, 5:].mul_(0.1)
            conv.bias.view(3, 85)[:, 5:].normal_(-5.0, 0.5)
    return det.to(dev).eval()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(det, dev, N, dtype, reps, warmup):
    pipe = pkg.FusedTestPipeline(img_scale=SCALES, size_divisor=32, mean=(0, 0, 0), std=(255, 255, 255), to_rgb=True,
                                 pad_before_normalize=False, device=dev, flip=True)
    src = np.random.default_rng(0).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    batches, metas = pipe([src] * N)
    geos = [tuple(b.shape[2:]) for b in batches]
    flips = [pkg.tta.flip_code(m[0]) for m in metas]
    tta = det.compile_tta(N, geos, flips, device=dev, graph=True, dtype=dtype)
    pkg.tta.set_tta_metas(tta.post, metas)
    inputs = [torch.cat([batches[a] for a in augs]) for augs in tta.tta_groups]
    t_tta = timed(lambda: tta.run(*inputs), reps, warmup)
    singles = []
    for b, m in zip(batches, metas):
        p = det.compile(N, b.shape[2], b.shape[3], device=dev, rescale=True, graph=True, dtype=dtype)
        pkg.yolocsp_head.set_scale_factors(p.post, m, True)
        singles.append((p, b))
    t_single = sum(timed(lambda p=p, b=b: p.run(b), reps, warmup) for p, b in singles)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    post_ops = [o for o in tta.ops if o.kind in POST_KINDS]
    t_post = timed(lambda: [o.fn(stream) for o in post_ops], reps, warmup)
    dets = pkg.tta.collect_tta(tta.post, metas, True, 80)
    return dict(metric='tta_step_ms', batch=N, dtype=str(dtype).replace('torch.', ''), augs=len(flips),
                groups=len(tta.tta_groups), tta_ms=round(t_tta, 3), four_simple_test_ms=round(t_single, 3),
                tta_over_simple=round(t_tta / t_single, 3), post_ms=round(t_post, 3),
                post_share=round(t_post / t_tta, 3), slots_total=tta.post['S_total'],
                candidates_img0=int(tta.post['counts'][0]), dets_img0=int(sum(len(c) for c in dets[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8')
    ap.add_argument('--dtypes', default='fp32,bf16')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    det = detector(dev)
    with torch.no_grad():
        for dt in a.dtypes.split(','):
            for n in a.batches.split(','):
                print(json.dumps(run(det, dev, int(n), DTYPES[dt], a.reps, a.warmup)), flush=True)


if __name__ == '__main__':
    main()
