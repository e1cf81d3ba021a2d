"""Images/s of the fp8 (e4m3) inference plan against the 16-bit plan of the same detector, in one process on one GPU.

    python tools/fp8_bench.py [--configs v4l,v4s,v5l] [--reps 20] [--warmup 5] [--trials 5]

Configurations: YOLOv4-L 608 batch 32 (bf16), YOLOv4-S 416 batch 256 (fp16, BASELINE configs[3]'s network), YOLOv5-L
640 batch 32 (bf16).  Each detector is random-init, BatchNorm-calibrated and fp8-calibrated on its own batch; both plans
are captured into hipGraphs and timed with HIP events: `warmup` replays, then `trials` windows of `reps` replays,
alternating the two plans window by window.  Reported: median images/s per plan, the spread (min..max) over the windows,
the fp8 / 16-bit ratio.  Per-class kernel times come from one run under `rocprofv3 --kernel-trace --stats`.
Prints one JSON line per configuration.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd.calibrate import calibrate_bn, calibrate_fp8  # noqa: E402

CONFIGS = {'v4l': ('yolov4l', 608, 32, torch.bfloat16), 'v4s': ('yolov4s', 416, 256, torch.float16),
           'v5l': ('yolov5l', 640, 32, torch.bfloat16)}


def _window(plan, img, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        plan.run(img)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, reps, warmup, trials):
    model, size, batch, dt16 = CONFIGS[name]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg(model))
    det.init_weights()
    det.eval().to(dev)
    img = bench.synthetic_images(batch, size, 1000, dev)
    plan = det.compile(batch, size, size, device=dev, rescale=True)
    calibrate_bn(plan, img)
    bench.init_head(det, plan, img, 1500.0)
    det._engines.clear()
    del plan
    calibrate_fp8(det, img[:min(batch, 8)])
    plans = {'h16': det.compile(batch, size, size, device=dev, rescale=True, graph=True, dtype=dt16),
             'fp8': det.compile(batch, size, size, device=dev, rescale=True, graph=True, dtype=torch.float8_e4m3fn)}
    for p in plans.values():
        for _ in range(warmup):
            p.run(img)
    torch.cuda.synchronize()
    ms = {k: [] for k in plans}
    for _ in range(trials):
        for k, p in plans.items():
            ms[k].append(_window(p, img, reps))
    out = dict(config=name, model=model, size=size, batch=batch, dtype16=str(dt16).replace('torch.', ''))
    for k, v in ms.items():
        v = sorted(v)
        out[f'{k}_img_s'] = round(batch * 1000.0 / v[len(v) // 2], 1)
        out[f'{k}_img_s_spread'] = [round(batch * 1000.0 / v[-1], 1), round(batch * 1000.0 / v[0], 1)]
    out['fp8_over_h16'] = round(out['fp8_img_s'] / out['h16_img_s'], 3)
    print(json.dumps(out), flush=True)
    del plans, det
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='v4l,v4s,v5l')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trials', type=int, default=5)
    a = ap.parse_args()
    for c in a.configs.split(','):
        run(c, a.reps, a.warmup, a.trials)


if __name__ == '__main__':
    main()
