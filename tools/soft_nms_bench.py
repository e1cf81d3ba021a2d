"""Soft-NMS cost on one MI355X: prints one JSON line per measurement.

    python tools/soft_nms_bench.py [--reps 20] [--warmup 5]

1. The post-process stage of the headline plan (YOLOv4-L 608x608 fp32 batch 32, bench.py's head calibration init_head:
   about 2 000 candidates per image): the plan's NMS launch alone on the plan's own buffers (decode re-run before each
   timed launch, its time subtracted), for hard NMS and for soft-NMS linear / gaussian; plus the soft plans' whole step.
2. The split path (uncalibrated head: every (box, class) pair is a candidate): collect_results' yv4_soft_nms_split.
3. The standalone op against the host restatement (tests/_soft_nms_ref.py) at a few sizes.
Times are HIP events around `reps` launches after `warmup`."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bench  # noqa: E402
import mmdet_yolov4_amd as pkg  # noqa: E402

SOFT = {'linear': dict(type='soft_nms', iou_threshold=0.3, method='linear'),
        'gaussian': dict(type='soft_nms', iou_threshold=0.3, method='gaussian', sigma=0.5)}


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


def stage(det, img, nms_cfg, reps, warmup, calibrate):
    det.bbox_head.test_cfg['nms'] = nms_cfg
    det._engines.clear()
    plan = det.compile(img.shape[0], img.shape[2], img.shape[3], device=img.device, rescale=False, graph=False)
    if calibrate:
        bench.init_head(det, plan, img, 2000)
    plan.run(img)
    torch.cuda.synchronize()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    reset = [o for o in plan.ops if o.kind in ('reset', 'topk', 'decode')]
    nms = [o for o in plan.ops if o.kind == 'nms']
    t_dec = timed(lambda: [o.fn(stream) for o in reset], reps, warmup)
    t_all = timed(lambda: [o.fn(stream) for o in reset + nms], reps, warmup)
    t_step = timed(lambda: plan.run(img), reps, warmup)
    counts = plan.post['counts'].cpu().numpy()
    kept = plan.post['count'].cpu().numpy()
    return dict(nms_ms=t_all - t_dec, step_ms=t_step, candidates_mean=float(counts.mean()),
                candidates_max=int(counts.max()), selections_mean=float(kept.mean()), kernel=nms[0].name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg('yolov4l'))
    det.init_weights()
    det = det.to(dev).eval()
    img = torch.randn(a.batch, 3, 608, 608, device=dev) * 0.5
    base = None
    for name, cfg in [('nms', dict(type='nms', iou_threshold=0.65))] + list(SOFT.items()):
        r = stage(det, img, cfg, a.reps, a.warmup, calibrate=True)
        if name == 'nms':
            base = r
        r.update(what='post_stage', nms=name, batch=a.batch, added_ms_vs_hard=r['nms_ms'] - base['nms_ms'],
                 per_step_us=1e3 * r['nms_ms'] / max(r['selections_mean'], 1.0))
        print(json.dumps(r), flush=True)
    # the split path: an uncalibrated head whose every (box, class) pair passes score_thr (1.8 M candidates per image, 80
    # labels of 22 743), 2 images, collection (the per-image yv4_soft_nms_split) timed on the host
    det4 = pkg.build_detector(bench.model_cfg('yolov4l'))
    det4.init_weights()
    with torch.no_grad():
        for conv in det4.bbox_head.convs_pred:
            conv.bias.view(3, 85)[:, 4:] = 0.0
    det4 = det4.to(dev).eval()
    img4 = img[:2].contiguous()
    for name, cfg in SOFT.items():
        det4.bbox_head.test_cfg['nms'] = cfg
        det4._engines.clear()
        plan = det4.compile(2, 608, 608, device=dev, rescale=False, graph=False)
        from mmdet_yolov4_amd.yolocsp_head import collect_results
        plan.run(img4)
        torch.cuda.synchronize()
        counts = plan.post['counts'].cpu().numpy()
        t0 = time.perf_counter()
        collect_results(plan.post, with_nms=True)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) * 1e3 / 2
        print(json.dumps(dict(what='split_path', nms=name, ms_per_image=t, candidates_mean=float(counts.mean()))),
              flush=True)
    # the standalone op against the host restatement
    import _soft_nms_ref as R
    for n in (1000, 5000, 10000):
        rng = np.random.default_rng(n)
        xy = rng.uniform(0, 2000, (n, 2)).astype(np.float32)
        b = np.concatenate([xy, xy + rng.uniform(8, 80, (n, 2)).astype(np.float32)], 1)
        s = rng.uniform(0, 1, n).astype(np.float32)
        bt, st = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
        t_gpu = timed(lambda: pkg.soft_nms(bt, st, 0.3, 0.5, 1e-3, 'linear'), 5, 2)
        t0 = time.perf_counter()
        R.soft_nms_fast(b, s, 0.3, 0.5, 1e-3, 'linear')
        t_host = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(what='standalone', n=n, gpu_ms=t_gpu, host_restatement_ms=t_host)), flush=True)


if __name__ == '__main__':
    main()
