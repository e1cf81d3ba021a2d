#!/usr/bin/env python
"""Rate of the fused YOLOv3 mstrain input pipeline (csrc/augment_v3.hip) at the recipe's sizes: COCO-sized u8 sources ->
PhotoMetricDistortion, Expand, MinIoURandomCrop, Resize to a per-image scale in [(320, 320), (608, 608)], flip, normalise,
Pad(32), collate -> (N, 3, Hmax, Wmax) fp32.
    python tools/v3_aug_bench.py [--batch 32] [--steps 30] [--cpu-samples 4]
Reports the kernel's device time per batch (HIP events around launches on prepared descriptors) with the bytes it must
move (u8 source bytes + fp32 output bytes) against the HBM figures DESIGN uses, the host's time for the draws, the box chain
and the descriptors separately, the wall-clock rate of whole calls, and the numpy restatement (tests/_v3_aug_ref.py, one
core) on a few samples as the CPU yardstick."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd.augment_v3 import FusedV3TrainPipeline
from mmdet_yolov4_amd.ops import stream_ptr

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.3e12          # MI355X_MICROARCH's spec / measured stream figure

V3_TRAIN_PIPELINE = [     # configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78
    dict(type='LoadImageFromFile', to_float32=True), dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion'),
    dict(type='Expand', mean=[0, 0, 0], to_rgb=True, ratio_range=(1, 2)),
    dict(type='MinIoURandomCrop', min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9), min_crop_size=0.3),
    dict(type='Resize', img_scale=[(320, 320), (608, 608)], keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True),
    dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--pool', type=int, default=64, help='distinct source images resident on the device')
    ap.add_argument('--cpu-samples', type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU (there is no CPU fallback)'
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    h, w = a.height, a.width
    pool = []
    for _ in range(a.pool):
        k = rng.randint(1, 15)
        xy = rng.rand(k, 2) * [w * 0.7, h * 0.7]
        wh = rng.rand(k, 2) * [w * 0.3, h * 0.3] + 8
        b = np.concatenate([xy, np.minimum(xy + wh, [w, h])], 1).astype(np.float32)
        pool.append((torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev), b,
                     rng.randint(0, 80, k).astype(np.int64)))
    pipe = pkg.build_train_pipeline(V3_TRAIN_PIPELINE)
    assert isinstance(pipe, FusedV3TrainPipeline)
    draw = np.random.RandomState(1)

    def batch():
        return [pool[i] for i in rng.randint(0, a.pool, a.batch)]
    # ---- whole calls, wall clock (draws + boxes + descriptors + uploads + launch), closed by a synchronise
    for _ in range(3):
        out = pipe(batch(), rng=draw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = pipe(batch(), rng=draw)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps
    # ---- host shares, each timed alone over the same batches
    batches = [batch() for _ in range(a.steps)]
    t0 = time.perf_counter()
    params = [[pipe.draw_params(draw, h, w, s[1]) for s in bt] for bt in batches]
    t_draw = (time.perf_counter() - t0) / a.steps
    t0 = time.perf_counter()
    for bt, ps in zip(batches, params):
        for s, p in zip(bt, ps):
            pipe.transform_boxes(p, h, w, s[1], s[2])
    t_boxes = (time.perf_counter() - t0) / a.steps
    t0 = time.perf_counter()
    tables = []
    for bt, ps in zip(batches, params):
        table = (_lib.V3AugImage * a.batch)()
        for n, (s, p) in enumerate(zip(bt, ps)):
            table[n] = pipe.describe(s[0], p)
        tables.append(bytes(table))
    t_desc = (time.perf_counter() - t0) / a.steps
    # ---- the kernel alone: prepared descriptor tables, HIP events around the launches
    L = _lib.lib()
    mean, std = pipe.mean.ctypes.data, pipe.std.ctypes.data
    work, out_bytes, src_bytes = [], 0, 0
    for tb, ps in zip(tables, params):
        Hm = max(pipe.pad_shape(p)[0] for p in ps)
        Wm = max(pipe.pad_shape(p)[1] for p in ps)
        d_table = torch.frombuffer(bytearray(tb), dtype=torch.uint8).to(dev)
        work.append((d_table, torch.empty((a.batch, 3, Hm, Wm), dtype=torch.float32, device=dev), Hm, Wm))
        out_bytes += a.batch * 3 * Hm * Wm * 4
        src_bytes += a.batch * h * w * 3
    def launches():
        for d_table, img, Hm, Wm in work:
            _lib.check(L.yv4_v3_augment_u8(d_table.data_ptr(), a.batch, img.data_ptr(), Hm, Wm, mean, std, int(pipe.to_rgb),
                                           stream_ptr()), 'yv4_v3_augment_u8')
    launches()
    torch.cuda.synchronize()
    reps = 5
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launches()
    e1.record()
    torch.cuda.synchronize()
    dev_s = e0.elapsed_time(e1) / 1e3 / (reps * a.steps)
    moved = (out_bytes + src_bytes) / a.steps
    res = dict(metric='images/sec (YOLOv3 mstrain input pipeline: distort + expand + crop + resize + flip + normalise + pad, '
                      'whole calls)', value=round(a.batch / wall, 1), unit='images/sec', batch=a.batch, source=[h, w],
               ms_per_batch_wall=round(wall * 1e3, 3), device_ms_per_batch=round(dev_s * 1e3, 4),
               device_images_per_sec=round(a.batch / dev_s, 1),
               host_ms_per_batch=dict(draws=round(t_draw * 1e3, 3), boxes=round(t_boxes * 1e3, 3),
                                      descriptors=round(t_desc * 1e3, 3)),
               bytes_per_batch=dict(source_u8=src_bytes // a.steps, output_fp32=out_bytes // a.steps),
               achieved_tb_per_s=round(moved / dev_s / 1e12, 3), share_of_hbm_spec=round(moved / dev_s / HBM_SPEC, 3),
               share_of_hbm_measured=round(moved / dev_s / HBM_MEASURED, 3),
               mean_output_hw=[round(float(np.mean([wk[2] for wk in work])), 1), round(float(np.mean([wk[3] for wk in work])), 1)],
               mean_boxes_per_image=round(float(np.mean([len(b) for b in out['gt_bboxes']])), 1))
    if a.cpu_samples:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import _v3_aug_ref as R                                     # the CPU yardstick (test infrastructure)
        cs = [(s[0].cpu().numpy(), p) for s, p in list(zip(batches[0], params[0]))[:a.cpu_samples]]
        t0 = time.perf_counter()
        for src, p in cs:
            R.pipeline(src, p, pipe.mean, pipe.std, pipe.to_rgb, pipe.size_divisor, pipe.expand_fill)
        res['cpu_baseline'] = dict(value=round(len(cs) / (time.perf_counter() - t0), 2), unit='images/sec', cores=1,
                                   kind='port', sample=f'{len(cs)} samples through tests/_v3_aug_ref.py (numpy float32)')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
