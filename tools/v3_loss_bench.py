"""YOLOV3Head.loss, forward + backward, fused (yv4_yolov3_loss_fwd / _bwd) against the tensor-op path (YV4_FUSED_LOSS=0)
at the recipe shape: 608 x 608, 80 classes, 3 levels of 3 anchors, batch 64, seeded random ground truths (0-14 per
image), for NCHW maps and for the channels-last maps YOLOV3Head.fwd produces.  HIP events around whole steps after a
warm-up: these times include the host's Python enqueue; the kernels' own times come from a kernel trace
(rocprofv3 --kernel-trace --stats, with --fused-only).

Bytes: `map_mb` is the size of the prediction maps (a NOMINAL rate `map_gbs_nominal` divides it by the forward step);
`fwd_mb` / `bwd_mb` count what the dense kernels actually touch, from the batch's assignment: the objectness logit of
every anchor that is not ignored, the whole rows of the positives, the per-anchor id (written forward, read backward)
and -- backward -- one write of every map element.  Channels-last maps hold an anchor's attributes in one 340-byte row,
so there a 4-byte objectness read costs a whole cache line: the counted bytes are a lower bound on that layout's traffic.

    python tools/v3_loss_bench.py [--batch 64] [--steps 10] [--warmup 3] [--composed-steps 3] [--layout both]
                                  [--fused-only] [--json out.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd import yolov3 as V3  # noqa: E402

DEV = 'cuda:0'


def make(batch, size=608, C=80, max_gt=14, seed=0, channels_last=False):
    g = torch.Generator().manual_seed(seed)
    maps = [torch.randn(batch, 3 * (5 + C), size // s, size // s, generator=g).to(DEV) for s in (32, 16, 8)]
    if channels_last:
        maps = [m.contiguous(memory_format=torch.channels_last) for m in maps]
    gts, labels = [], []
    for _ in range(batch):
        k = int(torch.randint(0, max_gt + 1, (1,), generator=g))
        c = torch.rand(k, 2, generator=g) * (size - 1)
        wh = 4 + torch.rand(k, 2, generator=g) * 300
        gts.append(torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, size - 1).to(DEV))
        labels.append(torch.randint(0, C, (k,), generator=g).to(DEV))
    return maps, gts, labels


def head():
    return pkg.YOLOV3Head(
        num_classes=80, in_channels=[8, 8, 8], out_channels=[8, 8, 8],
        loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
        loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'),
        train_cfg=dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0)))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run(a, layout):
    h = head()
    maps, gts, labels = make(a.batch, channels_last=layout == 'channels_last')
    metas = [dict() for _ in gts]
    leaves = [m.clone().requires_grad_(True) for m in maps]
    assert h._fused_loss_ok(leaves)

    def step():
        losses = h.loss(leaves, gts, labels, metas)
        sum(sum(v) for v in losses.values()).backward()
        for p in leaves:
            p.grad = None

    def fwd_only():
        with torch.no_grad():
            V3.v3_fused_loss(h, maps, gts, labels)

    fused = timed(step, a.steps, a.warmup)
    fused_fwd = timed(fwd_only, a.steps, a.warmup)
    res = dict(layout=layout, batch=a.batch, gts=sum(int(g.shape[0]) for g in gts))
    if not a.fused_only:
        os.environ['YV4_FUSED_LOSS'] = '0'
        assert not h._fused_loss_ok(leaves)
        res['composed_ms'] = timed(step, a.composed_steps, 1)
        os.environ.pop('YV4_FUSED_LOSS')
    with torch.no_grad():
        _, assigned = V3.v3_fused_loss(h, maps, gts, labels)
    anchors = assigned.numel()
    live = int((assigned >= 0).sum())
    pos = int((assigned > 0).sum())
    attr = maps[0].shape[1] // 3
    map_bytes = sum(m.numel() for m in maps) * 4
    fwd_bytes = 4 * live + 4 * attr * pos + 4 * anchors
    bwd_bytes = 4 * anchors + 4 * live + 4 * attr * pos + map_bytes
    res.update(positives=pos, negatives=live - pos, anchors=anchors, map_mb=map_bytes / 1e6,
               fwd_mb=fwd_bytes / 1e6, bwd_mb=bwd_bytes / 1e6, fused_ms=fused, fused_fwd_ms=fused_fwd,
               map_gbs_nominal=map_bytes / (fused_fwd * 1e-3) / 1e9)
    if 'composed_ms' in res:
        res['speedup'] = res['composed_ms'] / fused
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--composed-steps', type=int, default=3)
    ap.add_argument('--layout', choices=('nchw', 'channels_last', 'both'), default='both')
    ap.add_argument('--fused-only', action='store_true', help='skip the tensor-op path (kernel-trace runs)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    layouts = ('nchw', 'channels_last') if a.layout == 'both' else (a.layout,)
    out = []
    for layout in layouts:
        out.append(run(a, layout))
        print(json.dumps(out[-1]), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
