"""YOLOCSPHead loss, forward + backward, for every box loss (GIoU, IoU linear / log, DIoU, CIoU) with and without
SoftFocalLoss, at the batch-64 YOLOv4-L 608 bf16 training shapes: maps (64, 256, 76 / 38 / 19) channels-last bf16
(255 channels + 1 of padding), bench.py's synthetic ground truths (Poisson(12) boxes per image).

Two measurements per configuration, both under HIP events around a window of whole steps after a warm-up:

  abi     yv4_yolo_loss_fwd_ex + yv4_yolo_loss_bwd_ex on preallocated buffers (a dozen launches per step: the kernels and
          their memsets, next to no host work).  ``plain`` is yv4_yolo_loss_fwd / _bwd on the same buffers; the windows of
          ``plain`` and of GIoU through ``_ex`` alternate, and every window is repeated: min / median / max are reported,
          so the run-to-run spread is visible next to every difference.
  module  ``head.loss`` + ``backward`` on RawPredMaps, fused against the tensor-op path (YV4_FUSED_LOSS=0) of the SAME
          configuration; these times include the host's Python enqueue.

``--plain-only`` times the plain entry points alone: with ``YV4_LIB_PATH`` pointing at a build of the parent commit (which
has no ``_ex`` calls) this is the parent's number on the same box, for the same-box comparison.

    python tools/loss_variants_bench.py [--batch 64] [--steps 300] [--warmup 30] [--repeats 7] [--module-steps 5]
                                        [--plain-only] [--json profiles/loss_variants_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd import _lib, ops  # noqa: E402
from mmdet_yolov4_amd.yolocsp_head import RawPredMap  # noqa: E402

DEV = 'cuda:0'
BCE = dict(type='CrossEntropyLoss', use_sigmoid=True)
BOX = dict(giou=dict(type='GIoULoss'), iou_linear=dict(type='IoULoss', linear=True), iou_log=dict(type='IoULoss'),
           diou=dict(type='DIoULoss'), ciou=dict(type='CIoULoss'))


def synthetic_gts(batch, size, seed):
    """bench.py's ``synthetic_gts``."""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    lo, hi = torch.log(torch.tensor(8.0)), torch.log(torch.tensor(400.0))
    for _ in range(batch):
        n = max(1, int(torch.poisson(torch.tensor(12.0), generator=g)))
        c = torch.rand(n, 2, generator=g) * size
        wh = torch.exp(torch.rand(n, 2, generator=g) * (hi - lo) + lo)
        boxes.append(torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, size).to(DEV))
        labels.append(torch.randint(0, 80, (n,), generator=g).to(DEV))
    return boxes, labels


def make_head(kind, focal):
    def bce(w):
        raw = dict(BCE, loss_weight=w)
        return dict(type='SoftFocalLoss', raw_loss=raw, gamma=focal, alpha=0.25) if focal else raw
    return pkg.YOLOCSPHead(num_classes=80, in_channels=[8, 8, 8], loss_bbox=dict(BOX[kind], loss_weight=3.2),
                           loss_conf=bce(64.), loss_cls=bce(32.)).to(DEV).train()


def make_maps(batch, size, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    raws, biases = [], []
    for s in (8, 16, 32):
        raw = (torch.randn(batch, size // s, size // s, 256, generator=g) * 1.5).to(DEV).to(dtype)     # NHWC storage
        raws.append(raw)
        biases.append((torch.randn(255, generator=g) * 0.5).to(DEV))
    return raws, biases


class AbiCall:
    """The descriptor ``YoloLossFunction`` builds, on buffers allocated once."""

    def __init__(self, head, raws, biases, boxes, labels):
        L, A, attr = 3, 3, 85
        N = raws[0].shape[0]
        gt = torch.cat(boxes).float().contiguous()
        G = gt.shape[0]
        d = _lib.LossDesc()
        d.num_levels, d.N, d.A, d.num_classes, d.G = L, N, A, 80, G
        d.dtype = _lib.DTYPE_CODE[raws[0].dtype]
        TA = 0
        keep = [gt]
        for l in range(L):
            _, H, W, Cp = raws[l].shape
            lv = d.levels[l]
            draw = torch.empty_like(raws[l])
            dbias = torch.empty(2, A * attr, dtype=torch.float64, device=DEV)
            keep += [draw, dbias]
            lv.raw, lv.bias, lv.draw, lv.dbias = raws[l].data_ptr(), biases[l].data_ptr(), draw.data_ptr(), dbias.data_ptr()
            lv.H, lv.W, lv.Cp, lv.stride = H, W, Cp, int(head.featmap_strides[l])
            ba = head.anchor_generator.base_anchors[l].float().cpu()
            for k in range(A):
                for c in range(4):
                    lv.base_anchors[k][c] = float(ba[k, c])
            TA += H * W * A
        S = 5 * A * G
        i32 = dict(dtype=torch.int32, device=DEV)
        bufs = [torch.empty(L * S, **i32), torch.empty(N * TA, **i32), torch.empty(L, **i32),
                torch.empty(L * S, dtype=torch.float32, device=DEV), torch.empty(2, L, 3, dtype=torch.float64, device=DEV)]
        label = torch.cat(labels).long().contiguous()
        img = torch.repeat_interleave(torch.arange(N), torch.tensor([int(b.shape[0]) for b in boxes])).to(DEV)
        gpos = torch.empty(L * S * attr * 4, dtype=torch.float32, device=DEV)
        self.losses = torch.empty(L, 3, dtype=torch.float32, device=DEV)
        self.gout = torch.ones(L, 3, dtype=torch.float32, device=DEV)
        d.gt, d.gt_label, d.gt_img = gt.data_ptr(), label.data_ptr(), img.data_ptr()
        d.shape_thr, d.smooth, d.ratio, d.eps = 4.0, 0.0, 1.0, 1e-6
        d.w_cls, d.w_conf, d.w_bbox = 32., 64., 3.2
        d.slot_anchor, d.winner, d.npos, d.conf_t, d.sums = (t.data_ptr() for t in bufs)
        d.gpos, d.losses = gpos.data_ptr(), self.losses.data_ptr()
        self.d, self.keep, self.positives = d, keep + bufs + [label, img, gpos, raws, biases], None
        self.G, self.boxes = G, N * TA

    def step(self, opts):
        lib, s = _lib.lib(), ops.stream_ptr()
        if opts is None:
            rc = lib.yv4_yolo_loss_fwd(C.byref(self.d), s) or lib.yv4_yolo_loss_bwd(C.byref(self.d), self.gout.data_ptr(), s)
        else:
            rc = lib.yv4_yolo_loss_fwd_ex(C.byref(self.d), C.byref(opts), s) or \
                lib.yv4_yolo_loss_bwd_ex(C.byref(self.d), C.byref(opts), self.gout.data_ptr(), s)
        _lib.check(rc, 'yolo loss')


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3          # us per step


def stats(xs):
    return dict(min_us=min(xs), median_us=statistics.median(xs), max_us=max(xs),
                spread_pct=100.0 * (max(xs) - min(xs)) / statistics.median(xs), windows=len(xs))


def options(kind, focal):
    o = _lib.LossOpts()
    o.box_kind = list(BOX).index(kind)
    if focal:
        o.conf_focal = o.cls_focal = 1
        o.conf_gamma = o.cls_gamma = focal
        o.conf_alpha = o.cls_alpha = 0.25
    return o


def module_times(head, raws, biases, boxes, labels, steps):
    maps, leaves = [], []
    for raw, bias in zip(raws, biases):
        r = raw.permute(0, 3, 1, 2).requires_grad_(True)
        b = bias.clone().requires_grad_(True)
        leaves += [r, b]
        maps.append(RawPredMap(r, b, 3, 85))

    def step():
        out = head.loss(maps, boxes, labels, None)
        sum(sum(x.sum() for x in v) for k, v in out.items() if k.startswith('loss')).backward()
        for p in leaves:
            p.grad = None

    res = {}
    for name, env, n in (('fused', '1', 4 * steps), ('tensor_op', '0', steps)):
        os.environ['YV4_FUSED_LOSS'] = env
        assert head._fused_loss_ok(maps) == (env == '1')
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        res[name + '_us'] = statistics.median(window(step, n) for _ in range(3))
    os.environ.pop('YV4_FUSED_LOSS')
    res['speedup'] = res['tensor_op_us'] / res['fused_us']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--module-steps', type=int, default=5)
    ap.add_argument('--plain-only', action='store_true', help='yv4_yolo_loss_fwd / _bwd alone (a parent-commit library)')
    ap.add_argument('--json', default=os.path.join('profiles', 'loss_variants_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    boxes, labels = synthetic_gts(a.batch, a.size, 0)
    raws, biases = make_maps(a.batch, a.size, torch.bfloat16)
    call = AbiCall(make_head('giou', None), raws, biases, boxes, labels)
    out = dict(batch=a.batch, size=a.size, dtype='bf16', G=call.G, anchor_boxes=call.boxes, steps=a.steps, repeats=a.repeats,
               lib=os.environ.get('YV4_LIB_PATH', 'in-tree'), has_loss_ex=_lib.has('loss_ex'))
    for _ in range(a.warmup):
        call.step(None)
    torch.cuda.synchronize()
    if a.plain_only or not _lib.has('loss_ex'):
        out['plain'] = stats([window(lambda: call.step(None), a.steps) for _ in range(a.repeats)])
        print(json.dumps(out['plain']), flush=True)
    else:
        giou = options('giou', None)
        for _ in range(a.warmup):
            call.step(giou)
        plain, ex = [], []
        for _ in range(a.repeats):                          # alternating windows of the two entry points
            plain.append(window(lambda: call.step(None), a.steps))
            ex.append(window(lambda: call.step(giou), a.steps))
        out['plain'], base = stats(plain), stats(ex)
        out['abi'], out['module'] = {}, {}
        for kind in BOX:
            for focal in (None, 1.5, 2.0):
                tag = kind + (f'+focal{focal}' if focal else '')
                o = options(kind, focal)
                for _ in range(a.warmup):
                    call.step(o)
                torch.cuda.synchronize()
                st = base if tag == 'giou' else stats([window(lambda: call.step(o), a.steps) for _ in range(a.repeats)])
                st['ratio_to_giou'] = st['median_us'] / base['median_us']
                out['abi'][tag] = st
                if focal != 2.0:
                    out['module'][tag] = module_times(make_head(kind, focal), raws, biases, boxes, labels, a.module_steps)
                print(tag, json.dumps(st), json.dumps(out['module'].get(tag)), flush=True)
        out['ex_giou_over_plain'] = base['median_us'] / out['plain']['median_us']
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(plain=out['plain'], ex_giou_over_plain=out.get('ex_giou_over_plain'))))


if __name__ == '__main__':
    main()
