"""The fused YOLOCSPHead loss with the IoU / DIoU / CIoU box terms and SoftFocalLoss (csrc/loss.hip:
yv4_yolo_loss_fwd_ex / _bwd_ex) per element against a float64 reference (tests/_loss_variants_ref.py: cases, coverage
conditions -- checked by test_loss_variants_host.py on the CPU --, configurations and the reference).

The C ABI is driven with a ``LossDesc`` plus ``LossOpts``, so that the work buffers can be read back.  Per configuration:
the (L, 3) losses, every positive's objectness target and the whole of every ``draw`` / ``dbias`` against float64
autograd, in the default and in the deterministic mode.

Bound: ``e(kernel) <= 4 * e32 + 8 * 2**-24`` with ``e(x) = max |x - ref64| / max |ref64|`` and ``e32`` the
same measure of the REFERENCE's own float32 evaluation on the CPU.  It comes from the reference, not from what the kernels
reach.
"""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib, ops
from mmdet_yolov4_amd.yolocsp_head import FusedLosses, RawPredMap, loss_options

import _loss_ref as R
import _loss_variants_ref as V

pytestmark = pytest.mark.gpu

BCE = dict(type='CrossEntropyLoss', use_sigmoid=True)


@contextlib.contextmanager
def det_mode(on):
    was = pkg.deterministic()
    pkg.set_deterministic(on)
    try:
        yield
    finally:
        pkg.set_deterministic(was)


def loss_cfg(weight, focal):
    raw = dict(BCE, loss_weight=weight)
    return raw if focal is None else dict(type='SoftFocalLoss', raw_loss=raw, gamma=focal[0], alpha=focal[1])


_heads = {}


def head_for(case, c, dev):
    key = (case.name, c.tag)
    if key not in _heads:
        _heads[key] = pkg.YOLOCSPHead(
            num_classes=case.C if case.C else 5, in_channels=[8] * case.L, featmap_strides=case.strides,
            anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=case.base_sizes, strides=case.strides),
            class_agnostic=case.agnostic, one_hot_smoother=case.smoother,
            loss_bbox=dict(V.BOX_CFG[c.kind], loss_weight=V.W_BBOX), loss_conf=loss_cfg(V.W_CONF, c.conf),
            loss_cls=loss_cfg(V.W_CLS, c.cls)).to(dev).train()
    return _heads[key]


def run_abi(head, case, raws, biases, gout, dev, opts='head'):
    """One forward + backward through the C ABI.  raws: (N, H, W, Cp) NHWC device tensors; biases: (co,) fp32.
    ``opts``: 'head' = the head's ``loss_options`` through the _ex calls; None = yv4_yolo_loss_fwd / _bwd; else a LossOpts."""
    L, A, attr, N, G = case.L, case.A, case.attr, case.N, case.G
    assert head.num_anchors[0] == A and (0 if head.class_agnostic else head.num_classes) == case.C
    d = _lib.LossDesc()
    d.num_levels, d.N, d.A, d.num_classes, d.G = L, N, A, case.C, G
    d.dtype = _lib.DTYPE_CODE[raws[0].dtype]
    TA = 0
    for l in range(L):
        n_, H, W, Cp = raws[l].shape
        assert raws[l].is_contiguous() and (n_, H, W) == (N,) + tuple(case.sizes[l]) and Cp == case.Cp
        lv = d.levels[l]
        lv.raw, lv.bias = raws[l].data_ptr(), biases[l].data_ptr()
        lv.H, lv.W, lv.Cp, lv.stride = H, W, Cp, int(head.featmap_strides[l])
        ba = head.anchor_generator.base_anchors[l].float().cpu()
        for k in range(A):
            for c in range(4):
                lv.base_anchors[k][c] = float(ba[k, c])
        TA += H * W * A
    S = 5 * A * G
    i32 = dict(dtype=torch.int32, device=dev)
    slot_anchor = torch.full((max(L * S, 1),), -7, **i32)
    winner = torch.full((N * TA,), -7, **i32)
    npos = torch.full((L,), -7, **i32)
    conf_t = torch.zeros(max(L * S, 1), dtype=torch.float32, device=dev)
    sums = torch.empty(2, L, 3, dtype=torch.float64, device=dev)
    gt = torch.cat(case.boxes).reshape(-1, 4).to(dev).float().contiguous()
    gt_label = torch.cat(case.labels).to(dev).long().contiguous()
    sizes = [int(b.shape[0]) for b in case.boxes]
    gt_img = torch.repeat_interleave(torch.arange(N), torch.tensor(sizes)).to(dev)
    d.gt, d.gt_label, d.gt_img = gt.data_ptr(), gt_label.data_ptr(), gt_img.data_ptr()
    d.shape_thr, d.smooth, d.ratio = float(head.shape_match_thres), float(head.one_hot_smoother), \
        float(head.conf_iou_loss_ratio)
    d.eps = float(head.loss_bbox.eps)
    d.w_cls, d.w_conf, d.w_bbox = (V.W_CLS if case.C else 0.), V.W_CONF, float(head.loss_bbox_weight)
    d.slot_anchor, d.winner, d.npos, d.conf_t, d.sums = (t.data_ptr() for t in (slot_anchor, winner, npos, conf_t, sums))
    losses = torch.empty(L, 3, dtype=torch.float32, device=dev)
    d.losses = losses.data_ptr()
    o = loss_options(head) if isinstance(opts, str) else opts
    lib = _lib.lib()
    if o is None:
        _lib.check(lib.yv4_yolo_loss_fwd(C.byref(d), ops.stream_ptr()), 'yv4_yolo_loss_fwd')
    else:
        _lib.check(lib.yv4_yolo_loss_fwd_ex(C.byref(d), C.byref(o), ops.stream_ptr()), 'yv4_yolo_loss_fwd_ex')
    gout = gout.to(dev).float().contiguous()
    draws = [torch.full_like(r, float('nan')) for r in raws]           # every element must be WRITTEN
    dbias = [torch.empty(2, A * attr, dtype=torch.float64, device=dev) for _ in range(L)]
    gpos = torch.empty(max(L * S * attr, 1) * (4 if ops.deterministic() else 1), dtype=torch.float32, device=dev)
    for l in range(L):
        d.levels[l].draw, d.levels[l].dbias = draws[l].data_ptr(), dbias[l].data_ptr()
    d.gpos = gpos.data_ptr()
    if o is None:
        _lib.check(lib.yv4_yolo_loss_bwd(C.byref(d), gout.data_ptr(), ops.stream_ptr()), 'yv4_yolo_loss_bwd')
    else:
        _lib.check(lib.yv4_yolo_loss_bwd_ex(C.byref(d), C.byref(o), gout.data_ptr(), ops.stream_ptr()), 'yv4_yolo_loss_bwd_ex')
    torch.cuda.synchronize()
    return SimpleNamespace(losses=losses.cpu(), slot_anchor=slot_anchor[:L * S].view(L, S).cpu(), winner=winner.view(N, TA).cpu(),
                           npos=npos.cpu(), conf_t=conf_t[:L * S].view(L, S).cpu(), draw=[x.cpu() for x in draws],
                           dbias=[b[0].cpu() for b in dbias], TA=TA, S=S)


def run_case(name, tag, dev, dtype=torch.float32, det=False, maps_dtype=None):
    """The case's inputs drawn in ``dtype`` and run through the instantiation for ``maps_dtype`` (default: the same)."""
    maps_dtype = maps_dtype or dtype
    case, inputs, _, _ = V.references(name, tag, dtype)
    raws = [raw.to(dev).to(maps_dtype).contiguous() for raw, _ in inputs]
    biases = [b.to(dev).float().contiguous() for _, b in inputs]
    with det_mode(det):
        return run_abi(head_for(case, V.CONFIGS[tag], dev), case, raws, biases, R.gout_matrix(case.L), dev)


def check_forward(name, out, r64, e32, case, tag):
    e = R.loss_errors(out.losses, r64.losses)
    msgs = []
    for l in range(case.L):
        asg = case.assign[l]
        assert int(out.npos[l]) == asg.slot.numel() and asg.slot.numel() > 0, (name, l)
        for j, key in enumerate(('cls', 'conf', 'bbox')):
            print(R.describe(f'{tag} {name} loss_{key}[{l}]', float(e[l, j]), float(e32.losses[l, j])))
            if not float(e[l, j]) <= R.bound(float(e32.losses[l, j])):
                msgs.append(f'loss_{key}[{l}]: kernel {float(out.losses[l, j])!r} ref64 {float(r64.losses[l, j])!r} e {float(e[l, j]):.3e} > '
                            f'{R.bound(float(e32.losses[l, j])):.3e}')
        ect = R.err(out.conf_t[l][asg.slot], r64.conf_t[l])
        print(R.describe(f'{tag} {name} conf_t[{l}]', ect, e32.conf_t[l]))
        if not ect <= R.bound(e32.conf_t[l]):
            i = int((out.conf_t[l][asg.slot].double() - r64.conf_t[l]).abs().argmax())
            msgs.append(f'conf_t level {l}: e {ect:.3e} > {R.bound(e32.conf_t[l]):.3e}, worst slot (level, k, a, g) = '
                        f'{(l, int(asg.k[i]), int(asg.a[i]), int(asg.g[i]))}')
    assert not msgs, f'{tag} {name}: ' + '; '.join(msgs)


def check_backward(name, out, r64, e32, case, tag):
    msgs = []
    for l in range(case.L):
        draw = out.draw[l].float()
        assert not bool(torch.isnan(draw).any()), f'{tag} {name} level {l}: draw has nan (an element never written, or a nan gradient)'
        if draw[..., case.co:].numel() and float(draw[..., case.co:].abs().max()) != 0:
            msgs.append(f'level {l}: padding channel not zero')
        d = draw[..., :case.co]
        ed = R.err(d, r64.draw[l])
        print(R.describe(f'{tag} {name} draw[{l}]', ed, e32.draw[l]))
        if not ed <= R.bound(e32.draw[l]):
            bad = int((d.double() - r64.draw[l]).abs().argmax())
            n, y, x, ch = [int(v) for v in torch.unravel_index(torch.tensor(bad), d.shape)]
            msgs.append(f'draw level {l}: e {ed:.3e} > {R.bound(e32.draw[l]):.3e}; worst element (n, y, x, anchor, attribute) = '
                        f'{(n, y, x, ch // case.attr, ch % case.attr)}: kernel {float(d.reshape(-1)[bad])!r} ref64 '
                        f'{float(r64.draw[l].reshape(-1)[bad])!r}')
        eb = R.err(out.dbias[l], r64.dbias[l])
        print(R.describe(f'{tag} {name} dbias[{l}]', eb, e32.dbias[l]))
        if not eb <= R.bound(e32.dbias[l]):
            ch = int((out.dbias[l] - r64.dbias[l]).abs().argmax())
            msgs.append(f'dbias level {l}: e {eb:.3e} > {R.bound(e32.dbias[l]):.3e}; worst channel (anchor, attribute) = '
                        f'{divmod(ch, case.attr)}: kernel {float(out.dbias[l][ch])!r} ref64 {float(r64.dbias[l][ch])!r}')
    assert not msgs, f'{tag} {name}: ' + '; '.join(msgs)


def same_bits(a, b):
    ok = torch.equal(a.losses, b.losses) and torch.equal(a.conf_t, b.conf_t) and torch.equal(a.winner, b.winner)
    return ok and all(torch.equal(x, y) for x, y in zip(a.draw, b.draw)) and all(torch.equal(x, y) for x, y in zip(a.dbias, b.dbias))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(V.CONFIGS))
@pytest.mark.parametrize('name', list(V.CASES))
def test_variant_against_float64(name, tag, gpu_device):
    """Losses, objectness targets, draw and dbias of every configuration, default and deterministic mode; two
    deterministic runs give identical bits."""
    case, _, r64, e32 = V.references(name, tag)
    out = run_case(name, tag, gpu_device)
    assert torch.equal(out.winner.long(), R.expected_winner(case))
    check_forward(name, out, r64, e32, case, f'default {tag}')
    check_backward(name, out, r64, e32, case, f'default {tag}')
    det = run_case(name, tag, gpu_device, det=True)
    check_forward(name, det, r64, e32, case, f'det {tag}')
    check_backward(name, det, r64, e32, case, f'det {tag}')
    assert same_bits(det, run_case(name, tag, gpu_device, det=True)), f'{name} {tag}: the deterministic mode does not repeat'


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('tag', ['iou_log', 'diou', 'ciou-conf1.5-cls1.5', 'giou-conf2.0-cls2.0'])
@pytest.mark.parametrize('name', ['v_edges', 'v_nonsquare_agnostic'])
def test_16bit_maps_are_fp32_kernels_plus_one_rounding(name, tag, dtype, gpu_device):
    """The kernels are one template over the map type and compute in fp32: on ``raw.float()`` the fp32 instantiation sees
    the same numbers.  Deterministic mode: losses, conf_t and dbias bit for bit, draw = the fp32 kernel's rounded once;
    and the fp32 kernel on those inputs is within the bound of float64."""
    case, _, r64, e32 = V.references(name, tag, dtype)
    o16 = run_case(name, tag, gpu_device, dtype=dtype, det=True)
    o32 = run_case(name, tag, gpu_device, dtype=dtype, det=True, maps_dtype=torch.float32)
    check_forward(name, o32, r64, e32, case, f'det {tag} {str(dtype)[6:]} as fp32')
    check_backward(name, o32, r64, e32, case, f'det {tag} {str(dtype)[6:]} as fp32')
    assert torch.equal(o16.slot_anchor, o32.slot_anchor) and torch.equal(o16.winner, o32.winner)
    assert torch.equal(o16.conf_t, o32.conf_t) and torch.equal(o16.losses, o32.losses)
    for l in range(case.L):
        assert o16.draw[l].dtype == dtype
        assert torch.equal(o16.dbias[l], o32.dbias[l]), f'{name} {tag} level {l}: dbias differs'
        assert torch.equal(o16.draw[l].view(torch.int16), o32.draw[l].to(dtype).view(torch.int16)), f'{name} {tag} level {l}: draw'


@pytest.mark.parametrize('name', ['nonsquare_tall', 'edges'])
def test_ex_with_default_options_is_the_plain_call(name, gpu_device):
    """``_ex`` with {GIoU, no focal} gives the bits of yv4_yolo_loss_fwd / _bwd in deterministic mode, on existing
    ``_loss_ref`` cases: the GIoU path did not move."""
    dev = gpu_device
    case, inputs, r64, e32 = R.references(name)
    head = pkg.YOLOCSPHead(num_classes=case.C, in_channels=[8] * case.L, featmap_strides=case.strides,
                           anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=case.base_sizes, strides=case.strides),
                           one_hot_smoother=case.smoother).to(dev).train()
    raws = [raw.to(dev).contiguous() for raw, _ in inputs]
    biases = [b.to(dev).float().contiguous() for _, b in inputs]
    with det_mode(True):
        plain = run_abi(head, case, raws, biases, R.gout_matrix(case.L), dev, opts=None)
        ex = run_abi(head, case, raws, biases, R.gout_matrix(case.L), dev, opts=_lib.LossOpts())
        via_head = run_abi(head, case, raws, biases, R.gout_matrix(case.L), dev)
    assert same_bits(plain, ex) and same_bits(plain, via_head)
    check_forward(name, ex, r64, e32, case, 'det ex-default')
    check_backward(name, ex, r64, e32, case, 'det ex-default')


def _module_run(head, case, inputs, dev, fused):
    keys = ('loss_conf', 'loss_bbox') if case.agnostic else ('loss_cls', 'loss_conf', 'loss_bbox')

    def total(fl):
        return sum(w * v for key in keys for w, v in zip(R.WEIGHTS[key], [x.sum() for x in fl[key]]))

    os.environ['YV4_FUSED_LOSS'] = '1' if fused else '0'
    try:
        leaves, maps = [], []
        for raw, bias in inputs:
            r = raw.to(dev).permute(0, 3, 1, 2).requires_grad_(True)        # NCHW view of NHWC storage: channels_last
            b = bias.to(dev).requires_grad_(True)
            leaves.append((r, b))
            maps.append(RawPredMap(r, b, case.A, case.attr))
        fl = head.loss(maps, [b.to(dev) for b in case.boxes], [l.to(dev) for l in case.labels], None)
        assert isinstance(fl, FusedLosses) == fused
        got = torch.stack([torch.stack([(fl[k][l] if k in fl else torch.zeros((), device=dev)).reshape(())
                                        for k in ('loss_cls', 'loss_conf', 'loss_bbox')]) for l in range(case.L)])
        total(fl).backward()
    finally:
        os.environ.pop('YV4_FUSED_LOSS', None)
    return got.detach(), leaves, total


def test_through_the_module_ciou_soft_focal(gpu_device):
    """``head.loss`` + ``backward`` on RawPredMaps with CIoULoss + SoftFocalLoss (both terms) gives the ABI call's tensors
    bit for bit in deterministic mode, and equals the tensor-op path (YV4_FUSED_LOSS=0) under the bound."""
    dev = gpu_device
    name, tag = 'v_dups', 'ciou-conf1.5-cls1.5'
    case, inputs, r64, e32 = V.references(name, tag)
    head = head_for(case, V.CONFIGS[tag], dev)
    assert type(head.loss_bbox).__name__ == 'CIoULoss' and type(head.loss_conf).__name__ == 'SoftFocalLoss'
    bal = torch.tensor([[1.0, float(head.conf_level_balance_weight[l]), 1.0] for l in range(case.L)], device=dev)
    with det_mode(True):
        got, leaves, total = _module_run(head, case, inputs, dev, fused=True)
        leaf = torch.zeros(case.L, 3, device=dev, requires_grad=True)
        total(FusedLosses(leaf * bal, None, with_cls=True)).backward()
        raws = [raw.to(dev).contiguous() for raw, _ in inputs]
        biases = [b.to(dev).float().contiguous() for _, b in inputs]
        out = run_abi(head, case, raws, biases, leaf.grad, dev)
    assert torch.equal(got.cpu(), (out.losses.to(dev) * bal).cpu())
    for l, (r, b) in enumerate(leaves):
        assert torch.equal(r.grad.permute(0, 2, 3, 1).cpu(), out.draw[l]), f'{name} level {l}: draw'
        assert torch.equal(b.grad.cpu(), out.dbias[l].float()), f'{name} level {l}: dbias'
    ref, ref_leaves, _ = _module_run(head, case, inputs, dev, fused=False)
    balc = bal.cpu()
    e = R.loss_errors(got.cpu() / balc, ref.cpu() / balc)
    for l in range(case.L):
        for j in range(3):
            print(R.describe(f'fused vs tensor-op loss[{l},{j}]', float(e[l, j]), float(e32.losses[l, j])))
            assert float(e[l, j]) <= R.bound(float(e32.losses[l, j])), (l, j, float(e[l, j]))
        scale = float(bal[l, 1])          # the module's upstream gradient carries the level balance on the objectness term
        for what, a, b, e_ in (('draw', leaves[l][0].grad.permute(0, 2, 3, 1)[..., :case.co], ref_leaves[l][0].grad.permute(0, 2, 3, 1)[..., :case.co], e32.draw[l]),
                               ('dbias', leaves[l][1].grad, ref_leaves[l][1].grad, e32.dbias[l])):
            ee = R.err(a.cpu(), b.cpu())
            print(R.describe(f'fused vs tensor-op {what}[{l}] (balance {scale})', ee, e_))
            assert ee <= R.bound(e_), (what, l, ee)


def test_one_training_step_with_ciou(golden, gpu_device):
    """A tiny YOLOv4 detector with ``loss_bbox=CIoULoss`` trains through the recipe's hooks (warm-up, EMA, the fp16
    gradient-accumulating optimizer hook): the fused kernels produced the loss with the CIoU box term, the loss is
    finite and the weights move."""
    import numpy as np
    from conftest import arch_from, state_dict_from
    from mmdet_yolov4_amd import hooks as H
    from mmdet_yolov4_amd.optim import build_optimizer
    g = golden('train_v4')
    stages, reps, chans = arch_from(g)
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[stages, reps, chans], out_indices=[3, 4, 5]),
        neck=dict(type='YOLOV4Neck', in_channels=[32, 64, 64], out_channels=[32, 64, 128], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=[32, 64, 128],
                       loss_bbox=dict(type='CIoULoss', loss_weight=3.2)), train_cfg=None,
        test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=300)))
    det.load_state_dict(state_dict_from(g), strict=True)
    det.to(gpu_device)
    seen = []
    orig = det.bbox_head._loss_fused

    def spy(*a, **k):
        seen.append(loss_options(det.bbox_head).box_kind)
        return orig(*a, **k)
    det.bbox_head._loss_fused = spy
    img = torch.from_numpy(g['img']).to(gpu_device)
    data = dict(img=img, img_metas=[dict(), dict()],
                gt_bboxes=[torch.from_numpy(g['gt_bboxes0']).to(gpu_device), torch.from_numpy(g['gt_bboxes1']).to(gpu_device)],
                gt_labels=[torch.from_numpy(g['gt_labels0']).to(gpu_device), torch.from_numpy(g['gt_labels1']).to(gpu_device)])
    opt = build_optimizer(det, dict(type='SGD', lr=0.01, momentum=0.937, weight_decay=0.0005, nesterov=True,
                                    paramwise_cfg=dict(bias_decay_mult=0., norm_decay_mult=0.)))
    before = {k: v.detach().clone() for k, v in det.state_dict().items() if k.endswith('conv.weight')}
    runner = H.Runner(det, opt, max_epochs=2)
    runner.register_hook_from_cfg(dict(type='DetailedLinearWarmUpHook', warmup_iters=4, priority='NORMAL'))
    runner.register_hook_from_cfg(dict(type='StateEMAHook', momentum=0.9, interval=1, warm_up=2, priority='HIGH'))
    runner.register_hook(H.Fp16GradAccumulateOptimizerHook(accumulation=1, grad_clip=dict(max_norm=35, norm_type=2),
                                                           loss_scale='dynamic'), 'ABOVE_NORMAL')
    losses = []

    class Rec(H.Hook):
        def after_train_iter(self, r):
            losses.append(r.outputs['log_vars']['loss'])
    runner.register_hook(Rec(), 'LOWEST')
    runner.run(H.BatchSource([data] * 6, 2))        # (the dynamic loss scale skips the first steps while it backs off)
    torch.cuda.synchronize()
    assert seen and all(k == _lib.BOX_CIOU for k in seen), 'the fused loss with the CIoU term did not run'
    assert len(losses) == 12 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    after = det.state_dict()
    moved = sum(int(not torch.equal(v, after[k])) for k, v in before.items())
    assert moved >= len(before) // 2, (moved, len(before))
    assert all(bool(torch.isfinite(after[k]).all()) for k in before)
