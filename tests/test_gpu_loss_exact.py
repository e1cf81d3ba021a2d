"""The fused YOLOCSPHead loss (csrc/loss.hip: yv4_yolo_loss_fwd / _bwd) per element against a float64 reference, at the
sizes and edges where the kernels take their real paths (tests/_loss_ref.py: cases, coverage conditions, reference).

The C ABI is driven with a ``LossDesc`` built the way ``YoloLossFunction.forward`` builds it, so that the work buffers
(``slot_anchor``, ``winner``, ``npos``, ``conf_t``) can be read back:

  a. the assignment's integer outputs equal the oracle's ``responsible_indices`` lists, exactly and in order;
  b. the (L, 3) losses and every positive's objectness target against float64;
  c. the whole of every ``draw`` / ``dbias`` against float64 autograd;
  d. 16-bit maps are the fp32 kernels plus one rounding (bit for bit where no float atomic meets another);
  e. the deterministic mode: b. and c. under the same bounds, and identical bits from run to run;
  f. ``head.loss`` + ``backward`` on ``RawPredMap``s gives the ABI call's tensors.

Bound: with ``e(x) = max |x - ref64| / max |ref64|`` and ``e32`` the same measure of the REFERENCE's own
float32 evaluation on the CPU, ``e(kernel) <= 4 * e32 + 8 * 2**-24``.  It comes from the reference, not from what the
kernels achieve.
"""
import contextlib
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib, ops
from mmdet_yolov4_amd.yolocsp_head import RawPredMap

import _loss_ref as R

pytestmark = pytest.mark.gpu

ALL = list(R.CASES)
SIXTEEN = [(torch.bfloat16, 4e-3, 2.0 ** -8), (torch.float16, 1e-3, 2.0 ** -11)]   # dtype, the old file's bound, half an ulp


@contextlib.contextmanager
def det_mode(on):
    was = pkg.deterministic()
    pkg.set_deterministic(on)
    try:
        yield
    finally:
        pkg.set_deterministic(was)


_heads = {}


def head_for(case, dev):
    if case.name not in _heads:
        _heads[case.name] = pkg.YOLOCSPHead(
            num_classes=case.C if case.C else 5, in_channels=[8] * case.L, featmap_strides=case.strides,
            anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=case.base_sizes, strides=case.strides),
            class_agnostic=case.agnostic, one_hot_smoother=case.smoother).to(dev).train()
    return _heads[case.name]


def run_abi(head, case, raws, biases, gout, dev):
    """One forward + backward through the C ABI.  raws: (N, H, W, Cp) NHWC device tensors; biases: (co,) fp32."""
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
    d.w_cls = float(head.loss_cls.loss_weight) if case.C else 0.
    d.w_conf, d.w_bbox = float(head.loss_conf.loss_weight), float(head.loss_bbox_weight)
    d.slot_anchor, d.winner, d.npos, d.conf_t, d.sums = (t.data_ptr() for t in (slot_anchor, winner, npos, conf_t, sums))
    losses = torch.empty(L, 3, dtype=torch.float32, device=dev)
    d.losses = losses.data_ptr()
    _lib.check(_lib.lib().yv4_yolo_loss_fwd(C.byref(d), ops.stream_ptr()), 'yv4_yolo_loss_fwd')
    gout = gout.to(dev).float().contiguous()
    draws = [torch.full_like(r, float('nan')) for r in raws]           # every element must be WRITTEN
    dbias = [torch.empty(2, A * attr, dtype=torch.float64, device=dev) for _ in range(L)]
    gpos = torch.empty(max(L * S * attr, 1) * (4 if ops.deterministic() else 1), dtype=torch.float32, device=dev)
    for l in range(L):
        d.levels[l].draw, d.levels[l].dbias = draws[l].data_ptr(), dbias[l].data_ptr()
    d.gpos = gpos.data_ptr()
    _lib.check(_lib.lib().yv4_yolo_loss_bwd(C.byref(d), gout.data_ptr(), ops.stream_ptr()), 'yv4_yolo_loss_bwd')
    torch.cuda.synchronize()
    return SimpleNamespace(losses=losses.cpu(), slot_anchor=slot_anchor[:L * S].view(L, S).cpu(), winner=winner.view(N, TA).cpu(),
                           npos=npos.cpu(), conf_t=conf_t[:L * S].view(L, S).cpu(), draw=[x.cpu() for x in draws],
                           dbias=[b[0].cpu() for b in dbias], TA=TA, S=S)


_runs = {}


def run_case(name, dev, dtype=torch.float32, det=False, maps_dtype=None, fresh=False):
    """The case's inputs drawn in ``dtype`` and run through the instantiation for ``maps_dtype`` (default: the same);
    ``maps_dtype=float32`` with a 16-bit ``dtype`` is the fp32 kernel on ``raw.float()``."""
    maps_dtype = maps_dtype or dtype
    key = (name, dtype, det, maps_dtype)
    if fresh or key not in _runs:
        case, inputs, _, _ = R.references(name, dtype)
        raws = [raw.to(dev).to(maps_dtype).contiguous() for raw, _ in inputs]
        biases = [b.to(dev).float().contiguous() for _, b in inputs]
        with det_mode(det):
            out = run_abi(head_for(case, dev), case, raws, biases, R.gout_matrix(case.L), dev)
        if fresh:
            return out
        _runs[key] = out
    return _runs[key]


def where(case, l, flat_index, shape):
    """(level, n, y, x, anchor, attribute) of a flat index into a (N, H, W, channels) tensor."""
    n, y, x, c = [int(v) for v in torch.unravel_index(torch.tensor(flat_index), shape)]
    return (l, n, y, x, c // case.attr, c % case.attr) if c < case.co else (l, n, y, x, 'pad', c)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_assignment_exact(name, gpu_device):
    """a. slot_anchor / npos / winner against ``responsible_indices``: no tolerance."""
    case = R.get_case(name)
    out = run_case(name, gpu_device)
    A, G = case.A, case.G
    imgs = torch.repeat_interleave(torch.arange(case.N), torch.tensor([int(b.shape[0]) for b in case.boxes]))
    for l, asg in enumerate(case.assign):
        slots = (out.slot_anchor[l] >= 0).nonzero().reshape(-1)
        g = slots % G if G else slots
        got = torch.stack([imgs[g], out.slot_anchor[l][slots].long(), g, slots], 1) if G else torch.zeros(0, 4, dtype=torch.long)
        want = torch.stack([asg.img, asg.anchor, asg.g, asg.slot], 1)
        n = min(got.shape[0], want.shape[0])
        diff = (got[:n] != want[:n]).any(1).nonzero().reshape(-1)
        if diff.numel() or got.shape[0] != want.shape[0]:
            i = int(diff[0]) if diff.numel() else n
            s = int(got[i, 3]) if i < got.shape[0] else int(want[i, 3])
            raise AssertionError(f'{name}: first differing slot (level, k, a, g) = {(l, s // (A * G), (s // G) % A, s % G)}: kernel '
                                 f'{got[i].tolist() if i < got.shape[0] else None}, oracle '
                                 f'{want[i].tolist() if i < want.shape[0] else None} as (img, anchor, g, slot); '
                                 f'{got.shape[0]} valid slots against {want.shape[0]} positives')
        assert bool((out.slot_anchor[l][out.slot_anchor[l] < 0] == -1).all())
        assert int(out.npos[l]) == asg.slot.numel(), (name, l, int(out.npos[l]), asg.slot.numel())
    want_w = R.expected_winner(case)
    if not torch.equal(out.winner.long(), want_w):
        bad = int((out.winner.long() != want_w).reshape(-1).nonzero()[0])
        raise AssertionError(f'{name}: winner differs first at (img, anchor box) = {divmod(bad, out.TA)}: kernel '
                             f'{int(out.winner.reshape(-1)[bad])}, largest slot {int(want_w.reshape(-1)[bad])}')


def check_forward(name, out, r64, e32, case, tag):
    e = R.loss_errors(out.losses, r64.losses)
    msgs = []
    for l in range(case.L):
        for j, key in enumerate(('cls', 'conf', 'bbox')):
            print(R.describe(f'{tag} {name} loss_{key}[{l}]', float(e[l, j]), float(e32.losses[l, j])))
            if not float(e[l, j]) <= R.bound(float(e32.losses[l, j])):
                msgs.append(f'loss_{key}[{l}]: kernel {float(out.losses[l, j])!r} ref64 {float(r64.losses[l, j])!r} e {float(e[l, j]):.3e} > '
                            f'{R.bound(float(e32.losses[l, j])):.3e}')
        asg = case.assign[l]
        ect = R.err(out.conf_t[l][asg.slot], r64.conf_t[l])
        print(R.describe(f'{tag} {name} conf_t[{l}]', ect, e32.conf_t[l]))
        if not ect <= R.bound(e32.conf_t[l]):
            i = int((out.conf_t[l][asg.slot].double() - r64.conf_t[l]).abs().argmax())
            s = int(asg.slot[i])
            msgs.append(f'conf_t level {l}: e {ect:.3e} > {R.bound(e32.conf_t[l]):.3e}, worst slot (level, k, a, g) = '
                        f'{(l, int(asg.k[i]), int(asg.a[i]), int(asg.g[i]))} (slot {s})')
    assert not msgs, f'{tag} {name}: ' + '; '.join(msgs)


def check_backward(name, out, r64, e32, case, tag):
    msgs = []
    for l in range(case.L):
        fh, fw = case.sizes[l]
        draw = out.draw[l].float()
        assert not bool(torch.isnan(draw).any()), f'{tag} {name} level {l}: draw has elements the backward never wrote'
        pad = draw[..., case.co:]
        if pad.numel() and float(pad.abs().max()) != 0:
            bad = int((draw != 0).logical_and(torch.arange(case.Cp) >= case.co).reshape(-1).nonzero()[0])
            msgs.append(f'padding channel not zero at {where(case, l, bad, draw.shape)}')
        d = draw[..., :case.co]
        # anchor boxes without a positive carry their objectness gradient only
        none = (R.positives_per_box(case, l) == 0).view(case.N, fh, fw, case.A, 1)
        rest = d.reshape(case.N, fh, fw, case.A, case.attr).clone()
        rest[..., 4] = 0
        stray = (rest != 0) & none
        if bool(stray.any()):
            msgs.append(f'anchor box without a positive has a non-objectness gradient at '
                        f'{where(case, l, int(stray.reshape(-1).nonzero()[0]), d.shape)}')
        ed = R.err(d, r64.draw[l])
        print(R.describe(f'{tag} {name} draw[{l}]', ed, e32.draw[l]))
        if not ed <= R.bound(e32.draw[l]):
            lim = R.bound(e32.draw[l]) * float(r64.draw[l].abs().max())
            bad = int(((d.double() - r64.draw[l]).abs() > lim).reshape(-1).nonzero()[0])
            msgs.append(f'draw level {l}: e {ed:.3e} > {R.bound(e32.draw[l]):.3e}; first bad element (level, n, y, x, anchor, '
                        f'attribute) = {where(case, l, bad, d.shape)}: kernel {float(d.reshape(-1)[bad])!r} ref64 '
                        f'{float(r64.draw[l].reshape(-1)[bad])!r}')
        eb = R.err(out.dbias[l], r64.dbias[l])
        print(R.describe(f'{tag} {name} dbias[{l}]', eb, e32.dbias[l]))
        if not eb <= R.bound(e32.dbias[l]):
            c = int((out.dbias[l] - r64.dbias[l]).abs().argmax())
            msgs.append(f'dbias level {l}: e {eb:.3e} > {R.bound(e32.dbias[l]):.3e}; worst channel (anchor, attribute) = '
                        f'{divmod(c, case.attr)}: kernel {float(out.dbias[l][c])!r} ref64 {float(r64.dbias[l][c])!r}')
    assert not msgs, f'{tag} {name}: ' + '; '.join(msgs)


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('name', ALL)
def test_forward_against_float64(name, det, gpu_device):
    """b. (and e.) losses and objectness targets, fp32 maps."""
    case, _, r64, e32 = R.references(name)
    check_forward(name, run_case(name, gpu_device, det=det), r64, e32, case, 'det' if det else 'default')


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('name', ALL)
def test_backward_against_float64(name, det, gpu_device):
    """c. (and e.) the whole conv-output gradient and the bias gradient, fp32 maps."""
    case, _, r64, e32 = R.references(name)
    check_backward(name, run_case(name, gpu_device, det=det), r64, e32, case, 'det' if det else 'default')


@pytest.mark.parametrize('dtype,old_tol,half_ulp', SIXTEEN, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('name', ['coco', 'nonsquare_tall', 'edges', 'agnostic'])
def test_16bit_maps_are_fp32_kernels_plus_one_rounding(name, dtype, old_tol, half_ulp, gpu_device):
    """d. The kernels are one template over the map type and compute in fp32: on ``raw.float()`` the fp32 instantiation
    sees the same numbers.  Deterministic mode: everything bit for bit.  Default mode: ``draw`` bit for bit on every
    anchor box with at most one positive; where float atomics meet in arrival order (rows with several positives) both
    runs are within the bound of float64, hence within twice the bound plus the 16-bit rounding of each other; losses
    and dbias (double atomics in arrival order) are under the bound."""
    case, _, r64, e32 = R.references(name, dtype)
    for det in (True, False):
        o16 = run_case(name, gpu_device, dtype=dtype, det=det)
        o32 = run_case(name, gpu_device, dtype=dtype, det=det, maps_dtype=torch.float32)
        tag = f'{"det" if det else "default"} {str(dtype)[6:]}'
        assert torch.equal(o16.slot_anchor, o32.slot_anchor) and torch.equal(o16.winner, o32.winner)
        assert torch.equal(o16.conf_t, o32.conf_t), f'{tag} {name}: conf_t differs between the instantiations'
        check_forward(name, o32, r64, e32, case, tag + ' as fp32')
        check_backward(name, o32, r64, e32, case, tag + ' as fp32')
        check_forward(name, o16, r64, e32, case, tag)
        for l in range(case.L):
            assert o16.draw[l].dtype == dtype
            want = o32.draw[l].to(dtype)
            same = o16.draw[l].view(torch.int16) == want.view(torch.int16)
            if det:
                assert torch.equal(o16.losses, o32.losses), f'{tag} {name}: losses differ'
                assert torch.equal(o16.dbias[l], o32.dbias[l]), f'{tag} {name} level {l}: dbias differs'
                assert bool(same.all()), (f'{tag} {name}: draw16 != draw32.to(dtype) first at '
                                          f'{where(case, l, int((~same).reshape(-1).nonzero()[0]), same.shape)}')
            else:
                fh, fw = case.sizes[l]
                single = (R.positives_per_box(case, l) <= 1).view(case.N, fh, fw, case.A, 1)
                ok = same[..., :case.co].reshape(case.N, fh, fw, case.A, case.attr) | ~single
                assert bool(ok.all()) and bool(same[..., case.co:].all()), \
                    (f'{tag} {name}: an anchor box with at most one positive differs from the fp32 kernel rounded once, first at '
                     f'{where(case, l, int((~ok).reshape(-1).nonzero()[0]), ok.shape[:3] + (case.co,))}')
                m = float(r64.draw[l].abs().max())
                gap = (o16.draw[l].double() - o32.draw[l].double()).abs()
                lim = 2 * R.bound(e32.draw[l]) * m + half_ulp * o32.draw[l].double().abs() + 2.0 ** -149
                assert bool((gap <= lim).all()), f'{tag} {name} level {l}: a shared row is further from the fp32 kernel than two bounds'
                eb = R.err(o16.dbias[l], r64.dbias[l])
                print(R.describe(f'{tag} {name} dbias[{l}]', eb, e32.dbias[l]))
                assert eb <= R.bound(e32.dbias[l]), (tag, name, l, eb)
            # the statement of test_gpu_fused_loss.py stays
            assert R.err(o16.draw[l][..., :case.co], r64.draw[l]) <= old_tol
            assert float(o16.draw[l][..., case.co:].float().abs().max()) == 0


@pytest.mark.parametrize('name', ['coco', 'edges'])
def test_deterministic_mode_repeats_bit_for_bit(name, gpu_device):
    """e. three runs under set_deterministic(True): identical bits in losses, draw, dbias."""
    runs = [run_case(name, gpu_device, det=True, fresh=True) for _ in range(3)]
    for o in runs[1:]:
        assert torch.equal(o.losses, runs[0].losses)
        for l in range(len(o.draw)):
            assert torch.equal(o.draw[l], runs[0].draw[l]) and torch.equal(o.dbias[l], runs[0].dbias[l])
        assert torch.equal(o.conf_t, runs[0].conf_t) and torch.equal(o.winner, runs[0].winner)


@pytest.mark.parametrize('name', ['nonsquare_tall', 'nonsquare_wide', 'agnostic'])
def test_through_the_module(name, gpu_device):
    """f. ``head.loss`` + ``backward`` on RawPredMaps (``_loss_fused``, the image index table, ``FusedLosses``) gives the
    tensors of the ABI call, bit for bit in deterministic mode.  The upstream gradient of the ABI call is taken through
    the same aggregation (weights x level balance) on a leaf, so that it is the very fp32 matrix the module passes."""
    dev = gpu_device
    case, inputs, _, _ = R.references(name)
    head = head_for(case, dev)
    bal = torch.tensor([[1.0, float(head.conf_level_balance_weight[l]), 1.0] for l in range(case.L)], device=dev)
    keys = ('loss_conf', 'loss_bbox') if case.agnostic else ('loss_cls', 'loss_conf', 'loss_bbox')

    def total(fl):
        return sum(w * v for key in keys for w, v in zip(R.WEIGHTS[key], [x.sum() for x in fl[key]]))

    with det_mode(True):
        leaves, maps = [], []
        for raw, bias in inputs:
            r = raw.to(dev).permute(0, 3, 1, 2).requires_grad_(True)        # NCHW view of NHWC storage: channels_last
            b = bias.to(dev).requires_grad_(True)
            leaves.append((r, b))
            maps.append(RawPredMap(r, b, case.A, case.attr))
        fl = head.loss(maps, [b.to(dev) for b in case.boxes], [l.to(dev) for l in case.labels], None)
        assert ('loss_cls' in fl) == (not case.agnostic)
        got = torch.stack([torch.stack([(fl[k][l] if k in fl else torch.zeros((), device=dev)).reshape(())
                                        for k in ('loss_cls', 'loss_conf', 'loss_bbox')]) for l in range(case.L)])
        total(fl).backward()
        leaf = torch.zeros(case.L, 3, device=dev, requires_grad=True)
        from mmdet_yolov4_amd.yolocsp_head import FusedLosses
        total(FusedLosses(leaf * bal, None, with_cls=not case.agnostic)).backward()
        raws = [raw.to(dev).contiguous() for raw, _ in inputs]
        biases = [b.to(dev).float().contiguous() for _, b in inputs]
        out = run_abi(head, case, raws, biases, leaf.grad, dev)
    assert torch.equal(got.detach().cpu(), (out.losses.to(dev) * bal).cpu())
    assert abs(float(fl['num_gts']) - case.G / case.N) < 1e-4
    for l, (r, b) in enumerate(leaves):
        assert torch.equal(r.grad.permute(0, 2, 3, 1).cpu(), out.draw[l]), f'{name} level {l}: draw'
        assert torch.equal(b.grad.cpu(), out.dbias[l].float()), f'{name} level {l}: dbias'
