"""The fused YOLOv3 loss (csrc/loss_v3.hip: yv4_yolov3_loss_fwd / _bwd) per element against a float64 reference, at the
shapes and edges where its kernels take their other paths (tests/_v3_loss_ref.py: cases, coverage conditions, reference).

The C ABI is driven with a ``V3LossDesc`` built the way ``YoloV3LossFunction.forward`` builds it, so that the work buffers
can be read back.  Integer buffers are pre-filled with a sentinel and ``dpred`` with NaN: an unwritten element shows.

  a. ``assigned``, ``img_off``, ``gt_cell``, ``gt_max`` (bit patterns) and -- ``gt_max_assign_all=False`` -- ``gt_arg``
     equal the reference's, whole arrays, no tolerance;
  b. the (L, 4) losses and every gradient element against float64, default and deterministic mode; the deterministic
     mode repeats bit for bit;
  c. the exact row count: with every objectness and class logit at 64.0 the raw ``loss_conf`` sum word of a level is
     ``64 x #negatives`` and the ``loss_cls`` word ``64 x (C - 1) x #positives``, exactly, in both modes;
  d. ``head.loss`` + ``backward`` returns the ABI call's tensors bit for bit.

Bound: with ``e(x) = max |x - ref64| / max |ref64|`` and ``e32`` the same measure of the
REFERENCE's own float32 evaluation on the CPU, ``e(kernel) <= 4 * e32 + 8 * 2**-24``; per loss value, and for the
gradients per level and attribute group (xy, wh, conf, cls).  It comes from the reference, not from what the kernels
achieve.
"""
import contextlib
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib, ops

import _v3_loss_ref as R

pytestmark = pytest.mark.gpu

RUNS = list(R.CASES) + ['layouts@nhwc', 'layouts@view']        # 'layouts' itself is the contiguous NCHW run
SENTINEL = -7
PAD_N, PAD_C = 1, 8                                             # the strided view starts at image 1, channel 8


@contextlib.contextmanager
def det_mode(on):
    was = pkg.deterministic()
    pkg.set_deterministic(on)
    try:
        yield
    finally:
        pkg.set_deterministic(was)


_heads = {}


def head_for(case, count=False):
    """The head a configuration file would build for the case.  ``count``: part c's terms (no smoothing, 'sum')."""
    key = (case.name, count)
    if key not in _heads:
        def term(u, typ, **kw):
            return dict(type=typ, loss_weight=1.0 if count else case.weights[u], reduction='sum' if count else case.reduction[u],
                        **kw)
        _heads[key] = pkg.YOLOV3Head(
            num_classes=case.C, in_channels=[8] * case.L, out_channels=[8] * case.L, featmap_strides=case.strides,
            anchor_generator=dict(type='YOLOAnchorGenerator', base_sizes=case.base_sizes, strides=case.strides),
            one_hot_smoother=0.0 if count else case.smoother,
            loss_cls=term(0, 'CrossEntropyLoss', use_sigmoid=True), loss_conf=term(1, 'CrossEntropyLoss', use_sigmoid=True),
            loss_xy=term(2, 'CrossEntropyLoss', use_sigmoid=True), loss_wh=term(3, 'MSELoss'),
            train_cfg=dict(assigner=dict(type='GridAssigner', **case.assigner)))
    return _heads[key]


def device_maps(case, maps, dev, layout=None):
    """The logical NCHW maps in the layouts the case (or ``layout``) names.  Returns (maps, buffers): for 'view' the map
    is the channel range [8 : 8 + A*(5+C)) and the image range [1 : 1 + N) of a wider, longer buffer of NaN."""
    out, bufs = [], []
    for l, m in enumerate(maps):
        how = layout or case.layouts[l]
        m = m.to(dev)
        if how == 'nchw':
            out.append(m.contiguous())
            bufs.append(None)
        elif how == 'nhwc':
            out.append(m.contiguous(memory_format=torch.channels_last))
            bufs.append(None)
        else:
            N, Cc, H, W = m.shape
            buf = torch.full((N + 2, Cc + PAD_C + 5, H, W), float('nan'), device=dev)
            buf[PAD_N:PAD_N + N, PAD_C:PAD_C + Cc] = m
            out.append(buf[PAD_N:PAD_N + N, PAD_C:PAD_C + Cc])
            bufs.append(buf)
    return out, bufs


def run_abi(head, case, maps, gout, dev, bufs=None):
    """One forward + backward through the C ABI on device maps of any strides."""
    L, A, N, G = case.L, case.A, case.N, case.G
    assert head.num_anchors == A and head.num_classes == case.C
    asg = head.assigner
    d = _lib.V3LossDesc()
    d.num_levels, d.N, d.A, d.num_classes, d.G = L, N, A, case.C, G
    d.gt_max_assign_all = 1 if asg.gt_max_assign_all else 0
    TA = 0
    for l, p in enumerate(maps):
        n_, cc, H, W = p.shape
        assert (n_, cc, H, W) == (N, A * (5 + case.C)) + tuple(case.sizes[l]) and p.dtype == torch.float32
        lv = d.levels[l]
        lv.pred = p.data_ptr()
        lv.sn, lv.sc, lv.sh, lv.sw = p.stride()
        lv.H, lv.W, lv.stride = H, W, int(head.featmap_strides[l])
        ba = head.anchor_generator.base_anchors[l].float().cpu()
        for k in range(A):
            for c in range(4):
                lv.base_anchors[k][c] = float(ba[k, c])
        TA += H * W * A
    i32 = dict(dtype=torch.int32, device=dev)
    img_off = torch.full((N + 1,), SENTINEL, **i32)
    gt_cell = torch.full((max(L * G, 1),), SENTINEL, **i32)
    gt_max = torch.full((max(G, 1),), SENTINEL, **i32)
    gt_arg = torch.full((max(G, 1),), SENTINEL, **i32)
    assigned = torch.full((N, TA), SENTINEL, **i32)
    sums = torch.full((2, L, 4), float('nan'), dtype=torch.float64, device=dev)
    losses = torch.full((L, 4), float('nan'), dtype=torch.float32, device=dev)
    gt = torch.cat(case.boxes).reshape(-1, 4).to(dev).float().contiguous()
    gt_label = torch.cat(case.labels).reshape(-1).to(dev).long().contiguous()
    gt_img = torch.repeat_interleave(torch.arange(N), torch.tensor([int(b.shape[0]) for b in case.boxes])).to(dev).long()
    d.gt, d.gt_label, d.gt_img = gt.data_ptr(), gt_label.data_ptr(), gt_img.data_ptr()
    d.pos_iou_thr, d.min_pos_iou = float(asg.pos_iou_thr), float(asg.min_pos_iou)
    if isinstance(asg.neg_iou_thr, float):
        d.neg_lo, d.neg_hi = -1.0, float(asg.neg_iou_thr)
    else:
        d.neg_lo, d.neg_hi = float(asg.neg_iou_thr[0]), float(asg.neg_iou_thr[1])
    eps = head.bbox_coder.eps
    d.eps, d.eps_hi = float(eps), float(torch.tensor(1 - eps, dtype=torch.float32))
    d.iou_eps = 1e-6
    d.smoother = float(head.one_hot_smoother)
    for k, t in enumerate((head.loss_cls, head.loss_conf, head.loss_xy, head.loss_wh)):
        d.loss_weight[k] = float(t.loss_weight)
        d.reduce_mean[k] = 1 if t.reduction == 'mean' else 0
    d.img_off, d.gt_cell, d.gt_max, d.gt_arg = (t.data_ptr() for t in (img_off, gt_cell, gt_max, gt_arg))
    d.assigned, d.sums, d.losses = assigned.data_ptr(), sums.data_ptr(), losses.data_ptr()
    _lib.check(_lib.lib().yv4_yolov3_loss_fwd(C.byref(d), ops.stream_ptr()), 'yv4_yolov3_loss_fwd')
    gout = gout.to(dev).float().contiguous()
    grads, dbufs = [], []
    for l, p in enumerate(maps):
        if bufs is not None and bufs[l] is not None:                      # the gradient of a view lives in a buffer like its map's
            dbuf = torch.full_like(bufs[l], float('nan'))
            gr = dbuf[PAD_N:PAD_N + N, PAD_C:PAD_C + p.shape[1]]
            assert gr.stride() == p.stride()
        else:
            dbuf = None
            gr = torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=dev).fill_(float('nan'))
        d.levels[l].dpred = gr.data_ptr()
        grads.append(gr)
        dbufs.append(dbuf)
    _lib.check(_lib.lib().yv4_yolov3_loss_bwd(C.byref(d), gout.data_ptr(), ops.stream_ptr()), 'yv4_yolov3_loss_bwd')
    torch.cuda.synchronize()
    return SimpleNamespace(losses=losses.cpu(), sums=sums.view(torch.int64).cpu(), assigned=assigned.cpu(), img_off=img_off.cpu(),
                           gt_cell=gt_cell[:L * G].view(L, G).cpu(), gt_max=gt_max[:G].cpu(), gt_arg=gt_arg[:G].cpu(),
                           grads=[g.cpu() for g in grads], grad_strides=[g.stride() for g in grads],
                           dbufs=[None if b is None else b.cpu() for b in dbufs], keep=(maps, gt, gt_label, gt_img))


def split(run):
    name, _, layout = run.partition('@')
    return name, (layout or None)


_runs = {}


def run_case(run, dev, det=False, fresh=False):
    key = (run, det)
    if fresh or key not in _runs:
        name, layout = split(run)
        case, asg, maps, _, _ = R.references(name)
        dmaps, bufs = device_maps(case, maps, dev, layout)
        with det_mode(det):
            out = run_abi(head_for(case), case, dmaps, R.gout_matrix(case.L), dev, bufs)
        if fresh:
            return out
        _runs[key] = out
    return _runs[key]


def first_diff(got, want):
    bad = (got != want).reshape(-1).nonzero().reshape(-1)
    i = int(bad[0])
    return f'{bad.numel()} differ, first at flat index {i}: kernel {int(got.reshape(-1)[i])}, reference {int(want.reshape(-1)[i])}'


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS)
def test_integer_outputs_exact(run, gpu_device):
    """a. whole arrays, ``torch.equal``."""
    name, _ = split(run)
    case, asg = R.get_case(name)
    out = run_case(run, gpu_device)
    assert torch.equal(out.img_off.long(), asg.img_off), f'{run}: img_off: ' + first_diff(out.img_off.long(), asg.img_off)
    assert torch.equal(out.gt_cell.long(), asg.gt_cell), f'{run}: gt_cell: ' + first_diff(out.gt_cell.long(), asg.gt_cell)
    assert torch.equal(out.gt_max, asg.gt_max), f'{run}: gt_max bit patterns: ' + first_diff(out.gt_max, asg.gt_max)
    if not case.assigner['gt_max_assign_all']:
        assert torch.equal(out.gt_arg.long(), asg.gt_arg), f'{run}: gt_arg: ' + first_diff(out.gt_arg.long(), asg.gt_arg)
    if not torch.equal(out.assigned.long(), asg.assigned):
        bad = int((out.assigned.long() != asg.assigned).reshape(-1).nonzero()[0])
        n, k = divmod(bad, asg.TA)
        raise AssertionError(f'{run}: assigned: ' + first_diff(out.assigned.long(), asg.assigned) + f' = (image {n}, anchor box {k})')


def check_against_float64(run, out, tag):
    name, layout = split(run)
    case, asg, maps, r64, e32 = R.references(name)
    msgs = []
    e = R.loss_errors(out.losses, r64.losses)
    for l in range(case.L):
        for u, key in enumerate(R.TERMS):
            ev, e3 = float(e[l, u]), float(e32.losses[l, u])
            print(f'V3EXACT|{run}|{tag}|{key}[{l}]|{ev:.3e}|{e3:.3e}|{R.bound(e3):.3e}')
            if not ev <= R.bound(e3):
                msgs.append(f'{key}[{l}]: kernel {float(out.losses[l, u])!r} ref64 {float(r64.losses[l, u])!r} e {ev:.3e} > '
                            f'{R.bound(e3):.3e}')
    for l in range(case.L):
        g = out.grads[l]
        if bool(torch.isnan(g).any()):
            msgs.append(f'level {l}: the backward left {int(torch.isnan(g).sum())} gradient elements unwritten')
            continue
        for gname, lo, hi in R.GROUPS:
            got, want = R.group_view(case, g, lo, hi), R.group_view(case, r64.grads[l], lo, hi)
            ev, e3 = R.err(got, want), e32.grads[(l, gname)]
            print(f'V3EXACT|{run}|{tag}|grad_{gname}[{l}]|{ev:.3e}|{e3:.3e}|{R.bound(e3):.3e}')
            if not ev <= R.bound(e3):
                i = int((got.double() - want).abs().reshape(-1).argmax())
                pos = [int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)]
                msgs.append(f'grad {gname} level {l}: e {ev:.3e} > {R.bound(e3):.3e}; worst (n, a, attribute - {lo}, y, x) = {pos}: '
                            f'kernel {float(got.reshape(-1)[i])!r} ref64 {float(want.reshape(-1)[i])!r}')
        if out.dbufs[l] is not None:                # the strided view: nothing outside it was touched
            inside = torch.zeros_like(out.dbufs[l], dtype=torch.bool)
            inside[PAD_N:PAD_N + case.N, PAD_C:PAD_C + g.shape[1]] = True
            if not bool(torch.isnan(out.dbufs[l][~inside]).all()):
                msgs.append(f'level {l}: the backward wrote outside the view')
    assert not msgs, f'{tag} {run}: ' + '; '.join(msgs)


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('run', RUNS)
def test_losses_and_gradients_against_float64(run, det, gpu_device):
    """b. every loss value and every gradient element, both modes."""
    check_against_float64(run, run_case(run, gpu_device, det=det), 'det' if det else 'default')


@pytest.mark.parametrize('run', ['la_5x2', 'many_gts', 'row_counts', 'layouts@view'])
def test_deterministic_mode_repeats_bit_for_bit(run, gpu_device):
    """b. two runs under set_deterministic(True): identical sum words, losses and gradients."""
    a = run_case(run, gpu_device, det=True)
    b = run_case(run, gpu_device, det=True, fresh=True)
    assert bool(a.sums[1].any()), 'the fixed-point lo words were not written: not the deterministic path'
    assert torch.equal(a.sums, b.sums) and torch.equal(a.losses, b.losses) and torch.equal(a.assigned, b.assigned)
    for x, y in zip(a.grads, b.grads):
        assert torch.equal(x, y)


def test_no_gt_is_all_negative(gpu_device):
    """G = 0: every id is 0, the cls / xy / wh losses are exactly 0 and only the objectness gradient is non-zero."""
    case, asg = R.get_case('no_gt')
    for det in (False, True):
        out = run_case('no_gt', gpu_device, det=det)
        assert int((out.assigned != 0).sum()) == 0
        assert float(out.losses[:, [0, 2, 3]].abs().max()) == 0 and float(out.losses[:, 1].min()) > 0
        for l in range(case.L):
            for gname, lo, hi in R.GROUPS:
                m = float(R.group_view(case, out.grads[l], lo, hi).abs().max())
                assert (m > 0) == (gname == 'conf'), (det, l, gname, m)


@pytest.mark.parametrize('name', R.COUNT_CASES)
def test_exact_row_count(name, gpu_device):
    """c. bce(64, 0) is exactly 64 in fp32 and bce(64, 1) = 1.6e-28 vanishes beside it in a double: the raw sum words
    count the rows.  One dropped, duplicated or mis-assigned row changes the word by 64."""
    dev = gpu_device
    case, asg = R.get_case(name)
    want = R.count_expectation(case, asg)
    dmaps, _ = device_maps(case, R.exact_count_maps(case), dev)
    head = head_for(case, count=True)
    assert head.one_hot_smoother == 0 and head.loss_conf.reduction == 'sum' and head.loss_cls.reduction == 'sum'
    for det in (False, True):
        with det_mode(det):
            out = run_abi(head, case, dmaps, torch.ones(case.L, 4), dev)
        assert torch.equal(out.assigned.long(), asg.assigned), f'{name}: assigned: ' + first_diff(out.assigned.long(), asg.assigned)
        for l, (neg, pos) in enumerate(want):
            for u, count, what in ((1, 64 * neg, 'loss_conf'), (0, 64 * (case.C - 1) * pos, 'loss_cls')):
                if det:
                    hi, lo = int(out.sums[0, l, u]), int(out.sums[1, l, u])
                    assert lo >= 0, f'{name} level {l} {what}: the overflow flag is set'
                    got = (hi + (lo >> 32)) * 2 ** 32 + (lo & (2 ** 32 - 1))        # in units of 2**-40
                    assert got == count * 2 ** 40, (f'det {name} level {l} {what}: sum word {got / 2 ** 40!r}, rows say {count} '
                                                    f'({neg} negatives, {pos} positives)')
                else:
                    got = float(out.sums[0, l, u].view(torch.float64))
                    assert not bool(out.sums[1].any())
                    assert got == float(count), (f'default {name} level {l} {what}: sum word {got!r}, rows say {count} '
                                                 f'({neg} negatives, {pos} positives)')


@pytest.mark.parametrize('run', RUNS)
def test_abi_path_equals_the_autograd_path(run, gpu_device):
    """d. ``head.loss`` + ``backward`` on the same tensors: the ABI call's losses bit for bit in deterministic mode, its
    gradients bit for bit in both (they have no sums), with the maps' strides; a strided view's buffer gets exact zeros
    outside the view."""
    dev = gpu_device
    name, layout = split(run)
    case, asg, maps, _, _ = R.references(name)
    head = head_for(case)
    gout = R.gout_matrix(case.L).to(dev)
    for det in (True, False):
        out = run_case(run, dev, det=det)
        dmaps, bufs = device_maps(case, maps, dev, layout)
        leaves = [b.requires_grad_(True) if b is not None else m.requires_grad_(True) for m, b in zip(dmaps, bufs)]
        views = [leaf[PAD_N:PAD_N + case.N, PAD_C:PAD_C + m.shape[1]] if b is not None else leaf
                 for leaf, m, b in zip(leaves, dmaps, bufs)]
        with det_mode(det):
            assert head._fused_loss_ok(views), run
            fl = head.loss(views, [b.to(dev) for b in case.boxes], [x.to(dev) for x in case.labels], [dict() for _ in range(case.N)])
            assert list(fl) == list(R.TERMS)
            mat = torch.stack([torch.stack([v.reshape(()) for v in fl[k]]) for k in R.TERMS], 1)
            got = torch.autograd.grad((mat * gout).sum(), views, retain_graph=True)
            (mat * gout).sum().backward()
        if det:
            assert torch.equal(mat.detach().cpu(), out.losses), f'{run}: losses differ from the ABI call'
        for l in range(case.L):
            assert got[l].stride() == views[l].stride() == out.grad_strides[l], (run, l, got[l].stride(), views[l].stride())
            assert torch.equal(got[l].cpu(), out.grads[l]), f'{run} level {l} (det={det}): gradient differs from the ABI call'
            if bufs[l] is not None:
                full = leaves[l].grad.cpu()
                inside = torch.zeros_like(full, dtype=torch.bool)
                inside[PAD_N:PAD_N + case.N, PAD_C:PAD_C + views[l].shape[1]] = True
                assert bool((full[~inside] == 0).all()), f'{run} level {l}: the buffer gradient is not zero outside the view'
                assert torch.equal(full[inside].reshape(out.grads[l].shape), out.grads[l])
            else:
                assert torch.equal(leaves[l].grad.cpu(), out.grads[l])
