"""Cases, float64 reference and configurations for the fused YOLOCSPHead loss with the IoU / DIoU / CIoU box terms and
SoftFocalLoss (a helper module, not a conftest; used by test_loss_variants_host.py and test_gpu_loss_variants.py).

Like ``_loss_ref`` (whose case builders, assignment, error measure and bound are reused), the loss has a discrete half --
``oracle.responsible_indices`` on the fp32 boxes -- and a continuous half, which is stated HERE: the gather, sigmoid and
decode of ``oracle.head_loss``, then the package's torch restatements of the box losses (``losses.iou_loss`` /
``diou_loss`` / ``ciou_loss``, pinned bit for bit by tests/golden/loss_variants.npz against the reference's classes) and
the SoftFocalLoss expression (yolocsp_head.py:21-50; pinned against ``losses.SoftFocalLoss`` in the host test), in
``dtype``.  float32 is the reference, float64 what the kernels are compared with; ``e32`` is the former's error against
the latter and the GPU bound is ``4 * e32 + 8 * 2**-24``.

Everything here runs on the CPU.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from mmdet_yolov4_amd import losses as Ls
from oracle import yolov4_oracle as O

import _loss_ref as R

W_CLS, W_CONF, W_BBOX = 32., 64., 3.2          # the head's default loss weights
EPS = 1e-6
KINDS = ('giou', 'iou_linear', 'iou_log', 'diou', 'ciou')          # position = yv4_loss_opts.box_kind
BOX_CFG = dict(giou=dict(type='GIoULoss'), iou_linear=dict(type='IoULoss', linear=True),
               iou_log=dict(type='IoULoss', linear=False), diou=dict(type='DIoULoss'), ciou=dict(type='CIoULoss'))
ALPHA = 0.25


def cfg(kind, conf=None, cls=None):
    """A configuration: box kind, and (gamma, alpha) of SoftFocalLoss on the objectness / class term or None."""
    tag = kind + (f'-conf{conf[0]}' if conf else '') + (f'-cls{cls[0]}' if cls else '')
    return SimpleNamespace(kind=kind, conf=conf, cls=cls, tag=tag)


PLAIN = [cfg(k) for k in KINDS[1:]]                                 # per box kind (GIoU without focal is the existing file)
FOCAL = [cfg(k, conf=(g, ALPHA) if 'conf' in on else None, cls=(g, ALPHA) if 'cls' in on else None)
         for k in ('giou', 'ciou') for g in (1.5, 2.0) for on in (('conf',), ('cls',), ('conf', 'cls'))]
CONFIGS = {c.tag: c for c in PLAIN + FOCAL}


def box_loss(kind, pred, target):
    if kind == 'giou':
        return 1 - Ls.bbox_overlaps_giou_aligned(pred, target, eps=EPS)
    if kind in ('iou_linear', 'iou_log'):
        return Ls.iou_loss(pred, target, linear=kind == 'iou_linear', eps=EPS)
    return (Ls.diou_loss if kind == 'diou' else Ls.ciou_loss)(pred, target, eps=EPS)


def bce_or_focal(x, t, focal):
    """Element losses: sigmoid BCE, or SoftFocalLoss around it in the reference's expression order."""
    loss = F.binary_cross_entropy_with_logits(x, t, reduction='none')
    if focal is None:
        return loss
    gamma, alpha = focal
    p = torch.sigmoid(x)
    p_t = t * p + (1 - t) * (1 - p)
    return loss * (t * alpha + (1 - t) * (1 - alpha)) * (1.0 - p_t) ** gamma


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def case_coco():
    """80 classes, three levels, batch 8, random boxes as ``_loss_ref._random_boxes`` draws them."""
    N, S_ = 8, 608
    base, strides = O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES
    g = torch.Generator().manual_seed(140)
    per_img = []
    for n in range(N):
        k = R._poisson(g, 30)
        b = R._random_boxes(g, k, S_, S_)
        lab = torch.randint(0, 80, (k,), generator=g)
        per_img.append([(b[i].tolist(), int(lab[i])) for i in range(k)])
    plant = R._box(215.0, 301.0, 72., 90.)            # matches an anchor of each level; three copies share anchor boxes
    per_img[2] = [(plant, 10 + 30 * i) for i in range(3)] + per_img[2]
    return R._assemble('v_coco', N, S_, S_, strides, base, 80, per_img, None, None, seed=141, cp=256)


def case_nonsquare_agnostic():
    N, H, W = 3, 320, 416
    base, strides = O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES
    g = torch.Generator().manual_seed(150)
    per_img = []
    for n in range(N):
        b = R._random_boxes(g, 10, H, W)
        per_img.append([(b[i].tolist(), 0) for i in range(10)])
    for l, s in enumerate(strides):                    # per level two boxes of one image on one anchor box
        bw, bh = base[l][1]
        for i in range(2):
            per_img[l % N].append((R._box(2.25 * s, 3.25 * s, bw * (1.2 - 0.2 * i), bh * 0.9), 0))
    return R._assemble('v_nonsquare_agnostic', N, H, W, strides, base, 80, per_img, None, None, seed=151, cp=16, agnostic=True)


def case_edges():
    """``_loss_ref``'s hand-built boxes with other random extras; the raw maps are planted by ``make_inputs``."""
    return R.case_edges('v_edges', extra_random=16, seed=160)


def case_dups():
    """For the comparison with the tensor-op path, whose index_put is order-dependent on the GPU where DIFFERENT
    positives share an anchor box: here the only sharing positives are copies of one box (equal objectness targets)."""
    N, H, W, C = 2, 96, 128, 5
    strides = [8, 16, 32]
    g = torch.Generator().manual_seed(175)
    per_img = []
    for n in range(N):
        b = R._random_boxes(g, 5, H, W, lo=8.0, hi=110.0)
        lab = torch.randint(0, C, (5,), generator=g)
        per_img.append([(b[i].tolist(), int(lab[i])) for i in range(5)])
    per_img[0] += [(R._box(42.0, 42.0, 34., 62.), i) for i in range(3)]          # matches (30, 60) and neighbours of it
    per_img[1] += [(R._box(50.0, 40.0, 14., 13.), i + 1) for i in range(2)]      # (10, 12), (16, 30)
    per_img[1] += [(R._box(60.0, 50.0, 120., 100.), i + 2) for i in range(2)]    # (100, 90)
    return R._assemble('v_dups', N, H, W, strides, R.SMALL_BASE, C, per_img, None, None, seed=172)


CASES = dict(v_coco=case_coco, v_nonsquare_agnostic=case_nonsquare_agnostic, v_edges=case_edges)
_case_cache = {}


def get_case(name):
    if name not in _case_cache:
        case = (CASES.get(name) or dict(v_dups=case_dups)[name])()
        case.assign = R.assignment(case)
        _case_cache[name] = case
    return _case_cache[name]


def planted(case, l):
    """Indices (into level l's positive list) of the positives whose box logits ``make_inputs`` plants: every third."""
    return torch.arange(0, case.assign[l].slot.numel(), 3)


def make_inputs(case, dtype=torch.float32):
    """``_loss_ref.make_inputs``; the ``v_edges`` case then gets, for every third positive, box logits that put a tiny
    box (width / height logits -4: 0.13 % of the anchor's) a whole stride away from the anchor centre, on the side
    away from the ground truth's centre (offset logits +-6): positives with zero overlap."""
    inputs = R.make_inputs(case, dtype)
    if case.name != 'v_edges':
        return inputs
    gtb = torch.cat(case.boxes)
    anchors = O.grid_anchors(case.sizes, case.base_sizes, case.strides)
    for l, (raw, bias) in enumerate(inputs):
        asg = case.assign[l]
        fh, fw = case.sizes[l]
        for i in planted(case, l).tolist():
            n, anc, g = int(asg.img[i]), int(asg.anchor[i]), int(asg.g[i])
            cell, a = divmod(anc, case.A)
            y, x = divmod(cell, fw)
            ab = anchors[l][anc]
            acx, acy = float(ab[0] + ab[2]) / 2, float(ab[1] + ab[3]) / 2
            gcx, gcy = float(gtb[g, 0] + gtb[g, 2]) / 2, float(gtb[g, 1] + gtb[g, 3]) / 2
            want = torch.tensor([-6.0 if gcx >= acx else 6.0, -6.0 if gcy >= acy else 6.0, -4.0, -4.0])
            c0 = a * case.attr
            raw[n, y, x, c0:c0 + 4] = (want - bias[c0:c0 + 4]).to(dtype)
    return inputs


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def positive_terms(case, leaves, l, kind, dtype):
    """(box loss, iou, decoded boxes) of level l's positives in list order, differentiable."""
    asg = case.assign[l]
    anchors = O.grid_anchors(case.sizes, case.base_sizes, case.strides)[l].to(dtype)
    gtb = torch.cat(case.boxes).to(dtype)
    pm = leaves[l].permute(0, 2, 3, 1).reshape(case.N, -1, case.attr)
    pos = pm[asg.img, asg.anchor]
    pb = pos[:, :4].sigmoid()
    box = O.bbox_decode(anchors[asg.anchor], torch.cat((pb[:, :2] * 2. - 1., (pb[:, 2:] * 2.) ** 2.), -1), case.strides[l])
    return box_loss(kind, box, gtb[asg.g]), pos, box, gtb[asg.g]


def reference(case, inputs, c, dtype):
    """The head loss of configuration ``c`` in ``dtype`` on the fp32 inputs, differentiated by autograd under
    ``_loss_ref.WEIGHTS``.  Returns what ``_loss_ref.reference`` returns: losses (L, 3) [cls | conf before the level
    balance | bbox], per level conf_t of every positive in list order, draw (N, H, W, co), dbias (co,)."""
    leaves = [d.to(dtype).requires_grad_(True) for d in R.dense_maps(case, inputs)]
    gtl = torch.cat(case.labels)
    rows, conf_ts = [], []
    for l in range(case.L):
        asg = case.assign[l]
        pm = leaves[l].permute(0, 2, 3, 1).reshape(case.N, -1, case.attr)
        pred_conf = pm[..., 4]
        target_conf = torch.zeros_like(pred_conf)
        loss_bbox, loss_cls = pm.new_zeros(()), pm.new_zeros(())
        conf_t = torch.zeros(0, dtype=dtype)
        if asg.slot.numel():
            bl, pos, _, _ = positive_terms(case, leaves, l, c.kind, dtype)
            loss_bbox = bl.mean() * W_BBOX
            if case.C > 0:
                tcls = F.one_hot(gtl[asg.g], num_classes=case.C).to(dtype)
                if case.smoother != 0:
                    tcls = tcls * (1 - case.smoother) + case.smoother / case.C
                loss_cls = W_CLS * bce_or_focal(pos[:, 5:], tcls, c.cls).mean()
            conf_t = (1 - bl).detach().clamp(0.0, 1.0)
            flat = asg.img * pred_conf.shape[1] + asg.anchor           # the LAST positive in list order wins (oracle.head_loss)
            last = torch.full((pred_conf.numel(),), -1, dtype=torch.long)
            last.scatter_reduce_(0, flat, torch.arange(flat.numel()), reduce='amax', include_self=True)
            target_conf = target_conf.reshape(-1)
            target_conf[flat] = conf_t[last[flat]]
            target_conf = target_conf.view(pred_conf.shape)
        loss_conf = W_CONF * bce_or_focal(pred_conf, target_conf, c.conf).mean()
        rows.append(torch.stack([loss_cls, loss_conf, loss_bbox]))
        conf_ts.append(conf_t)
    losses = torch.stack(rows)
    assert losses.dtype == dtype
    (losses * R.gout_matrix(case.L).to(dtype)).sum().backward()
    draw = [x.grad.permute(0, 2, 3, 1).contiguous() for x in leaves]
    dbias = [x.grad.sum((0, 2, 3)) for x in leaves]
    return SimpleNamespace(losses=losses.detach(), conf_t=conf_ts, draw=draw, dbias=dbias)


_ref_cache = {}


def references(name, tag, dtype=torch.float32):
    """(case, inputs, ref64, e32) for a case, a configuration and a map dtype, computed once per process."""
    key = (name, tag, dtype)
    if key not in _ref_cache:
        case = get_case(name)
        inputs = make_inputs(case, dtype)
        c = CONFIGS[tag]
        r64 = reference(case, inputs, c, torch.float64)
        r32 = reference(case, inputs, c, torch.float32)
        e32 = SimpleNamespace(losses=R.loss_errors(r32.losses, r64.losses),
                              conf_t=[R.err(a, b) for a, b in zip(r32.conf_t, r64.conf_t)],
                              draw=[R.err(a, b) for a, b in zip(r32.draw, r64.draw)],
                              dbias=[R.err(a, b) for a, b in zip(r32.dbias, r64.dbias)])
        _ref_cache[key] = (case, inputs, r64, e32)
    return _ref_cache[key]


def branch_facts(case, inputs, kind):
    """Float64 facts about every positive of a case under a box kind, all levels concatenated: overlap area, the box
    loss, the objectness target and (CIoU) the trade-off term's denominator ``1 - iou + v``."""
    leaves = [d.double() for d in R.dense_maps(case, inputs)]
    ov, loss, den = [], [], []
    for l in range(case.L):
        if not case.assign[l].slot.numel():
            continue
        bl, _, box, tg = positive_terms(case, leaves, l, kind, torch.float64)
        wh = (torch.min(box[:, 2:], tg[:, 2:]) - torch.max(box[:, :2], tg[:, :2])).clamp(min=0)
        ov.append(wh[:, 0] * wh[:, 1])
        loss.append(bl)
        if kind == 'ciou':
            ious, _ = Ls._ious_c2(box, tg, EPS)
            v = 4 / math.pi ** 2 * (torch.atan((tg[:, 2] - tg[:, 0]) / (tg[:, 3] - tg[:, 1] + EPS))
                                    - torch.atan((box[:, 2] - box[:, 0]) / (box[:, 3] - box[:, 1] + EPS))) ** 2
            den.append(1 - ious + v)
    loss = torch.cat(loss)
    return SimpleNamespace(overlap=torch.cat(ov), loss=loss, conf_t=(1 - loss).clamp(0.0, 1.0),
                           den=torch.cat(den) if den else None)


def check_coverage(name):
    """The conditions a GPU case must meet so that it cannot pass by being empty; a failure is a test failure."""
    case = get_case(name)
    for l, asg in enumerate(case.assign):
        assert asg.slot.numel() >= 1, f'{name} level {l}: no positives'
    assert max(int(R.positives_per_box(case, l).max()) for l in range(case.L)) >= 2, f'{name}: no anchor box with two positives'
    inputs = make_inputs(case)
    if name == 'v_edges':
        for kind in KINDS[1:]:
            f = branch_facts(case, inputs, kind)
            assert int((f.overlap == 0).sum()) >= 1, f'{name} {kind}: no positive with zero overlap'
        f = branch_facts(case, inputs, 'iou_log')
        assert int(((f.loss >= 1) & (f.conf_t == 0)).sum()) >= 1, f'{name}: no IoU-log target clamped to 0'
    f = branch_facts(case, inputs, 'ciou')
    assert float(f.den.min()) >= 1e-3, f'{name}: a CIoU positive sits at the 0 / 0 point ({float(f.den.min()):.3e})'
    return case
