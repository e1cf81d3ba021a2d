"""Cases, reference and error measure for the fused YOLOv3 loss tests (a helper module, not a conftest).

The loss of ``csrc/loss_v3.hip`` has two halves, as the YOLOCSPHead loss of tests/_loss_ref.py has:

  * discrete (``assign``: grid anchors as base + shift, responsible cells, ``BboxOverlaps2D`` in its expression order,
    ``GridAssigner.assign``): fp32 rounding decides ``iou > thr`` and ``iou == gt_max``, so the fp32 evaluation on the CPU
    IS the definition.  It also yields the tables of the kernel's work buffers (``img_off``, ``gt_cell``, ``gt_max`` as
    bit patterns, ``gt_arg``).  One rule beyond the reference: a ground truth whose centre cell is off a
    level's map has no responsible cell at that level.  Nothing else changes for it: its IoUs count towards every
    anchor's maximum, and its own maximum is taken over the anchors other ground truths made responsible.
  * continuous (``reference(dtype=...)``: YOLOBBoxCoder.encode with both clamps, one-hot with smoother, BCE-with-logits
    and MSE rows, loss_weight, 'sum' / 'mean' with the reference's element counts, torch autograd for an unequal (L, 4)
    upstream matrix): float64 is what the kernels are compared with, float32 yields ``e32``.

Error measure and bound are those of DESIGN.md 4.7: ``e(x) = max |x - ref64| / max |ref64|`` (a reference of zeros
demands zeros), ``e(kernel) <= 4 * e32 + 8 * 2**-24``; per loss value, and for gradients per level and per attribute
group (xy, wh, conf, cls).

Nothing here calls the package under test.  Every case carries coverage assertions computed from ``assign`` alone.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import yolov4_oracle as O
from oracle.yolov3_oracle import V3_BASE_SIZES

FLOOR = 8 * 2.0 ** -24
GROUPS = (('xy', 0, 2), ('wh', 2, 4), ('conf', 4, 5), ('cls', 5, None))
TERMS = ('loss_cls', 'loss_conf', 'loss_xy', 'loss_wh')
NO_ARG = 2 ** 31 - 1                     # gt_arg of a ground truth no responsible anchor of its image attains
MINUS_ONE_BITS = int(torch.tensor(-1.0).view(torch.int32))
SATURATED = (0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0)
RECIPE_ASSIGNER = dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0, gt_max_assign_all=True)


def bound(e32):
    return 4.0 * e32 + FLOOR


def err(x, ref):
    """max |x - ref| / max |ref|; a reference that is all zero demands zero."""
    x, ref = x.double().reshape(-1), ref.double().reshape(-1)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    d, m = float((x - ref).abs().max()), float(ref.abs().max())
    if not math.isfinite(d):
        return math.inf
    if m == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / m


def gout_matrix(L):
    """The unequal upstream gradients, (L, 4) over [cls | conf | xy | wh]."""
    return torch.tensor([[0.7 + 0.15 * l, 1.1 - 0.1 * l, 0.9 + 0.2 * l, 1.3 - 0.05 * l] for l in range(L)],
                        dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# discrete half: fp32 on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def iou_fp32(gt, boxes):
    """BboxOverlaps2D(gt, boxes), mode 'iou', eps 1e-6, in its expression order: (G, B) fp32."""
    a1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lt = torch.max(gt[:, None, :2], boxes[None, :, :2])
    rb = torch.min(gt[:, None, 2:], boxes[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    ov = wh[..., 0] * wh[..., 1]
    union = torch.max(a1[:, None] + a2[None, :] - ov, ov.new_tensor([1e-6]))
    return ov / union


def centre_cells(case, gt):
    """(L, G) int64: the centre cell ``y * W + x`` of every ground truth at every level, -1 where it is off the map."""
    out = torch.full((case.L, gt.shape[0]), -1, dtype=torch.long)
    cx, cy = (gt[:, 0] + gt[:, 2]) * 0.5, (gt[:, 1] + gt[:, 3]) * 0.5
    for l, ((H, W), s) in enumerate(zip(case.sizes, case.strides)):
        fx, fy = torch.floor(cx / s), torch.floor(cy / s)
        on = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
        out[l] = torch.where(on, fy.long() * W + fx.long(), torch.full_like(fx, -1, dtype=torch.long))
    return out


def _first_index_of(mask, dim):
    """Smallest index along ``dim`` at which ``mask`` holds (the size of the dimension where it never does)."""
    n = mask.shape[dim]
    shape = [1, 1]
    shape[dim] = n
    idx = torch.arange(n).view(shape).expand_as(mask)
    return torch.where(mask, idx, torch.full_like(idx, n)).min(dim).values


def assign_image(case, anchors, gt, cells):
    """GridAssigner.assign for one image.  anchors (TA, 4) of all levels, gt (G, 4), cells (L, G) from ``centre_cells``.
    Returns assigned (TA,) int64, gt_max (G,) fp32 (-1 where the image has no responsible anchor), gt_arg (G,) int64."""
    cfg = case.assigner
    TA, G = anchors.shape[0], gt.shape[0]
    assigned = torch.full((TA,), -1, dtype=torch.long)
    if G == 0:
        assigned[:] = 0
        return assigned, torch.zeros(0), torch.zeros(0, dtype=torch.long)
    resp = torch.zeros(TA, dtype=torch.bool)
    off = 0
    for l, (H, W) in enumerate(case.sizes):
        flag = torch.zeros(H * W, dtype=torch.bool)
        flag[cells[l][cells[l] >= 0]] = True
        resp[off:off + H * W * case.A] = flag[:, None].expand(H * W, case.A).reshape(-1)
        off += H * W * case.A
    ov = iou_fp32(gt, anchors)
    mx = ov.max(dim=0).values
    neg = cfg['neg_iou_thr']
    if isinstance(neg, float):
        assigned[(mx >= 0) & (mx <= neg)] = 0
    else:
        assigned[(mx > neg[0]) & (mx <= neg[1])] = 0
    ov[:, ~resp] = -1.
    mx = ov.max(dim=0).values
    amx = _first_index_of(ov == mx[None, :], 0)                 # torch.max(dim=0): the first maximum
    gmx = ov.max(dim=1).values
    garg = _first_index_of(ov == gmx[:, None], 1)               # torch.max(dim=1): the first anchor attaining it
    pos = (mx > cfg['pos_iou_thr']) & resp
    assigned[pos] = amx[pos] + 1
    for i in range(G):
        if gmx[i] > cfg['min_pos_iou']:
            if cfg['gt_max_assign_all']:
                assigned[(ov[i] == gmx[i]) & resp] = i + 1
            elif resp[garg[i]]:
                assigned[garg[i]] = i + 1
    garg = torch.where(resp.any() & (gmx >= 0), garg, torch.full_like(garg, NO_ARG))
    return assigned, gmx, garg


def grid_anchors(case):
    """Per level (H*W*A, 4) fp32, index (y*W + x)*A + a: base anchor (centre stride / 2) + shift."""
    return O.grid_anchors(case.sizes, case.base_sizes, case.strides)


def assign(case):
    """The whole batch.  assigned (N, TA) int64; img_off (N + 1,); gt_cell (L, G); gt_max (G,) int32 bit patterns;
    gt_arg (G,) int64 anchor index inside the image (NO_ARG where nothing is responsible); iou: per image the (G_n, TA)
    fp32 IoUs, for the coverage assertions."""
    anchors = torch.cat(grid_anchors(case))
    TA = anchors.shape[0]
    counts = [int(b.shape[0]) for b in case.boxes]
    img_off = torch.tensor([0] + counts).cumsum(0)
    allgt = torch.cat(case.boxes).reshape(-1, 4)
    gt_cell = centre_cells(case, allgt)
    assigned = torch.zeros(case.N, TA, dtype=torch.long)
    gmax, garg, ious = [], [], []
    for n in range(case.N):
        g0, g1 = int(img_off[n]), int(img_off[n + 1])
        a, m, r = assign_image(case, anchors, case.boxes[n], gt_cell[:, g0:g1])
        assigned[n] = a
        gmax.append(m)
        garg.append(r)
        ious.append(iou_fp32(case.boxes[n], anchors) if g1 > g0 else torch.zeros(0, TA))
    gt_max = torch.cat(gmax).float().view(torch.int32) if case.G else torch.zeros(0, dtype=torch.int32)
    return SimpleNamespace(assigned=assigned, img_off=img_off, gt_cell=gt_cell, gt_max=gt_max,
                           gt_arg=torch.cat(garg) if case.G else torch.zeros(0, dtype=torch.long), iou=ious,
                           anchors=anchors, TA=TA)


def level_ids(case, asg, l):
    """(N, H*W*A) ids of level l."""
    off = sum(h * w * case.A for h, w in case.sizes[:l])
    H, W = case.sizes[l]
    return asg.assigned[:, off:off + H * W * case.A]


# ---------------------------------------------------------------------------------------------------------------------
# continuous half: ``dtype`` on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def encode(anchors, gt, stride, dtype, eps=1e-6):
    """YOLOBBoxCoder.encode (yolo_bbox_coder.py:26-59) in ``dtype``: both clamps."""
    anchors, gt = anchors.to(dtype), gt.to(dtype)
    xg, yg = (gt[..., 0] + gt[..., 2]) * 0.5, (gt[..., 1] + gt[..., 3]) * 0.5
    wg, hg = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
    xc, yc = (anchors[..., 0] + anchors[..., 2]) * 0.5, (anchors[..., 1] + anchors[..., 3]) * 0.5
    w, h = anchors[..., 2] - anchors[..., 0], anchors[..., 3] - anchors[..., 1]
    wt = torch.log((wg / w).clamp(min=eps))
    ht = torch.log((hg / h).clamp(min=eps))
    xt = ((xg - xc) / stride + 0.5).clamp(eps, 1 - eps)
    yt = ((yg - yc) / stride + 0.5).clamp(eps, 1 - eps)
    return torch.stack([xt, yt, wt, ht], dim=-1)


def targets(case, asg, l, dtype):
    """(N, H*W*A, 5 + C) target map and the positive / positive-or-negative masks of level l (yolo_head.py:513-560)."""
    ids = level_ids(case, asg, l)
    anchors = grid_anchors(case)[l]
    allgt = torch.cat(case.boxes).reshape(-1, 4)
    labels = torch.cat(case.labels).reshape(-1)
    t = torch.zeros(case.N, ids.shape[1], 5 + case.C, dtype=dtype)
    n, k = (ids > 0).nonzero(as_tuple=True)
    if n.numel():
        g = asg.img_off[n] + ids[n, k] - 1
        t[n, k, :4] = encode(anchors[k], allgt[g], case.strides[l], dtype)
        t[n, k, 4] = 1
        one_hot = F.one_hot(labels[g], num_classes=case.C).to(dtype)
        if case.smoother != 0:
            one_hot = one_hot * (1 - case.smoother) + case.smoother / case.C
        t[n, k, 5:] = one_hot
    return t, (ids > 0).to(dtype), (ids >= 0).to(dtype)


def make_maps(case, asg):
    """The L prediction maps, logical NCHW (N, A*(5+C), H, W) fp32: randn * 2, then what the case plants."""
    g = torch.Generator().manual_seed(case.seed)
    maps = [torch.randn(case.N, case.A * (5 + case.C), H, W, generator=g) * 2.0 for H, W in case.sizes]
    if case.name == 'clamps':
        # the xy logits of the positives sit near their targets: the group's largest gradient is then a few hundredths,
        # and a target that moves by the 1e-6 of a clamp shows in the relative measure
        attr = 5 + case.C
        for l, (H, W) in enumerate(case.sizes):
            t, pos, _ = targets(case, asg, l, torch.float32)
            rows = maps[l].view(case.N, case.A, attr, H, W).permute(0, 3, 4, 1, 2).reshape(case.N, -1, attr).clone()
            near = torch.logit(t[..., :2].clamp(0.02, 0.98)) + 0.05 * torch.randn(t[..., :2].shape, generator=g)
            rows[..., :2] = torch.where(pos.bool().unsqueeze(-1), near, rows[..., :2])
            maps[l] = rows.view(case.N, H, W, case.A, attr).permute(0, 3, 4, 1, 2).reshape(case.N, case.A * attr, H, W).contiguous()
    if case.name == 'saturated':
        vals = torch.tensor(SATURATED)
        attr = 5 + case.C
        for l, (H, W) in enumerate(case.sizes):
            rows = maps[l].view(case.N, case.A, attr, H, W).permute(0, 3, 4, 1, 2).reshape(case.N, -1, attr).clone()
            ids = level_ids(case, asg, l)
            for kind in (ids > 0, ids == 0, ids < 0):
                n, k = kind.nonzero(as_tuple=True)
                for i in range(min(int(n.numel()), 14)):
                    rows[n[i], k[i]] = vals[(i + torch.arange(attr)) % len(SATURATED)]
            maps[l] = rows.view(case.N, H, W, case.A, attr).permute(0, 3, 4, 1, 2).reshape(case.N, case.A * attr, H, W).contiguous()
    return maps


def exact_count_maps(case):
    """Part 3c: every objectness and class logit is 64.0 (bce(64, 0) == 64 exactly in fp32), the box logits random."""
    g = torch.Generator().manual_seed(case.seed + 7)
    attr = 5 + case.C
    maps = []
    for H, W in case.sizes:
        m = torch.randn(case.N, case.A, attr, H, W, generator=g)
        m[:, :, 4:] = 64.0
        maps.append(m.view(case.N, case.A * attr, H, W))
    return maps


def reference(case, asg, maps, dtype, gout=None):
    """losses (L, 4) [cls | conf | xy | wh] and the maps' gradients (logical NCHW) under ``gout`` (default
    ``gout_matrix``), in ``dtype``."""
    leaves = [m.detach().to(dtype, copy=True).requires_grad_(True) for m in maps]        # never the caller's tensors
    attr = 5 + case.C
    rows = []
    for l, pm in enumerate(leaves):
        p = pm.permute(0, 2, 3, 1).reshape(case.N, -1, attr)
        t, pos, pn = targets(case, asg, l, dtype)
        pos_ = pos.unsqueeze(-1)
        terms = [F.binary_cross_entropy_with_logits(p[..., 5:], t[..., 5:], reduction='none') * pos_,
                 F.binary_cross_entropy_with_logits(p[..., 4], t[..., 4], reduction='none') * pn,
                 F.binary_cross_entropy_with_logits(p[..., :2], t[..., :2], reduction='none') * pos_,
                 F.mse_loss(p[..., 2:4], t[..., 2:4], reduction='none') * pos_]
        rows.append(torch.stack([case.weights[u] * (v.mean() if case.reduction[u] == 'mean' else v.sum())
                                 for u, v in enumerate(terms)]))
    losses = torch.stack(rows)
    assert losses.dtype == dtype
    (losses * (gout_matrix(case.L) if gout is None else gout).to(dtype)).sum().backward()
    return SimpleNamespace(losses=losses.detach(), grads=[x.grad for x in leaves])


def group_view(case, grad, lo, hi):
    """The attribute range [lo, hi) of a logical NCHW gradient: (N, A, hi - lo, H, W)."""
    N, _, H, W = grad.shape
    return grad.reshape(N, case.A, 5 + case.C, H, W)[:, :, lo:hi]


def loss_errors(x, ref):
    x, ref = x.double(), ref.double()
    e = torch.zeros_like(ref)
    for i in range(ref.numel()):
        e.view(-1)[i] = err(x.view(-1)[i], ref.view(-1)[i])
    return e


def grad_errors(case, grads, ref_grads):
    """{(level, group): e}."""
    return {(l, name): err(group_view(case, grads[l], lo, hi), group_view(case, ref_grads[l], lo, hi))
            for l in range(case.L) for name, lo, hi in GROUPS}


def describe(tag, e, e32):
    return f'{tag}: e = {e:.3e}  e32 = {e32:.3e}  bound = {bound(e32):.3e}'


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _box(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _random_boxes(g, n, W, H, lo=4.0, hi=None):
    """Centres uniform in [0, W) x [0, H) (kept: the extents are not clipped), w / h log-uniform in [lo, hi]."""
    hi = hi or 0.9 * max(W, H)
    c = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)]) * 0.999
    wh = torch.exp(torch.rand(n, 2, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))
    return torch.cat([c - wh / 2, c + wh / 2], 1)


def _case(name, strides, base_sizes, sizes, C, boxes, seed, assigner=None, smoother=0.0, weights=(1.0, 1.0, 2.0, 2.0),
          reduction=('sum',) * 4, layouts=None, label_seed=None):
    boxes = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4) for b in boxes]
    g = torch.Generator().manual_seed(seed + 1000 if label_seed is None else label_seed)
    labels = [torch.randint(0, C, (int(b.shape[0]),), generator=g) for b in boxes]
    L, A = len(strides), len(base_sizes[0])
    assert all(len(b) == A for b in base_sizes) and len(base_sizes) == len(sizes) == L
    return SimpleNamespace(name=name, N=len(boxes), L=L, A=A, C=C, strides=list(strides),
                           base_sizes=[[tuple(x) for x in b] for b in base_sizes], sizes=[tuple(s) for s in sizes],
                           boxes=boxes, labels=labels, G=sum(int(b.shape[0]) for b in boxes), seed=seed,
                           assigner=dict(RECIPE_ASSIGNER, **(assigner or {})), smoother=smoother, weights=tuple(weights),
                           reduction=tuple(reduction), layouts=layouts or ['nchw'] * L)


def rows_of(case):
    return [case.N * h * w * case.A for h, w in case.sizes]


def _all_on_map(case, asg):
    assert bool((asg.gt_cell >= 0).all()), f'{case.name}: a centre is off a map'


def _kinds(case, asg):
    a = asg.assigned
    return int((a > 0).sum()), int((a == 0).sum()), int((a < 0).sum())


# -- levels_anchors ---------------------------------------------------------------------------------------------------
def _la_1x8(all_):
    # one level of 8 anchors; anchors 2 and 5 are the same box: every IoU ties between them
    base = [[(10, 14), (16, 30), (30, 22), (22, 40), (44, 30), (30, 22), (60, 50), (12, 50)]]
    g = torch.Generator().manual_seed(11)
    boxes = [torch.cat([_random_boxes(g, 5, 96, 64, 6, 60), torch.tensor([_box(40., 24., 28., 21.)])]),
             torch.cat([_random_boxes(g, 4, 96, 64, 6, 60), torch.tensor([_box(70., 41., 33., 20.)])])]
    return _case('la_1x8_all' if all_ else 'la_1x8_first', [16], base, [(4, 6)], 3, boxes, seed=12,
                 assigner=dict(pos_iou_thr=0.9, neg_iou_thr=0.4, min_pos_iou=0.1, gt_max_assign_all=all_),
                 reduction=('sum', 'mean', 'sum', 'mean') if all_ else ('mean', 'sum', 'mean', 'sum'), weights=(0.5, 1.5, 2.5, 3.5))


def _check_la_1x8(case, asg):
    _all_on_map(case, asg)
    A = case.A
    twins = 0
    for n in range(case.N):
        iou = asg.iou[n]
        g0 = int(asg.img_off[n])
        for i in range(iou.shape[0]):
            cell = int(asg.gt_cell[0, g0 + i])
            lo, hi = cell * A + 2, cell * A + 5
            gmax = torch.tensor(int(asg.gt_max[g0 + i]), dtype=torch.int32).view(torch.float32)
            if not (iou[i, lo] == iou[i, hi] and iou[i, lo] == gmax and float(gmax) > case.assigner['min_pos_iou']
                    and float(gmax) <= case.assigner['pos_iou_thr']):
                continue
            # the pair ties at this ground truth's maximum, below pos_iou_thr: only the claim can make them positive
            if case.assigner['gt_max_assign_all']:
                twins += int(asg.assigned[n, lo] == i + 1 and asg.assigned[n, hi] == i + 1)
            else:
                twins += int(asg.assigned[n, lo] == i + 1 and asg.assigned[n, hi] != i + 1 and int(asg.gt_arg[g0 + i]) == lo)
    assert twins >= 2, f'{case.name}: no ground truth whose maximum ties between the identical anchors 2 and 5 ({twins})'


def case_la_2x1():
    g = torch.Generator().manual_seed(13)
    boxes = [_random_boxes(g, 6, 96, 64, 8, 70), _random_boxes(g, 3, 96, 64, 8, 70), _random_boxes(g, 5, 96, 64, 8, 70)]
    return _case('la_2x1', [32, 8], [[(50, 40)], [(14, 18)]], [(2, 3), (8, 12)], 4, boxes, seed=14)


def case_la_5x2():
    g = torch.Generator().manual_seed(15)
    base = [[(50, 44), (30, 56)], [(28, 22), (16, 30)], [(14, 11), (8, 15)], [(7, 6), (4, 8)], [(3, 4), (2, 5)]]
    boxes = [_random_boxes(g, 4, 64, 64, 3, 60), _random_boxes(g, 3, 64, 64, 3, 60)]
    for l, per_level in enumerate(base):           # a box near an anchor of every level, so that every level has positives
        w, h = per_level[l % 2]
        cx, cy = [(33., 33.), (49., 17.), (9., 57.), (29., 5.), (59., 39.)][l]      # a cell centre of the level, plus one
        boxes[l % 2] = torch.cat([boxes[l % 2], torch.tensor([_box(cx, cy, w * 1.1, h * 0.9)])])
    return _case('la_5x2', [64, 32, 16, 8, 4], base, [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16)], 5, boxes, seed=16,
                 assigner=dict(neg_iou_thr=(0.05, 0.5)), layouts=['nhwc', 'nchw', 'nhwc', 'nchw', 'nhwc'])


def case_one_class():
    """C = 1 with label smoothing.  Image 0 also holds the same 10 x 15 box twice on a stride-8 cell centre: it passes
    pos_iou_thr on the (8, 12) anchor (0.64) and on the (12, 18) anchor (0.69, its maximum).  The claims give the second
    anchor to the LAST twin; the first anchor is no maximum, so it keeps the argmax over ground truths: the FIRST twin."""
    g = torch.Generator().manual_seed(17)
    boxes = [torch.cat([_random_boxes(g, 5, 64, 64, 6, 60), torch.tensor([_box(36., 36., 10., 15.)] * 2)]),
             _random_boxes(g, 4, 64, 64, 6, 60)]
    return _case('one_class', [16, 8], [[(30, 40), (44, 28), (20, 20)], [(8, 12), (14, 9), (12, 18)]], [(4, 4), (8, 8)], 1,
                 boxes, seed=18, smoother=0.1, layouts=['nchw', 'nhwc'])


def _check_one_class(case, asg):
    _check_generic(case, asg)
    assert case.C == 1 and case.smoother != 0
    iou, ids = asg.iou[0], asg.assigned[0]
    i, j = 5, 6                                              # the twins
    assert torch.equal(case.boxes[0][i], case.boxes[0][j])
    off = case.sizes[0][0] * case.sizes[0][1] * case.A
    k = off + (4 * 8 + 4) * case.A                           # level 1, cell (4, 4): its three anchors
    assert float(iou[i, k]) > 0.5 and float(iou[i, k + 2]) > float(iou[i, k]) and bool(iou[i, k] == iou[:, k].max())
    assert int(ids[k]) == i + 1 and int(ids[k + 2]) == j + 1, (int(ids[k]), int(ids[k + 2]))


# -- row_counts -------------------------------------------------------------------------------------------------------
def case_row_counts():
    """N = 1, A = 1: rows 1 (a 1x1 map), 256 (256x1: W = 1) and 257 (1x257: H = 1; 257 is prime, so nothing else gives
    it).  The two long maps share only their first cell, so this case leans on the off-map rule: the boxes down the
    column are off the row map and the other way round.  One box sits in the LAST cell of the 1x257 map: the single
    valid row of the dense launch's last workgroup is a positive.  The 1x1 map's only row is responsible but no ground
    truth's best anchor, so it is the negative row the exact count needs at every level."""
    boxes = [[_box(4., 4., 9., 9.), _box(3., 5., 12., 10.),                            # on every map
              _box(4., 8 * 100 + 3., 10., 12.), _box(5., 8 * 255 + 4., 14., 9.),       # column: cells 100 and 255 (the last)
              _box(8 * 37 + 2., 3., 9., 13.), _box(8 * 255 + 5., 4., 12., 11.),        # row: cells 37 and 255
              _box(8 * 256 + 4., 4., 10., 10.)]]                                       # row: cell 256, the 257th row
    return _case('row_counts', [64, 8, 8], [[(40, 44)], [(10, 11)], [(11, 10)]], [(1, 1), (256, 1), (1, 257)], 3, boxes,
                 seed=20)


def _check_row_counts(case, asg):
    r = rows_of(case)
    assert r[0] < 64 and r[1] == 256 and r[2] == 257, r
    assert case.sizes[0] == (1, 1) and case.sizes[1][1] == 1 and case.sizes[2][0] == 1 and case.layouts[0] == 'nchw'
    assert int(level_ids(case, asg, 2)[0, 256]) > 0, 'the 257th row of level 2 is not a positive'
    assert int(level_ids(case, asg, 1)[0, 255]) > 0
    assert int(asg.gt_cell[0, 0]) == 0 and int(level_ids(case, asg, 0)[0, 0]) == 0    # responsible, unclaimed: a negative
    assert int((asg.gt_cell < 0).sum()) > 0


# -- many_images / many_gts / no_gt -----------------------------------------------------------------------------------
def case_many_images():
    N = 257
    boxes = [torch.zeros(0, 4) for _ in range(N)]
    boxes[5] = torch.tensor([_box(10., 20., 20., 30.), _box(20., 50., 30., 24.)])
    boxes[100] = torch.tensor([_box(16., 16., 40., 40.)])
    boxes[255] = torch.tensor([_box(8., 40., 12., 30.), _box(25., 10., 14., 16.), _box(25., 10., 14., 16.)])
    boxes[256] = torch.tensor([_box(15., 45., 26., 28.), _box(12., 12., 50., 60.)])
    return _case('many_images', [64, 32], [[(50, 60), (30, 40)], [(14, 16), (26, 28)]], [(1, 1), (2, 1)], 2, boxes, seed=22,
                 layouts=['nchw', 'nhwc'])


def _check_many_images(case, asg):
    _all_on_map(case, asg)
    assert case.N + 1 > 256 and case.boxes[-1].shape[0] > 0
    assert case.boxes[0].shape[0] == 0 and case.boxes[128].shape[0] == 0
    assert int((asg.assigned[256] > 0).sum()) > 0 and int((asg.assigned[0] != 0).sum()) == 0


def case_many_gts():
    g = torch.Generator().manual_seed(23)
    boxes = [_random_boxes(g, 40, 64, 64, 3, 60), _random_boxes(g, 300, 64, 64, 3, 60)]
    return _case('many_gts', [16, 8], [[(30, 40), (44, 28), (20, 20)], [(8, 12), (14, 9), (12, 18)]], [(4, 4), (8, 8)], 4,
                 boxes, seed=24)


def _check_many_gts(case, asg):
    _all_on_map(case, asg)
    assert case.G * case.L * case.A > 256 and case.G > 256
    assert case.boxes[0].shape[0] == 40 and case.boxes[1].shape[0] == 300
    assert int(asg.assigned.max()) > 256                      # an id beyond the first workgroup's ground truths


def case_no_gt():
    return _case('no_gt', [16, 8], [[(30, 40), (44, 28), (20, 20)], [(8, 12), (14, 9), (12, 18)]], [(3, 5), (6, 10)], 5,
                 [torch.zeros(0, 4), torch.zeros(0, 4)], seed=26, layouts=['nchw', 'nhwc'])


# -- thresholds -------------------------------------------------------------------------------------------------------
def _thresholds(tag, neg, min_pos):
    """Stride 32, one base anchor (16, 30): its box in cell 0 is [8, 1, 24, 31], in cell 1 [40, 1, 56, 31]."""
    boxes = [[[8., 1., 16., 31.], [40., 1., 44., 31.]]]
    return _case('thresholds_' + tag, [32], [[(16, 30)]], [(2, 3)], 2, boxes, seed=28,
                 assigner=dict(pos_iou_thr=0.5, neg_iou_thr=neg, min_pos_iou=min_pos))


def _check_thresholds(case, asg):
    _all_on_map(case, asg)
    iou = asg.iou[0]
    half, quarter = torch.tensor(0.5), torch.tensor(0.25)
    assert torch.equal(asg.anchors[0], torch.tensor([8., 1., 24., 31.]))
    assert iou[0, 0].view(torch.int32) == half.view(torch.int32), 'IoU of gt 0 with anchor 0 is not 0.5 bit for bit'
    assert iou[1, 1].view(torch.int32) == quarter.view(torch.int32), 'IoU of gt 1 with anchor 1 is not 0.25 bit for bit'
    assert float(iou[0, 1]) == 0 and float(iou[1, 0]) == 0
    assert asg.gt_max.tolist() == [int(half.view(torch.int32)), int(quarter.view(torch.int32))]
    cfg = case.assigner
    assert float(iou[0, 0]) == cfg['pos_iou_thr']
    ids = asg.assigned[0].tolist()
    tag = case.name.split('_', 1)[1]
    if tag in ('tuple', 'min_equal'):
        assert float(iou[1, 1]) == cfg['neg_iou_thr'][0] and float(iou[0, 0]) == cfg['neg_iou_thr'][1]
        if tag == 'min_equal':
            assert float(iou[0, 0]) == cfg['min_pos_iou']
        assert ids == [0, -1, -1, -1, -1, -1], ids          # == neg hi: negative; == neg lo: ignored; no claim
    elif tag == 'claim':
        assert ids == [1, 2, -1, -1, -1, -1], ids
    else:
        assert float(iou[0, 0]) == cfg['neg_iou_thr']
        assert ids == [0, 0, 0, 0, 0, 0], ids


# -- clamps -----------------------------------------------------------------------------------------------------------
def case_clamps():
    """Stride 16, 4x4 map, anchors (16, 16) and (24, 12).  min_pos_iou = -0.5 lets a ground truth whose best IoU is 0
    (the zero-width one, first of its image so that later claims overwrite it) claim its responsible anchors."""
    up = float(torch.nextafter(torch.tensor(40.), torch.tensor(100.)))
    below = float(torch.nextafter(torch.tensor(40.), torch.tensor(0.)))
    img0 = [[8., 8., 24., 24.],                    # centre (16, 16): the left and top border of cell (1, 1) -> eps, eps
            [24., 40., below, 52.],                # centre x one fp32 step below 32 -> 1 - eps
            [40., 6., up, 20.],                    # 3.8e-6 wide: under 1e-6 x the anchors' widths -> log(eps) by the clamp
            [50., 40., 62., 56.]]
    img1 = [[10., 34., 10., 50.]]                  # zero width: ratio 0 -> log(eps)
    img1 += [[36., 36., 50., 46.]] * 8             # the same box eight times
    return _case('clamps', [16], [[(16, 16), (24, 12)]], [(4, 4)], 3, [img0, img1], seed=30,
                 assigner=dict(min_pos_iou=-0.5))


def _check_clamps(case, asg):
    _all_on_map(case, asg)
    b0 = case.boxes[0]
    assert float((b0[1, 0] + b0[1, 2]) * 0.5) == float(torch.nextafter(torch.tensor(32.), torch.tensor(0.)))
    assert 0 < float(b0[2, 2] - b0[2, 0]) < 1e-6 * 16 and float(case.boxes[1][0, 2] - case.boxes[1][0, 0]) == 0
    t, pos, _ = targets(case, asg, 0, torch.float32)
    ids = level_ids(case, asg, 0)
    eps, eps_hi, leps = torch.tensor(1e-6), torch.tensor(1 - 1e-6, dtype=torch.float32), torch.log(torch.tensor(1e-6))

    def rows(n, gid):
        return t[n][ids[n] == gid]
    r = rows(0, 1)
    assert r.shape[0] >= 1 and bool((r[:, 0] == eps).all()) and bool((r[:, 1] == eps).all()), 'no eps xy target'
    r = rows(0, 2)
    assert r.shape[0] >= 1 and bool((r[:, 0] == eps_hi).all()), 'no 1 - eps x target'
    r = rows(0, 3)
    assert r.shape[0] >= 1 and bool((r[:, 2] == leps).all()), 'the narrow box is not clamped'
    r = rows(1, 1)
    assert r.shape[0] >= 1 and bool((r[:, 2] == leps).all()), 'the zero-width box claims nothing'
    assert int((ids[1] == 9).sum()) >= 1 and int(((ids[1] >= 2) & (ids[1] <= 8)).sum()) == 0   # the last duplicate wins


# -- off_map ----------------------------------------------------------------------------------------------------------
def case_off_map():
    """Level 0: 2x2 at stride 32 (64 x 64); level 1: 3x3 at stride 16 (48 x 48).  Image 0 holds a box with centre x = 48 =
    W * stride of level 1 exactly (ON the coarser map, off the finer one) and a box with a negative centre x (off BOTH
    maps: it has no responsible cell anywhere), beside three boxes inside both maps."""
    img0 = [_box(48., 20., 20., 24.), _box(-4., 20., 32., 20.), _box(20., 20., 18., 22.), _box(36., 40., 14., 12.),
            _box(10., 38., 30., 28.)]
    img1 = [_box(30., 30., 30., 30.), _box(12., 12., 14., 18.)]
    return _case('off_map', [32, 16], [[(40, 40), (24, 50), (50, 24)], [(14, 18), (20, 14), (30, 30)]], [(2, 2), (3, 3)], 3,
                 [img0, img1], seed=32)


def _check_off_map(case, asg):
    c = asg.gt_cell
    assert float((case.boxes[0][0, 0] + case.boxes[0][0, 2]) * 0.5) == case.sizes[1][1] * case.strides[1]
    assert int(c[0, 0]) == 1 and int(c[1, 0]) == -1                  # on the coarser map (cell (0, 1)), off the finer
    assert int(c[0, 1]) == -1 and int(c[1, 1]) == -1                 # the negative centre: off both
    assert bool((c[:, 2:] >= 0).all())
    # the box without a responsible cell still has a maximum (over the others' responsible anchors) and still claims
    gmax1 = float(torch.tensor(int(asg.gt_max[1]), dtype=torch.int32).view(torch.float32))
    assert gmax1 > 0 and int((asg.assigned[0] == 2).sum()) >= 1
    assert float(asg.iou[0][1].max()) > 0


# -- saturated / layouts / recipe -------------------------------------------------------------------------------------
def case_saturated():
    g = torch.Generator().manual_seed(33)
    boxes = [_random_boxes(g, 8, 64, 64, 6, 60), _random_boxes(g, 8, 64, 64, 6, 60)]
    return _case('saturated', [16, 8], [[(30, 40), (44, 28), (20, 20)], [(8, 12), (14, 9), (12, 18)]], [(4, 4), (8, 8)], 4,
                 boxes, seed=34, assigner=dict(neg_iou_thr=0.1), layouts=['nhwc', 'nchw'])


def _check_saturated(case, asg):
    _all_on_map(case, asg)
    maps = make_maps(case, asg)
    attr = 5 + case.C
    for l, (H, W) in enumerate(case.sizes):
        rows = maps[l].view(case.N, case.A, attr, H, W).permute(0, 3, 4, 1, 2).reshape(case.N, -1, attr)
        ids = level_ids(case, asg, l)
        for kind, name in ((ids > 0, 'positive'), (ids == 0, 'negative'), (ids < 0, 'ignored')):
            assert int(kind.sum()) >= len(SATURATED), f'saturated level {l}: fewer than 7 {name} rows'
            conf = set(rows[kind][:, 4].tolist())
            assert conf >= set(SATURATED), f'saturated level {l}: {name} rows miss an objectness value'
            assert set(rows[kind][:, 0].tolist()) >= set(SATURATED) and set(rows[kind][:, attr - 1].tolist()) >= set(SATURATED)


def case_layouts():
    """Recipe anchors and strides, 80 classes, a 96 x 64 image: maps 2x3, 4x6, 8x12.  Run contiguous, channels-last and as
    a strided view by the GPU test; the reference is the same for the three."""
    g = torch.Generator().manual_seed(35)
    boxes = [_random_boxes(g, 7, 96, 64, 6, 90), _random_boxes(g, 5, 96, 64, 6, 90)]
    return _case('layouts', [32, 16, 8], V3_BASE_SIZES, [(2, 3), (4, 6), (8, 12)], 80, boxes, seed=36)


def case_recipe():
    """Part 3c only: the level shapes of a 608 x 608 recipe step (19 / 38 / 76, 45 486 rows for N = 2), few classes."""
    g = torch.Generator().manual_seed(37)
    boxes = [_random_boxes(g, 9, 608, 608, 8, 400), _random_boxes(g, 6, 608, 608, 8, 400)]
    return _case('recipe', [32, 16, 8], V3_BASE_SIZES, [(19, 19), (38, 38), (76, 76)], 4, boxes, seed=38,
                 layouts=['nhwc', 'nchw', 'nhwc'])


def _check_generic(case, asg):
    _all_on_map(case, asg)
    pos, neg, ign = _kinds(case, asg)
    assert pos > 0 and neg > 0, (case.name, pos, neg, ign)


def _check_no_gt(case, asg):
    assert case.G == 0 and int((asg.assigned != 0).sum()) == 0


def _check_la_5x2(case, asg):
    _check_generic(case, asg)
    assert case.L == 5 and case.A == 2 and _kinds(case, asg)[2] > 0
    for l in range(case.L):
        assert int((level_ids(case, asg, l) > 0).sum()) > 0, f'la_5x2: level {l} has no positive'


CASES = dict(
    la_1x8_first=(lambda: _la_1x8(False), _check_la_1x8),
    la_1x8_all=(lambda: _la_1x8(True), _check_la_1x8),
    la_2x1=(case_la_2x1, _check_generic),
    la_5x2=(case_la_5x2, _check_la_5x2),
    one_class=(case_one_class, _check_one_class),
    row_counts=(case_row_counts, _check_row_counts),
    many_images=(case_many_images, _check_many_images),
    many_gts=(case_many_gts, _check_many_gts),
    no_gt=(case_no_gt, _check_no_gt),
    thresholds_tuple=(lambda: _thresholds('tuple', (0.25, 0.5), 0.6), _check_thresholds),
    thresholds_min_equal=(lambda: _thresholds('min_equal', (0.25, 0.5), 0.5), _check_thresholds),
    thresholds_claim=(lambda: _thresholds('claim', (0.25, 0.5), 0.0), _check_thresholds),
    thresholds_float=(lambda: _thresholds('float', 0.5, 0.6), _check_thresholds),
    clamps=(case_clamps, _check_clamps),
    off_map=(case_off_map, _check_off_map),
    saturated=(case_saturated, _check_saturated),
    layouts=(case_layouts, _check_generic),
)
COUNT_CASES = ('row_counts', 'many_images', 'many_gts', 'recipe')        # part 3c
_BUILDERS = dict(CASES, recipe=(case_recipe, _check_generic))
_case_cache = {}


def get_case(name):
    """(case, assignment), built once; the case's coverage assertions run here."""
    if name not in _case_cache:
        build, check = _BUILDERS[name]
        case = build()
        assert case.name == name, (case.name, name)
        asg = assign(case)
        if name != 'recipe':
            assert sum(rows_of(case)) <= 3000, f'{name}: {sum(rows_of(case))} anchor boxes'
        check(case, asg)
        _case_cache[name] = (case, asg)
    return _case_cache[name]


_ref_cache = {}


def references(name):
    """(case, asg, maps, ref64, e32): e32.losses (L, 4), e32.grads {(level, group): e}; computed once per process."""
    if name not in _ref_cache:
        case, asg = get_case(name)
        maps = make_maps(case, asg)
        r64 = reference(case, asg, maps, torch.float64)
        r32 = reference(case, asg, maps, torch.float32)
        e32 = SimpleNamespace(losses=loss_errors(r32.losses, r64.losses), grads=grad_errors(case, r32.grads, r64.grads))
        _ref_cache[name] = (case, asg, maps, r64, e32, r32)
    return _ref_cache[name][:5]


def reference32(name):
    references(name)
    return _ref_cache[name][5]


def count_expectation(case, asg):
    """Part 3c: per level (#rows with id == 0, #positives); every level must have a negative row."""
    out = []
    for l in range(case.L):
        ids = level_ids(case, asg, l)
        neg, pos = int((ids == 0).sum()), int((ids > 0).sum())
        assert neg >= 1, f'{case.name}: level {l} has no negative row'
        out.append((neg, pos))
    return out
