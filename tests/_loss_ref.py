"""Cases, float64 reference and error measure for the fused YOLOCSPHead loss tests (a helper module, not a conftest).

The loss has a discrete half (``oracle.responsible_indices``: decided by fp32 rounding, kept in fp32 as the definition)
and a continuous half (``oracle.head_loss(dtype=...)``: float32 is the reference, float64 what the kernels are compared
with).  Everything here runs on the CPU, so the host suite checks every case's coverage conditions and computes the
reference's own fp32 error ``e32`` -- the number the GPU bound is set from -- before anything reaches a GPU.

Error measure per tensor: ``e(x) = max |x - ref64| / max |ref64|`` (per level for draw / dbias / conf_t, relative error
for each of the nine loss values).  Bound: ``e(kernel) <= 4 * e32 + 8 * 2**-24`` (``bound``); the reasoning is in
DESIGN.md 4.7.

Box centres stay inside the image (``0 <= cx < W * stride``, ``0 <= cy < H * stride``); box EXTENTS may reach outside it
where a level's anchors are larger than the image (the 96-pixel-wide ``edges`` image at stride 32).
"""
import math
from types import SimpleNamespace

import torch

from oracle import yolov4_oracle as O

WEIGHTS = dict(loss_cls=[1.0, 0.7, 1.3], loss_conf=[0.9, 1.1, 1.0], loss_bbox=[1.2, 1.0, 0.8])   # upstream gradients
SMALL_BASE = [[(10, 12), (16, 30), (30, 20)], [(30, 60), (60, 45), (58, 100)], [(100, 90), (150, 190), (300, 320)]]
FLOOR = 8 * 2.0 ** -24
DENSE_BWD_TRIP = 2048 * 256          # 16-byte chunks one trip of the dense backward's grid-stride loop covers per level


def bound(e32):
    return 4.0 * e32 + FLOOR


def err(x, ref):
    """max |x - ref| / max |ref|; a reference that is all zero demands zero."""
    x, ref = x.double().reshape(-1), ref.double().reshape(-1)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    d, m = float((x - ref).abs().max()), float(ref.abs().max())
    if m == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / m


def gout_matrix(L):
    """The unequal upstream gradients as the (L, 3) matrix [cls | conf | bbox] the kernels take."""
    return torch.tensor([[WEIGHTS['loss_cls'][l], WEIGHTS['loss_conf'][l], WEIGHTS['loss_bbox'][l]] for l in range(L)],
                        dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _box(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _random_boxes(g, n, H, W, lo=8.0, hi=400.0):
    """bench.synthetic_gts' distribution on an H x W image: centre uniform, w / h log-uniform, clipped to the image."""
    llo, lhi = math.log(lo), math.log(hi)
    c = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)])
    wh = torch.exp(torch.rand(n, 2, generator=g) * (lhi - llo) + llo)
    b = torch.cat([c - wh / 2, c + wh / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, W)
    b[:, 1::2] = b[:, 1::2].clamp(0, H)
    return b


def _first_box(base_sizes, strides):
    """A box that matches base anchor 0 of every level but the first (its k = 0 slot is the FIRST slot of those levels
    when it is box 0): geometric mean of the anchors concerned."""
    ws = [base_sizes[l][0][0] for l in range(1, len(strides))]
    hs = [base_sizes[l][0][1] for l in range(1, len(strides))]
    w = math.exp(sum(math.log(v) for v in ws) / len(ws))
    h = math.exp(sum(math.log(v) for v in hs) / len(hs))
    s = strides[-1]
    return _box(1.25 * s, 1.25 * s, round(w), round(h))


def _last_box(base_sizes, strides, H, W):
    """A box that matches the LAST base anchor of every level but the last and has a down neighbour there (its k = 4
    slot is the last slot of those levels when it is the last box): y / stride has a fraction above one half."""
    A = len(base_sizes[0])
    ws = [base_sizes[l][A - 1][0] for l in range(len(strides) - 1)]
    hs = [base_sizes[l][A - 1][1] for l in range(len(strides) - 1)]
    w = math.exp(sum(math.log(v) for v in ws) / len(ws))
    h = math.exp(sum(math.log(v) for v in hs) / len(hs))
    s = strides[-2]
    return _box(W // 2 + 3.0, 2 * s + 0.8125 * s, round(w), round(h))


def _edge_boxes(base_sizes, strides, H, W, C):
    """The hand-built boxes of the ``edges`` case, every kind at every level (centres in cell units x stride)."""
    boxes, labels = [], []
    nl = max(C, 1)

    def add(b, lab):
        boxes.append([float(v) for v in b])
        labels.append(lab % nl)

    for l, s in enumerate(strides):
        fh, fw = H // s, W // s
        assert fh >= 3 and fw >= 3
        bw, bh = base_sizes[l][1]
        w, h = bw * 1.25, bh * 0.75
        add(_box(2.0 * s, 1.0 * s, w, h), 0)                       # centre on a cell border in x and in y; y = 1.0: not > 1
        add(_box(1.0 * s, 2.0 * s, w, h), nl - 1)                  # x = 1.0 exactly: rem 0 < 0.5 but not > 1
        add(_box(1.5 * s, 2.5 * s, w, h), 1)                       # exactly half a cell: rem 0.5 is not < 0.5
        add(_box(0.5 * s, 0.75 * s, w, h), 2)                      # inside the first cell
        add(_box((fw - 0.5) * s, (fh - 0.25) * s, w, h), 3)        # inside the last cell
        add(_box(0.25 * s, (fh - 0.75) * s, w, h), 4)              # first column, last row
        add(_box((fw - 0.75) * s, 0.25 * s, w, h), 0)              # last column, first row
        x1 = 1.25 * s - 2 * bw                                     # (negative: then x2 < width and x2 - x1 is exact)
        add([x1, 1.25 * s - bh / 2, x1 + 4 * bw, 1.25 * s + bh / 2], 1)               # width exactly 4.0 x the anchor's
        inside = float(torch.nextafter(torch.tensor(4. * bw, dtype=torch.float32), torch.tensor(0.)))
        add([x1, 1.25 * s - bh / 2, x1 + inside, 1.25 * s + bh / 2], 2)               # one fp32 step inside
        t = torch.tensor(boxes[-2:], dtype=torch.float32)
        assert float(t[0, 2] - t[0, 0]) == 4. * bw and float(t[1, 2] - t[1, 0]) == inside and x1 < 0
        add([1.25 * s, 1.25 * s - bh / 2, 1.25 * s, 1.25 * s + bh / 2], 3)             # zero width: ratio 0, 1 / 0 = inf
        for i in range(8):                                         # the same box eight times, different labels
            add(_box(1.25 * s, 2.25 * s, w, h), i)                 # (left and up neighbours)
        add(_box(1.75 * s, (fh - 1.25) * s, w, h), nl - 1)         # two different boxes sharing an anchor box
        add(_box(1.70 * s, (fh - 1.30) * s, w * 0.9, h * 1.1), 0)  # (right (fw = 3: inv = 1.25 > 1) and down neighbours)
    return boxes, labels


def _assemble(name, N, H, W, strides, base_sizes, C, per_img, first, last, seed, cp=None, agnostic=False, smoother=0.0):
    """per_img: N lists of (box, label); ``first`` leads image 0, ``last`` ends image N - 1; an odd G is forced by one
    extra box in front of ``last``."""
    A = len(base_sizes[0])
    per_img = [list(p) for p in per_img]
    nl = max(C, 1)
    if first is not None:
        per_img[0].insert(0, (first, nl - 1))
    G = sum(len(p) for p in per_img) + (1 if last is not None else 0)
    if G and G % 2 == 0:
        per_img[-1].append((_box(W * 0.3, H * 0.6, base_sizes[0][0][0] * 1.5, base_sizes[0][0][1] * 1.5), 0))
    if last is not None:
        per_img[-1].append((last, 0))
    boxes = [torch.tensor([b for b, _ in p], dtype=torch.float32).reshape(-1, 4) for p in per_img]
    labels = [torch.tensor([int(l) for _, l in p], dtype=torch.long) for p in per_img]
    attr = 5 + (0 if agnostic else C)
    co = A * attr
    case = SimpleNamespace(name=name, N=N, H=H, W=W, strides=list(strides), base_sizes=[list(b) for b in base_sizes],
                           C=0 if agnostic else C, A=A, attr=attr, co=co, Cp=cp or co + (-co) % 8, boxes=boxes, labels=labels,
                           seed=seed, agnostic=agnostic, smoother=smoother, L=len(strides),
                           sizes=[(H // s, W // s) for s in strides], G=sum(b.shape[0] for b in boxes))
    assert case.Cp % 8 == 0 and case.Cp >= co
    for b in boxes:
        if b.numel():
            cx, cy = 0.5 * (b[:, 2] + b[:, 0]), 0.5 * (b[:, 3] + b[:, 1])
            assert bool(((cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)).all()), f'{name}: a box centre is outside the image'
    return case


def _poisson(g, lam):
    return max(1, int(torch.poisson(torch.tensor(float(lam)), generator=g)))


def case_coco():
    N, S_ = 8, 608
    base, strides = O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES
    g = torch.Generator().manual_seed(40)
    per_img = []
    for n in range(N):
        k = _poisson(g, 40)
        b = _random_boxes(g, k, S_, S_)
        lab = torch.randint(0, 80, (k,), generator=g)
        per_img.append([(b[i].tolist(), int(lab[i])) for i in range(k)])
    # random boxes alone give no anchor box more than 2 positives: plant one box five times, different labels, in two
    # images; 72 x 90 matches an anchor of each level ((40, 28), (36, 75), (142, 110))
    plant = _box(301.0, 215.0, 72., 90.)
    for n in (0, 3):
        per_img[n] = [(plant, 60 + 4 * i) for i in range(5)] + per_img[n]
    return _assemble('coco', N, S_, S_, strides, base, 80, per_img, _first_box(base, strides),
                     _last_box(base, strides, S_, S_), seed=41, cp=256)


def _case_nonsquare(name, H, W, seed):
    N = 3
    base, strides = O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES
    g = torch.Generator().manual_seed(seed)
    per_img = []
    for n in range(N):
        k = _poisson(g, 12)
        b = _random_boxes(g, k, H, W)
        lab = torch.randint(0, 80, (k,), generator=g)
        per_img.append([(b[i].tolist(), int(lab[i])) for i in range(k)])
    for l, s in enumerate(strides):                # every quadrant, the last row and the last column of cells, per level
        fh, fw = H // s, W // s
        bw, bh = base[l][1]
        for i, (x, y) in enumerate([(fw * 0.25, fh * 0.25), (fw * 0.75 + 0.25, fh * 0.25 + 0.25), (fw * 0.25, fh * 0.75),
                                    (fw * 0.75, fh * 0.75), (fw - 0.75, fh * 0.5 + 0.3), (fw * 0.5 + 0.3, fh - 0.75),
                                    (fw - 0.25, fh - 0.25)]):
            per_img[(l + i) % N].append((_box(x * s, y * s, bw * 1.2, bh * 0.9), 64 + (5 * l + i) % 16))
        for i in range(2):                         # two boxes of one image on one anchor box
            per_img[l % N].append((_box(2.25 * s, 2.25 * s, bw * (1.2 - 0.2 * i), bh * 0.9), 70 + i))
    return _assemble(name, N, H, W, strides, base, 80, per_img, _first_box(base, strides), _last_box(base, strides, H, W),
                     seed=seed + 1, cp=256)


def case_nonsquare_tall():
    return _case_nonsquare('nonsquare_tall', 608, 416, 50)


def case_nonsquare_wide():
    return _case_nonsquare('nonsquare_wide', 416, 608, 52)


def _spread(units, N, empty_img=1, half_img=2):
    """One image with no box, one holding half of all boxes, the rest over the others.  A unit (a list of boxes that
    must share an image: duplicates, boxes sharing an anchor box) is never split; large units are placed first."""
    per_img = [[] for _ in range(N)]
    others = [n for n in range(N) if n not in (empty_img, half_img)]
    turn = 0
    for u in sorted(units, key=len, reverse=True):
        rest = sum(len(per_img[n]) for n in others)
        if len(per_img[half_img]) <= rest:
            per_img[half_img] += u
        else:
            per_img[others[turn % len(others)]] += u
            turn += 1
    return per_img


def case_edges(name='edges', agnostic=False, extra_random=0, seed=60, cp=None):
    N, H, W, C = 4, 160, 96, 5
    strides = [8, 16, 32]
    eb, el = _edge_boxes(SMALL_BASE, strides, H, W, C)
    items = list(zip(eb, el))
    per = len(items) // len(strides)
    units = []
    for l in range(len(strides)):                  # per level: 10 single boxes, the eight duplicates, the sharing pair
        lv = items[l * per:(l + 1) * per]
        units += [[it] for it in lv[:10]] + [lv[10:18], lv[18:20]]
    if extra_random:
        g = torch.Generator().manual_seed(seed)
        b = _random_boxes(g, extra_random, H, W, lo=6.0, hi=120.0)
        lab = torch.randint(0, C, (extra_random,), generator=g)
        units += [[(b[i].tolist(), int(lab[i]))] for i in range(extra_random)]
    first = _box(40.0, 40.0, 55., 75.)             # matches (30, 60) and (100, 90)
    last = _box(51.0, 2 * 16 + 13.0, 42., 45.)     # matches (30, 20) and (58, 100); down neighbour at strides 8 and 16
    per_img = _spread(units, N)
    for i in range(4):                             # keeps one image at half of all boxes once first / last / odd-G are in
        per_img[2].append((_box(30. + 7 * i, 100. - 9 * i, 20. + i, 24. - i), i % C))
    case = _assemble(name, N, H, W, strides, SMALL_BASE, C, per_img, first, last, seed=seed + 1, cp=cp, agnostic=agnostic)
    counts = [b.shape[0] for b in case.boxes]
    assert counts[1] == 0 and 2 * counts[2] >= case.G, counts
    lab = torch.cat(case.labels)
    assert int(lab.min()) == 0 and int(lab.max()) == C - 1
    return case


def case_agnostic():
    return case_edges('agnostic', agnostic=True, extra_random=24, seed=70, cp=16)


def case_wide_a():
    """A = 4 with custom base sizes on two levels."""
    N, H, W, C = 2, 128, 160, 6
    strides = [8, 16]
    base = [[(8, 10), (14, 26), (28, 18), (20, 20)], [(30, 56), (56, 40), (50, 90), (44, 44)]]
    g = torch.Generator().manual_seed(80)
    per_img = []
    for n in range(N):
        b = _random_boxes(g, 14, H, W, lo=6.0, hi=150.0)
        lab = torch.randint(0, C, (14,), generator=g)
        per_img.append([(b[i].tolist(), int(lab[i])) for i in range(14)])
    for l, s in enumerate(strides):
        bw, bh = base[l][3]
        for i, (x, y) in enumerate([(2.25, 2.25), (2.25, 2.25), (3.75, 3.75), (W // s - 1.25, H // s - 1.25)]):
            per_img[i % N].append((_box(x * s, y * s, bw * 1.1, bh * 0.9), (l + i) % C))
    first = _box(40.0, 40.0, 34., 60.)                       # matches (30, 56): anchor 0 of level 1
    last = _box(83.0, 2 * 8 + 6.5, 22., 22.)                 # matches (20, 20): anchor 3 of level 0, down neighbour
    return _assemble('wide_a', N, H, W, strides, base, C, per_img, first, last, seed=81, cp=48, smoother=0.1)


def case_empty():
    base, strides = O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES
    return _assemble('empty', 8, 608, 608, strides, base, 80, [[] for _ in range(8)], None, None, seed=90, cp=256)


CASES = dict(coco=case_coco, nonsquare_tall=case_nonsquare_tall, nonsquare_wide=case_nonsquare_wide, edges=case_edges,
             agnostic=case_agnostic, wide_a=case_wide_a, empty=case_empty)
_case_cache = {}


def get_case(name):
    if name not in _case_cache:
        case = CASES[name]()
        case.assign = assignment(case)
        check_coverage(case)
        _case_cache[name] = case
    return _case_cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's assignment, with the candidate-slot number of every positive
# ---------------------------------------------------------------------------------------------------------------------
def assignment(case):
    """``responsible_indices`` on the fp32 boxes -> per level a namespace of (img, anchor, g, k, a, slot), in the
    oracle's list order.  The neighbour kind k is recovered from geometry alone (the positive's cell against the cell of
    the same (anchor, box) pair's k = 0 entry), and ``slot = (k * A + a) * G + g``.  That the slot numbers come out
    STRICTLY INCREASING in list order is asserted here: it is what makes the reference's "last write wins" the largest
    slot number."""
    resp = O.responsible_indices(case.sizes, case.boxes, 2, 4., case.base_sizes, case.strides)
    A, G = case.A, case.G
    out = []
    for l, (img, anchor, g) in enumerate(resp):
        fh, fw = case.sizes[l]
        a = anchor % A
        cell = torch.div(anchor, A, rounding_mode='floor')
        own = {}
        for i in range(anchor.numel()):
            own.setdefault((int(a[i]), int(g[i])), int(cell[i]))      # the k = 0 row comes first and always exists
        k = torch.empty_like(anchor)
        kind = {0: 0, -1: 1, -fw: 2, 1: 3, fw: 4}
        for i in range(anchor.numel()):
            k[i] = kind[int(cell[i]) - own[(int(a[i]), int(g[i]))]]
        slot = (k * A + a) * G + g
        if slot.numel() > 1:
            assert bool((slot[1:] > slot[:-1]).all()), f'{case.name} level {l}: list order is not slot order'
        assert bool(((anchor >= 0) & (anchor < fh * fw * A)).all())
        out.append(SimpleNamespace(img=img, anchor=anchor, g=g, k=k, a=a, slot=slot))
    return out


def expected_winner(case):
    """(N, TA) int64: per anchor box the largest slot number among its positives, -1 where it has none."""
    TA = sum(h * w * case.A for h, w in case.sizes)
    win = torch.full((case.N, TA), -1, dtype=torch.long)
    off = 0
    for l, asg in enumerate(case.assign):
        if asg.slot.numel():
            flat = win.view(-1)
            flat.scatter_reduce_(0, asg.img * TA + off + asg.anchor, asg.slot, reduce='amax', include_self=True)
        off += case.sizes[l][0] * case.sizes[l][1] * case.A
    return win


def positives_per_box(case, l):
    """(N, H*W*A) int64 count of positives per anchor box of level l."""
    fh, fw = case.sizes[l]
    cnt = torch.zeros(case.N * fh * fw * case.A, dtype=torch.long)
    asg = case.assign[l]
    if asg.slot.numel():
        cnt.index_add_(0, asg.img * (fh * fw * case.A) + asg.anchor, torch.ones_like(asg.anchor))
    return cnt.view(case.N, fh * fw * case.A)


def check_coverage(case):
    """Conditions, from the oracle's assignment alone, that the case contains what it was built for."""
    name, L, A, G = case.name, case.L, case.A, case.G
    S = 5 * A * G
    if name in ('coco', 'empty'):
        fh, fw = case.sizes[0]
        for ch in (4, 8):
            assert case.N * fh * fw * (case.Cp // ch) > DENSE_BWD_TRIP, f'{name}: the dense backward makes one trip only'
    if name == 'empty':
        assert G == 0
        return
    assert G % 2 == 1 and S % 8 != 0, f'{name}: S = {S} is a multiple of 8'
    for l, asg in enumerate(case.assign):
        for k in range(5):
            assert int((asg.k == k).sum()) >= 1, f'{name} level {l}: no positive of neighbour kind {k}'
        most = int(positives_per_box(case, l).max())
        assert most >= 2, f'{name} level {l}: no anchor box with two positives'
        if name in ('edges', 'coco', 'agnostic'):
            assert most >= 4, f'{name} level {l}: no anchor box with four positives'
    for l in range(1, L):       # an aligned run of 8 slot numbers that crosses the level border, valid slots on both sides
        border = l * S
        lo = border - border % 8
        assert lo < border, f'{name}: border {l} is aligned to 8'
        before = case.assign[l - 1].slot + (l - 1) * S
        after = case.assign[l].slot + l * S
        assert bool(((before >= lo) & (before < border)).any()) and bool(((after >= border) & (after < lo + 8)).any()), \
            f'{name}: no wave of 8 slots straddles the border of levels {l - 1} / {l} with positives on both sides'
    if name in ('coco', 'nonsquare_tall', 'nonsquare_wide'):
        lab = torch.cat(case.labels)
        assert case.C > 64
        assert any(bool((lab[asg.g] >= 64).any()) for asg in case.assign), f'{name}: no positive with a label >= 64'
    if name.startswith('nonsquare'):
        assert case.H != case.W
        for l, asg in enumerate(case.assign):
            fh, fw = case.sizes[l]
            cell = torch.div(asg.anchor, A, rounding_mode='floor')
            x, y = cell % fw, torch.div(cell, fw, rounding_mode='floor')
            for qx in (0, 1):
                for qy in (0, 1):
                    assert bool((((x >= fw // 2) == bool(qx)) & ((y >= fh // 2) == bool(qy))).any()), \
                        f'{name} level {l}: no positive in quadrant ({qx}, {qy})'
            assert bool((x == fw - 1).any()) and bool((y == fh - 1).any()), f'{name} level {l}: last row / column unused'
    if name in ('edges', 'agnostic'):
        _check_edges(case)


def _check_edges(case):
    """The hand-built boxes do what they were built for (the layout of ``_edge_boxes``: 20 boxes per level)."""
    allb = torch.cat(case.boxes)
    eb, _ = _edge_boxes(case.base_sizes, case.strides, case.H, case.W, 5)
    per = len(eb) // case.L

    def gid(i):
        hit = (allb == torch.tensor(eb[i], dtype=torch.float32)).all(1).nonzero().reshape(-1)
        assert hit.numel() >= 1
        return int(hit[0])

    for l, asg in enumerate(case.assign):
        def kinds(i, a=1):
            g = gid(l * per + i)
            return sorted(int(v) for v in asg.k[(asg.g == g) & (asg.a == a)])
        fw = case.sizes[l][1]
        # x = 2.0: (x % 1 = 0) left, and right while W - x > 1 (not on the 3-cell-wide level); y = 1.0: `> 1` fails, down
        assert kinds(0) == ([0, 1, 3, 4] if fw - 2.0 > 1 else [0, 1, 4]), (l, kinds(0))
        assert kinds(1) == [0, 2, 3, 4], (l, kinds(1))      # x = 1.0: rem 0 < 0.5 but not > 1: no left; y = 2.0: up, down
        assert kinds(2) == [0], (l, kinds(2))               # x = 1.5, y = 2.5: 0.5 is not < 0.5, either way round
        assert kinds(3) == [0, 4], (l, kinds(3))            # first cell: only (H - y) % 1 = 0.25 -> down
        assert kinds(4) == [0], (l, kinds(4))               # last cell: (H - y) % 1 = 0.25 but H - y <= 1
        assert kinds(5) == [0, 2], (l, kinds(5))            # first column (x <= 1), last row
        assert kinds(6) == [0, 1], (l, kinds(6))            # last column, first row (y <= 1)
        assert kinds(7) == [], (l, kinds(7))                # width exactly 4.0 x: not < 4
        assert kinds(8) == [0, 1, 2], (l, kinds(8))         # one fp32 step inside
        assert int((asg.g == gid(l * per + 9)).sum()) == 0  # zero width: no anchor at all
        assert kinds(10) == [0, 1, 2], (l, kinds(10))
        assert kinds(18) == [0, 3, 4] and kinds(19) == [0, 3, 4], (l, kinds(18), kinds(19))
        assert int(positives_per_box(case, l).max()) >= 8


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the reference
# ---------------------------------------------------------------------------------------------------------------------
def make_inputs(case, dtype=torch.float32):
    """Per level (raw (N, H, W, Cp) in ``dtype`` -- NHWC, padding channels filled like the rest --, bias (co,) fp32):
    randn * 1.5 and randn * 0.5 as the toy tests draw them."""
    g = torch.Generator().manual_seed(case.seed)
    out = []
    for (fh, fw) in case.sizes:
        raw = (torch.randn(case.N, fh, fw, case.Cp, generator=g) * 1.5).to(dtype)
        bias = torch.randn(case.co, generator=g) * 0.5
        out.append((raw, bias))
    return out


def dense_maps(case, inputs):
    """What the kernels read: fp32(raw) + bias, one fp32 rounding, as NCHW (N, co, H, W) fp32."""
    return [(raw[..., :case.co].float() + bias).permute(0, 3, 1, 2).contiguous() for raw, bias in inputs]


def reference(case, inputs, dtype):
    """``head_loss`` in ``dtype`` on the fp32 inputs, differentiated by autograd under the WEIGHTS upstream gradients.
    Returns losses (L, 3) [cls | conf before the level balance | bbox], per level conf_t of every positive in list
    order, draw (N, H, W, co) and dbias (co,), all in ``dtype``."""
    leaves = [d.to(dtype).requires_grad_(True) for d in dense_maps(case, inputs)]
    out = O.head_loss(leaves, case.boxes, case.labels, num_classes=case.C, base_sizes=case.base_sizes,
                      strides=case.strides, one_hot_smoother=case.smoother,
                      conf_level_balance_weight=(1.0,) * case.L, dtype=dtype)
    losses = torch.stack([torch.stack([out[k][l].reshape(()) for k in ('loss_cls', 'loss_conf', 'loss_bbox')])
                          for l in range(case.L)])
    assert losses.dtype == dtype
    (losses * gout_matrix(case.L).to(dtype)).sum().backward()
    anchors = O.grid_anchors(case.sizes, case.base_sizes, case.strides)
    gtb = torch.cat(case.boxes).to(dtype)
    conf_t = []
    with torch.no_grad():
        for l, asg in enumerate(case.assign):
            if not asg.slot.numel():
                conf_t.append(torch.zeros(0, dtype=dtype))
                continue
            pm = leaves[l].detach().permute(0, 2, 3, 1).reshape(case.N, -1, case.attr)
            pb = pm[asg.img, asg.anchor][:, :4].sigmoid()
            box = O.bbox_decode(anchors[l][asg.anchor].to(dtype), torch.cat((pb[:, :2] * 2. - 1., (pb[:, 2:] * 2.) ** 2.), -1),
                                case.strides[l])
            giou_l = 1 - O.bbox_overlaps_giou_aligned(box, gtb[asg.g], eps=1e-6)
            conf_t.append((1 - giou_l).clamp(0.0, 1.0))
    draw = [x.grad.permute(0, 2, 3, 1).contiguous() for x in leaves]
    dbias = [x.grad.sum((0, 2, 3)) for x in leaves]
    return SimpleNamespace(losses=losses.detach(), conf_t=conf_t, draw=draw, dbias=dbias)


def loss_errors(x, ref):
    """Relative error of each of the (L, 3) loss values."""
    x, ref = x.double(), ref.double()
    e = torch.zeros_like(ref)
    for idx in range(ref.numel()):
        e.view(-1)[idx] = err(x.view(-1)[idx], ref.view(-1)[idx])
    return e


_ref_cache = {}


def references(name, dtype=torch.float32):
    """(case, inputs, ref64, e32) for a case and map dtype, computed once per process.  ``e32`` holds the reference's own
    fp32 error in the measure above: losses (L, 3), and per level conf_t / draw / dbias."""
    key = (name, dtype)
    if key not in _ref_cache:
        case = get_case(name)
        inputs = make_inputs(case, dtype)
        r64 = reference(case, inputs, torch.float64)
        r32 = reference(case, inputs, torch.float32)
        e32 = SimpleNamespace(losses=loss_errors(r32.losses, r64.losses),
                              conf_t=[err(a, b) for a, b in zip(r32.conf_t, r64.conf_t)],
                              draw=[err(a, b) for a, b in zip(r32.draw, r64.draw)],
                              dbias=[err(a, b) for a, b in zip(r32.dbias, r64.dbias)])
        _ref_cache[key] = (case, inputs, r64, e32)
    return _ref_cache[key]


def describe(tag, e, e32):
    return f'{tag}: e = {e:.3e}  e32 = {e32:.3e}  bound = {bound(e32):.3e}  ratio e/e32 = {e / e32 if e32 else float("inf"):.2f}'
