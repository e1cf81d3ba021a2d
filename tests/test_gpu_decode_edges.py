"""yv4_decode_filter and yv4_decode_filter_v3 (csrc/postproc.hip) through the C ABI at the kernel's edges, against
tests/_post_ref.py: the candidate keys, counts and max_coord exactly (from the kernel's own conf / cls / boxes, whose
products and maxima numpy float32 reproduces bit for bit), boxes / conf / cls against the float64 decode.

Levels of 7x5, 13x11 and 4x4 cells with A = 3 and N = 3: 105, 429 and 48 boxes, ten 64-box tiles per image with tails
of 41, 45 and 48 boxes, five two-tile workgroups.  105 and 429 are odd, so images 1 and 2 of those levels start off a
16-byte boundary (the scalar load) for every class count but 3, and the tails have nval % 4 != 0."""
import numpy as np
import pytest
import torch

import _post_ref as R
import mmdet_yolov4_amd as pkg
from oracle import yolov3_oracle as V3
from oracle import yolov4_oracle as O

pytestmark = pytest.mark.gpu

HW = [(7, 5), (13, 11), (4, 4)]
A, N = 3, 3
STRIDES = [8, 16, 32]
SIZES = [h * w * A for h, w in HW]
TOTAL = sum(SIZES)
BASE_SIZES = {False: O.DEFAULT_BASE_SIZES, True: V3.V3_BASE_SIZES[::-1]}      # per head, for strides 8, 16, 32
SF = np.float32([[1.0, 1.0, 1.0, 1.0], [0.8125, 0.75, 0.8125, 0.75], [1.7, 1.3, 1.6, 1.2]])
CANARY64 = 0x5A5A5A5A5A5A5A5A
CANARY_F = -7.0                          # no sigmoid is negative
PAD = 64
TILE = 64

# candidates of a workgroup's two tiles -> the route its keys take (the workgroup buffers up to kDecKeyBuf = 1024 in LDS)
EARLY_FLUSH, AT_CAPACITY, DIRECT_PENDING = (600, 600), (1024, 0), (1025, 10)
BUFFER_THEN_DIRECT, BOTH_DIRECT, EMPTY = (10, 1025), (5120, 5120), (0, 0)
# per image, the five workgroups (tiles of 64+41 | 64+64 | 64+64 | 64+64 | 45+48 boxes; 5120 needs two full tiles)
WG_PLAN = [[EARLY_FLUSH, BOTH_DIRECT, AT_CAPACITY, DIRECT_PENDING, BUFFER_THEN_DIRECT],
           [DIRECT_PENDING, EMPTY, BOTH_DIRECT, EARLY_FLUSH, AT_CAPACITY],
           [BUFFER_THEN_DIRECT, EARLY_FLUSH, EMPTY, BOTH_DIRECT, DIRECT_PENDING]]


def tiles():
    """(level, first box in the level, boxes) of an image's tiles, in workgroup order."""
    out = []
    for l, n_l in enumerate(SIZES):
        out += [(l, b0, min(TILE, n_l - b0)) for b0 in range(0, n_l, TILE)]
    return out


def constructed_preds(rng, Cn):
    """Objectness +9 everywhere, class logits -9 except +9 on the planned number of (box, class) cells per tile, in
    random places: no product is anywhere near a threshold.  Box logits random in [-2, 2]."""
    attr = 5 + Cn
    preds = [np.full((N, n_l, attr), -9.0, np.float32) for n_l in SIZES]
    for p in preds:
        p[..., :4] = rng.uniform(-2, 2, p[..., :4].shape)
        p[..., 4] = 9.0
    t = tiles()
    assert len(t) == 10 and [nb for _, _, nb in t] == [64, 41, 64, 64, 64, 64, 64, 64, 45, 48]
    for n in range(N):
        for i, (l, b0, nb) in enumerate(t):
            count = WG_PLAN[n][i // 2][i % 2]
            assert count <= nb * Cn
            cells = rng.choice(nb * Cn, count, replace=False)
            preds[l][n, b0 + cells // Cn, 5 + cells % Cn] = 9.0
    return [p.reshape(N, h, w, A * attr) for p, (h, w) in zip(preds, HW)]


def random_preds(rng, Cn, grid=None):
    """Objectness and class logits normal * 2 (objectness on a grid of `grid` when given: exact ties), box logits
    uniform in [-2, 2]."""
    attr = 5 + Cn
    preds = []
    for (h, w), n_l in zip(HW, SIZES):
        p = (rng.standard_normal((N, n_l, attr)) * 2).astype(np.float32)
        p[..., :4] = rng.uniform(-2, 2, p[..., :4].shape)
        if grid:
            p[..., 4] = np.round(p[..., 4] / grid) * grid
        preds.append(p.reshape(N, h, w, A * attr))
    return preds


def oracle_fp32(preds, Cn, v3):
    """The fp32 CPU oracle's decode of the same maps (boxes before the division by scale_factor)."""
    nchw = [torch.from_numpy(np.ascontiguousarray(p.transpose(0, 3, 1, 2))) for p in preds]
    if v3:
        return torch.cat([b for b, _, _ in V3.decode_maps_v3(nchw, Cn, BASE_SIZES[True], STRIDES)], 1).numpy()
    return O.decode_maps(nchw, Cn, BASE_SIZES[False], STRIDES, class_agnostic=Cn == 0)[0].numpy()


def box_error(got, want, v3):
    """The project's measures: absolute for the CSP head, |d| / (1 + |want|) for YOLOv3's (its exp() is unbounded)."""
    d = np.abs(got.astype(np.float64) - want)
    return (d / (1 + np.abs(want))).max() if v3 else d.max()


def to_dev(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev)


def run_decode(dev, preds, Cn, v3, score_thr, key_cap, conf_thr=-1.0, sf=None, topk=None):
    lib = pkg._lib.lib()
    base = R.base_anchors(BASE_SIZES[v3], STRIDES)
    d_preds = [to_dev(p, dev) for p in preds]
    levels = (pkg._lib.LevelDesc * 3)()
    for i, p in enumerate(d_preds):
        levels[i].pred = p.data_ptr()
        levels[i].H, levels[i].W, levels[i].stride = HW[i][0], HW[i][1], STRIDES[i]
        for a in range(A):
            for c in range(4):
                levels[i].base_anchors[a][c] = float(base[i][a, c])
    boxes = torch.full((N * TOTAL * 4 + 2 * PAD,), float('nan'), dtype=torch.float32, device=dev)
    conf = torch.full((N * TOTAL + 2 * PAD,), float('nan'), dtype=torch.float32, device=dev)
    cls = torch.full((N * TOTAL * Cn + 2 * PAD,), CANARY_F, dtype=torch.float32, device=dev) if Cn else None
    keys = torch.from_numpy(np.full(N * key_cap + PAD, CANARY64, np.uint64).view(np.int64)).to(dev)
    counts = torch.full((N,), 77, dtype=torch.int32, device=dev)
    mx = torch.full((N,), 3.0, dtype=torch.float32, device=dev)
    d_sf = to_dev(sf, dev) if sf is not None else None
    d_topk = to_dev(topk, dev) if topk is not None else None
    common = (boxes.data_ptr() + PAD * 4, conf.data_ptr() + PAD * 4, cls.data_ptr() + PAD * 4 if Cn else None,
              keys.data_ptr(), key_cap, counts.data_ptr(), mx.data_ptr(), d_topk.data_ptr() if topk is not None else None,
              None)
    sfp = d_sf.data_ptr() if sf is not None else None
    torch.cuda.synchronize()
    pkg._lib.check(lib.yv4_decode_reset(counts.data_ptr(), mx.data_ptr(), N, None), 'yv4_decode_reset')
    if v3:
        rc = lib.yv4_decode_filter_v3(levels, 3, N, A, Cn, score_thr, conf_thr, sfp, *common)
    else:
        rc = lib.yv4_decode_filter(levels, 3, N, A, Cn, score_thr, sfp, *common)
    pkg._lib.check(rc, 'yv4_decode_filter')
    torch.cuda.synchronize()
    out = {}
    for name, t, per in (('boxes', boxes, 4), ('conf', conf, 1)) + ((('cls', cls, Cn),) if Cn else ()):
        a = t.cpu().numpy()
        n = N * TOTAL * per
        edge = np.concatenate([a[:PAD], a[PAD + n:]])
        assert (np.isnan(edge) if name != 'cls' else edge == CANARY_F).all(), f'{name} written out of bounds'
        out[name] = a[PAD:PAD + n].reshape((N, TOTAL, per) if per > 1 or name == 'cls' else (N, TOTAL))
    k = keys.cpu().numpy().view(np.uint64)
    assert (k[N * key_cap:] == CANARY64).all(), 'words after the key buffers were written'
    out.update(keys=k[:N * key_cap].reshape(N, key_cap), counts=counts.cpu().numpy(), max_coord=mx.cpu().numpy())
    return out


def check_decode(out, preds, Cn, v3, score_thr, tag, conf_thr=-1.0, sf=None, topk=None, overflow=()):
    """Everything one launch returns.  Returns the expected keys per image.

    Boxes: 1e-4 in the head's measure, which YOLOv3's relative measure keeps on every input here (the fp32 CPU oracle
    is within 4.1e-6 .. 1.1e-5 of the float64 decode).  The CSP head's is absolute, and with box logits up to +-2 the
    boxes reach |x| = 990, where one fp32 ulp is 6.1e-5: the fp32 CPU oracle itself is 0.89e-4 .. 1.75e-4 off the
    float64 decode on these inputs (1.04e-4 / 1.02e-4 on the constructed maps with 80 / 100 classes; 1.60e-4, 1.48e-4,
    1.07e-4, 1.39e-4, 1.75e-4 on the random maps with 0, 1, 3, 80, 100 classes; 1.45e-4, 1.36e-4, 0.89e-4 on the
    nms_pre maps with 0, 3, 100 classes, all with scale factors).  So the bound is four times the oracle's own error
    on the same input, measured here, where that exceeds 1e-4: room for another order of the same operations."""
    base = R.base_anchors(BASE_SIZES[v3], STRIDES)
    rb, rc, rs = R.decode_ref(preds, A, Cn, STRIDES, base, v3, scale_factor=sf)
    ob = oracle_fp32(preds, Cn, v3)
    oracle_err = box_error(ob / sf[:, None, :] if sf is not None else ob, rb, v3)
    box_tol = max(1e-4, 4 * oracle_err)
    err = box_error(out['boxes'], rb, v3)
    print(f'{tag}: box error {err:.3g} (fp32 oracle {oracle_err:.3g}, bound {box_tol:.3g}), conf error {np.abs(out["conf"] - rc).max():.3g}')
    assert err <= box_tol, f'{tag}: boxes off by {err}'
    assert np.abs(out['conf'] - rc).max() <= 1e-6, tag
    cls = out.get('cls')
    want, admitted = R.candidates_from(out['conf'], cls, score_thr, v3, level_sizes=SIZES, topk_keys=topk,
                                       conf_thr=conf_thr)
    if Cn:
        # class scores of the admitted boxes; the rows of boxes turned away by nms_pre / conf_thr are left unwritten
        assert np.abs(cls[admitted] - rs[admitted]).max() <= 1e-6, tag
        assert (cls[~admitted] == CANARY_F).all(), f'{tag}: class scores of a box that was not admitted were written'
    cap = out['keys'].shape[1]
    for n in range(N):
        cnt = want[n].size
        assert out['counts'][n] == cnt, f'{tag}: counts[{n}] = {out["counts"][n]}, want {cnt}'
        if n not in overflow:
            msg = R.diff_keys(out['keys'][n, :cnt], want[n], Cn, SIZES, names=('level', 'box'), image=n)
            assert msg is None, f'{tag}: {msg}'
            assert (out['keys'][n, cnt:cap] == CANARY64).all(), f'{tag}: image {n}: keys past counts[n] were written'
        # boxes.max() over the boxes that have a candidate, of the kernel's own boxes
        j = np.unique(R.key_flat(want[n]) // max(Cn, 1))
        mc = out['boxes'][n, j].max() if j.size else np.float32(-np.inf)
        msg = R.diff_bits(out['max_coord'][n:n + 1], np.float32([mc]), f'max_coord (image {n})')
        assert msg is None, f'{tag}: {msg}'
    return want


@pytest.mark.parametrize('v3', [False, True], ids=['csp', 'v3'])
@pytest.mark.parametrize('Cn', [80, 100])
def test_decode_key_routes_constructed(gpu_device, Cn, v3):
    """Per workgroup the planned number of candidates per tile: buffered, buffered at capacity, flushed early, written
    directly with a buffer pending, both tiles direct, none.  key_cap exact, then one short: counts keeps counting,
    key_cap distinct keys of the expected set are written, the next image's keys are intact."""
    rng = np.random.default_rng([1, Cn, v3])
    preds = constructed_preds(rng, Cn)
    planned = [sum(a + b for a, b in WG_PLAN[n]) for n in range(N)]
    assert planned == [14534, 13499, 13510]
    kw = dict(conf_thr=0.5) if v3 else {}                             # conf = sigmoid(9): everything stays
    out = run_decode(gpu_device, preds, Cn, v3, 0.5, planned[0], sf=SF, **kw)
    want = check_decode(out, preds, Cn, v3, 0.5, f'constructed C={Cn} v3={v3}', sf=SF, **kw)
    assert [k.size for k in want] == planned
    # the plan itself, per tile: the candidates of every tile are the planned number
    for n in range(N):
        box = R.key_flat(want[n]) // Cn
        for i, (l, b0, nb) in enumerate(tiles()):
            first = sum(SIZES[:l]) + b0
            assert ((box >= first) & (box < first + nb)).sum() == WG_PLAN[n][i // 2][i % 2]
    cap = planned[0] - 1
    out = run_decode(gpu_device, preds, Cn, v3, 0.5, cap, sf=SF, **kw)
    check_decode(out, preds, Cn, v3, 0.5, f'constructed C={Cn} v3={v3} overflow', sf=SF, overflow=(0,), **kw)
    written = out['keys'][0]
    assert np.unique(written).size == cap
    assert np.isin(written, want[0]).all()


RANDOM_CASES = [(Cn, v3) for Cn in (0, 1, 3, 80, 100) for v3 in (False, True) if Cn or not v3]


@pytest.mark.parametrize('Cn,v3', RANDOM_CASES, ids=[f'C{c}-{"v3" if v else "csp"}' for c, v in RANDOM_CASES])
def test_decode_random_logits_and_planted_thresholds(gpu_device, Cn, v3):
    """Random logits: the candidate keys are exactly those of the kernel's own conf / cls.  Then the thresholds are set
    to values the kernel itself produced: a candidate whose score (CSP: cls * conf, v3: cls) EQUALS score_thr is
    excluded (`>`), a box whose objectness EQUALS conf_thr stays (`>=`)."""
    rng = np.random.default_rng([2, Cn, v3])
    preds = random_preds(rng, Cn)
    cap = TOTAL * max(Cn, 1)
    tag = f'random C={Cn} v3={v3}'
    out = run_decode(gpu_device, preds, Cn, v3, 0.3, cap, sf=SF)
    want = check_decode(out, preds, Cn, v3, 0.3, tag, sf=SF)
    assert all(0 < k.size < cap for k in want)
    # plant: the median observed value of image 1 becomes the threshold
    conf, cls = out['conf'], out.get('cls')
    if Cn == 0:
        tested = conf[1]
    else:
        tested = (cls[1] if v3 else cls[1] * conf[1][:, None]).reshape(-1)
    assert tested.dtype == np.float32
    thr = float(np.sort(tested)[tested.size // 2])
    at = np.nonzero(tested == np.float32(thr))[0]
    assert at.size >= 1
    kw = {}
    if v3:
        cthr = float(np.sort(conf[1])[TOTAL // 3])
        kw = dict(conf_thr=cthr)
        box_at = np.nonzero(conf[1] == np.float32(cthr))[0]
        assert box_at.size >= 1 and cthr > 0
    out2 = run_decode(gpu_device, preds, Cn, v3, thr, cap, **kw)
    want2 = check_decode(out2, preds, Cn, v3, thr, tag + ' planted', **kw)
    got_flat = R.key_flat(out2['keys'][1, :out2['counts'][1]])
    assert not np.isin(at, got_flat).any(), f'{tag}: a score equal to score_thr passed'
    above = np.nonzero(tested > np.float32(thr))[0]
    if v3:
        above = above[conf[1][above // Cn] >= np.float32(cthr)]
        # a box at conf_thr keeps its class scores (written: it was admitted) and its candidates
        assert (out2['cls'][1, box_at] != CANARY_F).all(), f'{tag}: a box with conf == conf_thr was dropped'
        below = np.nonzero(conf[1] < np.float32(cthr))[0]
        assert below.size and (out2['cls'][1, below] == CANARY_F).all()
    np.testing.assert_array_equal(np.sort(got_flat), above)
    assert want2[1].size == above.size


NMS_PRE_CASES = [(0, False), (3, False), (100, False), (1, True), (80, True)]


@pytest.mark.parametrize('Cn,v3', NMS_PRE_CASES, ids=[f'C{c}-{"v3" if v else "csp"}' for c, v in NMS_PRE_CASES])
def test_decode_nms_pre_with_ties_across_the_cut(gpu_device, Cn, v3):
    """nms_pre per image (CSP head) and per level (YOLOv3): objectness logits on a grid of 1 / 2 give exact ties, and
    every cut is placed between two equal values of the kernel's own conf, so admission rests on the anchor index."""
    rng = np.random.default_rng([3, Cn, v3])
    preds = random_preds(rng, Cn, grid=0.5)
    cap = TOTAL * max(Cn, 1)
    tag = f'nms_pre C={Cn} v3={v3}'
    out = run_decode(gpu_device, preds, Cn, v3, 0.2, cap)
    check_decode(out, preds, Cn, v3, 0.2, tag + ' uncut')
    conf = out['conf']
    segs = SIZES if v3 else [TOTAL]
    topk = np.empty((N, len(segs)), np.uint64)
    for n in range(N):
        ab = 0
        for l, n_l in enumerate(segs):
            idx = np.arange(ab, ab + n_l)
            order = idx[np.lexsort((idx, -conf[n, idx].astype(np.float64)))]
            s = conf[n, order]
            k = next(k for k in range(n_l // 3, n_l) if s[k - 1] == s[k])           # the k-th and (k+1)-th are equal
            topk[n, l] = R.conf_key(conf[n, order[k - 1]], order[k - 1])[0]
            assert topk[n, l] == np.sort(R.conf_key(conf[n, idx], idx))[k - 1]
            ab += n_l
    kw = dict(conf_thr=0.25) if v3 else {}
    out2 = run_decode(gpu_device, preds, Cn, v3, 0.2, cap, sf=SF, topk=topk if v3 else topk[:, 0], **kw)
    want = check_decode(out2, preds, Cn, v3, 0.2, tag, sf=SF, topk=topk, **kw)
    assert all(0 < k.size for k in want)
    np.testing.assert_array_equal(out2['conf'], conf)                               # every box is still decoded
