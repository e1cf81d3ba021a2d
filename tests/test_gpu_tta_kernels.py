"""yv4_topk_slots and yv4_tta_merge (csrc/tta.hip) through the C ABI on constructed inputs, every comparison exact,
against tests/_post_ref.py (pinned on the CPU by tests/test_post_ref_host.py).

The TTA fixture has levels of 36 / 144 / 576 boxes, nms_pre = 40 and 6 classes: the bitonic sort never has more keys
than threads, the radix path (a top-k beyond 8192) never runs, a merge thread's class loop takes two trips.  Here the
slot tables are built at the sizes where the kernel changes path, on objectness with ties (the order then rests on the
anchor index alone), and the merge on up to 16 augmentations, 81 classes, workgroups that straddle three augmentations,
a key buffer that overflows and a max_coord that ends negative."""
import ctypes as C

import numpy as np
import pytest
import torch

import _post_ref as R
import mmdet_yolov4_amd as pkg

pytestmark = pytest.mark.gpu

CANARY32 = 0x5A5A5A5A
CANARY64 = 0x5A5A5A5A5A5A5A5A
PAD = 64


def to_dev(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev)


def check(rc, what):
    pkg._lib.check(rc, what)


# ---------------------------------------------------------------------------------------------------------------------
# slot tables
# ---------------------------------------------------------------------------------------------------------------------
def run_slots(dev, conf, sizes, nms_pre, keys):
    """yv4_topk_slots on conf (N, total); keys (N, L) uint64 or None.  The slot buffer is filled with a canary and
    has canary words before and after it."""
    lib = pkg._lib.lib()
    N, total = conf.shape
    L = len(sizes)
    sizes_c = (C.c_int32 * L)(*sizes)
    ks = R.slot_sizes(sizes, nms_pre)
    S = sum(ks)
    radix = [n for n, k in zip(sizes, ks) if k < n and k > 8192]
    ws = lib.yv4_topk_slots_work(L, sizes_c, nms_pre)
    assert (ws > 0) == bool(radix)
    if radix:                           # three key buffers and the histogram of the LARGEST radix level
        n = max(radix)
        assert ws >= 3 * 8 * n + 256 * ((n + 1023) // 1024) * 4
    work = torch.empty(ws, dtype=torch.uint8, device=dev) if ws else None
    buf = torch.full((N * S + 2 * PAD,), CANARY32, dtype=torch.int32, device=dev)
    d_conf = to_dev(conf, dev)
    d_keys = to_dev(keys, dev) if keys is not None else None
    torch.cuda.synchronize()
    check(lib.yv4_topk_slots(d_conf.data_ptr(), N, total, L, sizes_c, nms_pre,
                             d_keys.data_ptr() if d_keys is not None else None,
                             work.data_ptr() if work is not None else None, buf.data_ptr() + PAD * 4, S, None),
          'yv4_topk_slots')
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:PAD] == CANARY32).all(), 'words before the slot table were written'
    assert (out[PAD + N * S:] == CANARY32).all(), 'words after the slot table were written'
    return out[PAD:PAD + N * S].reshape(N, S)


# layout -> (level sizes, nms_pre values)
LAYOUTS = {
    'a': ((300, 1200, 4800), (1025,)),                 # P = 2048 keys on 1024 threads: two trips of every loop
    'b': ((1083, 4332, 17328), (1000, 3000)),          # the 608-pixel level sizes
    'c': ((9000, 20000), (8192,)),                     # the LDS sort at capacity
    'd': ((9000, 20000), (8193,)),                     # both levels radix, one work buffer sized by the larger
    'e': ((100, 20000), (10000,)),                     # an uncut level and a radix level
    'f': ((8194, 64), (8193,)),                        # the smallest radix level, a ragged sort tile
    'g': ((64, 5), (1,)),                              # k = 1
    'h': ((500, 500), (499, 500, -1)),                 # n_l - 1; uncut; uncut with topk_keys = NULL
    'i': ((1, 2, 63, 64, 65, 1023, 1025, 2049), (64,)),  # kMaxSlotLevels levels, cut and uncut, k = n_l - 1 again
}
SLOT_CASES = [(name, pre) for name, (_, pres) in LAYOUTS.items() for pre in pres]
DISTS = ['uniform', 'eight_values', 'constant', 'tie_across_cut']


def make_conf(rng, dist, N, sizes, nms_pre):
    total = sum(sizes)
    if dist == 'uniform':
        conf = rng.random((N, total), dtype=np.float32)
        conf[conf == 0] = np.float32(0.5)                           # (0, 1)
        return conf
    if dist == 'eight_values':                                       # heavy ties, exact 0.0 and 1.0 among them
        vals = np.float32([0.0, 1.0, 0.125, 0.25, 0.3, 0.5, 0.75, 0.9])
        return vals[rng.integers(0, 8, (N, total))]
    if dist == 'constant':                                           # pure index order
        return np.full((N, total), 0.5, np.float32)
    # the k-th and the (k+1)-th objectness of every cut level are equal: k - 3 values above seven tied ones (as many as
    # the level has room for), the rest below, in random positions
    conf = np.empty((N, total), np.float32)
    for n in range(N):
        ab = 0
        for nl in sizes:
            k = nms_pre if 0 < nms_pre < nl else max(nl // 2, 1)
            above = max(k - 3, 0)
            tied = min(7, nl - above)
            v = np.concatenate([0.6 + 0.4 * rng.random(above, dtype=np.float32), np.full(tied, 0.5, np.float32),
                                0.4 * rng.random(nl - above - tied, dtype=np.float32)]).astype(np.float32)
            conf[n, ab:ab + nl] = v[rng.permutation(nl)]
            if 0 < nms_pre < nl and tied >= 2:
                s = np.sort(conf[n, ab:ab + nl])[::-1]
                assert s[k - 1] == s[k]
            ab += nl
    return conf


@pytest.mark.parametrize('dist', DISTS)
@pytest.mark.parametrize('layout,nms_pre', SLOT_CASES, ids=[f'{n}{p}' for n, p in SLOT_CASES])
def test_topk_slots_exact(gpu_device, layout, nms_pre, dist):
    sizes = list(LAYOUTS[layout][0])
    for N in (1, 3):
        rng = np.random.default_rng([ord(layout), nms_pre + 1, DISTS.index(dist), N])
        conf = make_conf(rng, dist, N, sizes, nms_pre)
        want, keys = R.slots_ref(conf, sizes, nms_pre)
        cut = any(0 < nms_pre < n for n in sizes)
        got = run_slots(gpu_device, conf, sizes, nms_pre, keys if cut else None)       # h-1, h500: topk_keys = NULL
        msg = R.diff_slots(got, want, R.slot_sizes(sizes, nms_pre))
        assert msg is None, f'{layout} nms_pre={nms_pre} {dist} N={N}: {msg}'


def level_descs(preds_dev, strides, base, A):
    levels = (pkg._lib.LevelDesc * len(preds_dev))()
    for i, p in enumerate(preds_dev):
        levels[i].pred = p.data_ptr()
        levels[i].H, levels[i].W, levels[i].stride = p.shape[1], p.shape[2], int(strides[i])
        for a in range(A):
            for c in range(4):
                levels[i].base_anchors[a][c] = float(base[i][a, c])
    return levels


def test_decode_topk_slots_chain(gpu_device):
    """yv4_decode_filter_v3 -> yv4_conf_topk_levels -> yv4_topk_slots on the 608-pixel level sizes (layout b), A = 3,
    C = 2: the selected admission keys and the slot table are those of the kernel's own conf.  The objectness logits
    lie on a grid of 1 / 4, so every level has exact ties, also across its cut."""
    lib = pkg._lib.lib()
    dev = gpu_device
    N, A, Cn, nms_pre = 3, 3, 2, 1000
    hw, strides = [(19, 19), (38, 38), (76, 76)], [32, 16, 8]
    sizes = [h * w * A for h, w in hw]
    assert tuple(sizes) == LAYOUTS['b'][0]
    total, L = sum(sizes), 3
    rng = np.random.default_rng(608)
    preds = []
    for h, w in hw:
        p = (rng.standard_normal((N, h, w, A, 5 + Cn)) * 2).astype(np.float32)
        p[..., 4] = np.round(p[..., 4] * 4) / 4
        preds.append(p.reshape(N, h, w, A * (5 + Cn)))
    base = R.base_anchors([[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)],
                           [(10, 13), (16, 30), (33, 23)]], strides)
    d_preds = [to_dev(p, dev) for p in preds]
    levels = level_descs(d_preds, strides, base, A)
    boxes = torch.empty((N, total, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((N, total), dtype=torch.float32, device=dev)
    cls = torch.empty((N, total, Cn), dtype=torch.float32, device=dev)
    dummy_keys = torch.empty(1, dtype=torch.int64, device=dev)
    counts = torch.zeros(N, dtype=torch.int32, device=dev)
    mx = torch.zeros(N, dtype=torch.float32, device=dev)
    work = torch.empty(lib.yv4_conf_topk_levels_work(N, total, L), dtype=torch.uint8, device=dev)
    topk = torch.zeros(N * L, dtype=torch.int64, device=dev)
    sizes_c = (C.c_int32 * L)(*sizes)
    S = sum(R.slot_sizes(sizes, nms_pre))
    slots = torch.full((N * S + 2 * PAD,), CANARY32, dtype=torch.int32, device=dev)
    assert lib.yv4_topk_slots_work(L, sizes_c, nms_pre) == 0
    torch.cuda.synchronize()
    check(lib.yv4_decode_filter_v3(levels, L, N, A, Cn, 1.0, -1.0, None, boxes.data_ptr(), conf.data_ptr(),
                                   cls.data_ptr(), dummy_keys.data_ptr(), 1, counts.data_ptr(), mx.data_ptr(), None,
                                   None), 'yv4_decode_filter_v3')
    check(lib.yv4_conf_topk_levels(levels, L, N, A, Cn, nms_pre, work.data_ptr(), topk.data_ptr(), None),
          'yv4_conf_topk_levels')
    check(lib.yv4_topk_slots(conf.data_ptr(), N, total, L, sizes_c, nms_pre, topk.data_ptr(), None,
                             slots.data_ptr() + PAD * 4, S, None), 'yv4_topk_slots')
    torch.cuda.synchronize()
    conf_np = conf.cpu().numpy()
    ref = R.decode_ref(preds, A, Cn, strides, base, v3=True)
    assert np.abs(conf_np - ref[1]).max() <= 1e-6
    want, keys = R.slots_ref(conf_np, sizes, nms_pre)
    for n in range(N):                                   # the premise: every level's cut falls between equal values
        ab = 0
        for nl in sizes:
            s = np.sort(conf_np[n, ab:ab + nl])[::-1]
            assert s[nms_pre - 1] == s[nms_pre]
            ab += nl
    got_keys = topk.cpu().numpy().view(np.uint64).reshape(N, L)
    bad = np.argwhere(got_keys != keys)
    assert not bad.size, (f'admission key of image {bad[0][0]} level {bad[0][1]}: got {int(got_keys[tuple(bad[0])]):#x}, '
                          f'want {int(keys[tuple(bad[0])]):#x}')
    out = slots.cpu().numpy()
    assert (out[:PAD] == CANARY32).all() and (out[PAD + N * S:] == CANARY32).all()
    msg = R.diff_slots(out[PAD:PAD + N * S].reshape(N, S), want, R.slot_sizes(sizes, nms_pre))
    assert msg is None, msg
    assert int(counts.sum()) == 0                        # score_thr = 1: no candidates


# ---------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------
# S per augmentation: slots 0..61, 62, 63.. of the first workgroup belong to three augmentations; S_total % 64 != 0
S_CYCLE = (62, 1, 65, 130, 5, 3, 1, 1, 64, 64, 17, 9, 128, 2, 31, 100)
SCORE_MODES = ['one_percent', 'all', 'none', 'at_threshold', 'conf_zero']
THR = 0.05


def make_augs(rng, num_augs, N, Cn, mode, flips=None, beyond=False):
    """Random merge inputs: a different total per augmentation, slots a random subset in random order, different meta
    rows for every (a, n) with four different scale-factor components.  beyond: every box lies past img_w and img_h."""
    thr32 = np.float32(THR)
    augs, meta = [], np.empty((num_augs, N, 6), np.float32)
    for a in range(num_augs):
        S = S_CYCLE[a % len(S_CYCLE)]
        total = S + 3 + 5 * a
        h, w = 300 + 13 * a + 7 * np.arange(N), 420 + 11 * a + 5 * np.arange(N)
        meta[a, :, 0], meta[a, :, 1] = h, w
        meta[a, :, 2:] = 0.4 + rng.random((N, 4), dtype=np.float32) * 1.5
        xy = rng.random((N, total, 2), dtype=np.float32) * np.float32([400, 300])
        wh = rng.random((N, total, 2), dtype=np.float32) * 120
        if beyond:
            xy += np.stack([w, h], -1)[:, None, :].astype(np.float32) + np.float32(1)
        boxes = np.concatenate([xy, xy + wh], -1).astype(np.float32)
        conf = rng.random((N, total), dtype=np.float32)
        u = rng.random((N, total, Cn), dtype=np.float32)
        if mode == 'one_percent':
            cls = np.where(u < 0.01, 0.5 + u * 40, u * thr32).astype(np.float32)
        elif mode == 'all':
            cls = (0.1 + 0.9 * u).astype(np.float32)
        elif mode == 'none':
            cls = (u * np.float32(0.04)).astype(np.float32)
        elif mode == 'at_threshold':              # the threshold itself and its two neighbours: only the upper passes
            pick = rng.integers(0, 4, (N, total, Cn))
            cls = np.choose(pick, [np.full_like(u, thr32), np.full_like(u, np.nextafter(thr32, np.float32(1))),
                                   np.full_like(u, np.nextafter(thr32, np.float32(0))), u]).astype(np.float32)
        else:                                     # conf_zero: the score is 0.0, the class still passes on cls
            cls = u
            conf[rng.random((N, total)) < 0.5] = 0.0
        slots = np.stack([rng.permutation(total)[:S] for _ in range(N)]).astype(np.int32)
        flip = flips[a] if flips is not None else a % 4
        augs.append(dict(boxes=boxes, conf=conf, cls=cls, slots=slots, flip=int(flip), S=S, total=total))
    return augs, meta


def run_merge(dev, augs, meta, Cn, thr, key_cap):
    lib = pkg._lib.lib()
    A, N = len(augs), meta.shape[1]
    S_total = sum(g['S'] for g in augs)
    table = (pkg._lib.TtaAug * A)()
    keep = []
    for a, g in enumerate(augs):
        t = [to_dev(g[k], dev) for k in ('boxes', 'conf', 'cls', 'slots')]
        keep.append(t)
        table[a].boxes, table[a].conf, table[a].cls, table[a].slots = (x.data_ptr() for x in t)
        table[a].total, table[a].S, table[a].flip = g['total'], g['S'], g['flip']
    d_meta = to_dev(meta, dev)
    boxes_out = torch.full((N * S_total * 4 + 2 * PAD,), float('nan'), dtype=torch.float32, device=dev)
    keys = torch.from_numpy(np.full(N * key_cap + PAD, CANARY64, np.uint64).view(np.int64)).to(dev)
    counts = torch.full((N,), 77, dtype=torch.int32, device=dev)
    mx = torch.full((N,), 3.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    check(lib.yv4_decode_reset(counts.data_ptr(), mx.data_ptr(), N, None), 'yv4_decode_reset')
    check(lib.yv4_tta_merge(table, A, N, Cn, thr, d_meta.data_ptr(), boxes_out.data_ptr() + PAD * 4, keys.data_ptr(),
                            key_cap, counts.data_ptr(), mx.data_ptr(), None), 'yv4_tta_merge')
    torch.cuda.synchronize()
    b = boxes_out.cpu().numpy()
    assert np.isnan(b[:PAD]).all() and np.isnan(b[PAD + N * S_total * 4:]).all(), 'boxes_out written out of bounds'
    k = keys.cpu().numpy().view(np.uint64)
    assert (k[N * key_cap:] == CANARY64).all(), 'words after the key buffers were written'
    return dict(boxes=torch.from_numpy(b[PAD:PAD + N * S_total * 4].reshape(N, S_total, 4).copy()),
                keys=k[:N * key_cap].reshape(N, key_cap), counts=counts.cpu().numpy(), max_coord=mx.cpu().numpy())


def check_merge(got, want, augs, Cn, tag, overflow=()):
    """got against merge_ref's (boxes_out, keys, max_coord); the images in `overflow` hold more candidates than
    key_cap (their keys are checked by the caller)."""
    boxes, keys, mc = want
    seg = [g['S'] for g in augs]
    if not torch.equal(got['boxes'], torch.from_numpy(boxes)):
        raise AssertionError(f'{tag}: ' + R.diff_bits(got['boxes'].numpy(), boxes, 'boxes_out'))
    msg = R.diff_bits(got['max_coord'], mc, 'max_coord')
    assert msg is None, f'{tag}: {msg}'
    cap = got['keys'].shape[1]
    for n in range(boxes.shape[0]):
        assert got['counts'][n] == keys[n].size, f'{tag}: counts[{n}] = {got["counts"][n]}, want {keys[n].size}'
        if n in overflow:
            continue
        cnt = keys[n].size
        msg = R.diff_keys(got['keys'][n, :cnt], keys[n], Cn, seg, image=n)
        assert msg is None, f'{tag}: {msg}'
        assert np.array_equal(np.sort(got['keys'][n, :cnt]), keys[n])
        assert (got['keys'][n, cnt:cap] == CANARY64).all(), f'{tag}: image {n}: keys past counts[n] were written'


@pytest.mark.parametrize('num_augs', [1, 4, 16])
@pytest.mark.parametrize('Cn', [1, 3, 80, 81])
def test_tta_merge_exact(gpu_device, Cn, num_augs):
    for N in (1, 3):
        for mode in SCORE_MODES:
            rng = np.random.default_rng([Cn, num_augs, N, SCORE_MODES.index(mode)])
            augs, meta = make_augs(rng, num_augs, N, Cn, mode)
            want = R.merge_ref(augs, meta, Cn, THR)
            S_total = sum(g['S'] for g in augs)
            tag = f'C={Cn} augs={num_augs} N={N} {mode}'
            counts = [k.size for k in want[1]]
            if mode == 'all':
                assert counts == [S_total * Cn] * N
            elif mode == 'none':
                assert counts == [0] * N and np.isneginf(want[2]).all()
            elif mode == 'at_threshold':
                assert 0 < min(counts) and max(counts) < S_total * Cn
            got = run_merge(gpu_device, augs, meta, Cn, THR, S_total * Cn)
            check_merge(got, want, augs, Cn, tag)
            if mode == 'none':                                        # the key buffers are untouched
                assert (got['keys'] == CANARY64).all() and (got['counts'] == 0).all()
                assert np.isneginf(got['max_coord']).all()


def test_tta_merge_negative_max_coord(gpu_device):
    """Every box lies beyond img_w and img_h and every augmentation flips diagonally: the mapped coordinates, and so
    max_coord, are negative (the atomicMin-on-unsigned branch of the float maximum)."""
    Cn, num_augs, N = 3, 4, 3
    rng = np.random.default_rng(77)
    augs, meta = make_augs(rng, num_augs, N, Cn, 'one_percent', flips=[3] * num_augs, beyond=True)
    want = R.merge_ref(augs, meta, Cn, THR)
    assert (want[0] < 0).all() and (want[2] < 0).all() and np.isfinite(want[2]).all()
    assert min(k.size for k in want[1]) >= 2                          # more than one workgroup's atomic per image
    got = run_merge(gpu_device, augs, meta, Cn, THR, sum(g['S'] for g in augs) * Cn)
    check_merge(got, want, augs, Cn, 'negative max_coord')


@pytest.mark.parametrize('Cn', [3, 80])
def test_tta_merge_key_cap_exact_and_overflow(gpu_device, Cn):
    """key_cap equal to the largest image's passing count loses nothing; with one less, counts[n] still reports the
    full number, exactly key_cap distinct keys of the expected set are written (which one is dropped depends on the
    order of arrival), and the next image's keys and the words after the buffers are intact."""
    num_augs, N = 4, 3
    rng = np.random.default_rng([9, Cn])
    augs, meta = make_augs(rng, num_augs, N, Cn, 'all')
    for g in augs:                                                    # image 0 passes the most, image 2 the fewest
        u = rng.random(g['cls'].shape, dtype=np.float32)
        g['cls'] = (u * np.float32([1.0, 0.12, 0.08])[:, None, None]).astype(np.float32)
    want = R.merge_ref(augs, meta, Cn, THR)
    counts = [k.size for k in want[1]]
    assert counts[0] > counts[1] > counts[2] > 0
    got = run_merge(gpu_device, augs, meta, Cn, THR, counts[0])
    check_merge(got, want, augs, Cn, 'key_cap = count')
    cap = counts[0] - 1
    got = run_merge(gpu_device, augs, meta, Cn, THR, cap)
    check_merge(got, want, augs, Cn, 'key_cap = count - 1', overflow=(0,))
    written = got['keys'][0]
    assert np.unique(written).size == cap, 'an overflowing image must still fill its key_cap slots with distinct keys'
    stray = written[~np.isin(written, want[1][0])]
    assert not stray.size, f'{stray.size} written keys are no candidates of image 0, the first {int(stray[0]):#018x}'
