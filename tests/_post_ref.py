"""Numpy restatement of the post-processing chain between the pred maps and the NMS: the decode (both heads), the
candidate keys of yv4_decode_filter / yv4_decode_filter_v3, the slot tables of yv4_topk_slots and the merge of
yv4_tta_merge.  TEST INFRASTRUCTURE ONLY: no torch.cuda, no library call.

What is integer or a single IEEE fp32 operation in the kernels (csrc/tta.hip, csrc/postproc.hip are built with
-ffp-contract=off) is restated in uint32 / uint64 / float32 and compared bit for bit: the order-preserving keys, the
slot tables, the flip subtraction, the division by scale_factor, cls * conf.  The decode itself (sigmoid, exp) is
restated in float64 and compared to a tolerance.

A key is (score_to_key(score) << 32) | flat: ascending key = descending score, ties to the lower flat index.
"""
import numpy as np

U32 = np.uint32
U64 = np.uint64
ALL_ADMITTING = U64(0xFFFFFFFFFFFFFFFF)      # yv4_conf_topk_levels' key of a level that is not cut


# ---- keys (csrc/nms_common.h score_to_key / key_to_score, csrc/tta.hip conf_key) ------------------------------------
def score_to_key(s):
    u = np.ascontiguousarray(s, dtype=np.float32).view(U32)
    asc = np.where((u & U32(0x80000000)) != 0, ~u, u | U32(0x80000000))
    return (~asc).astype(U32)


def key_to_score(k):
    u = ~np.asarray(k, dtype=U32)
    u = np.where((u & U32(0x80000000)) != 0, u & U32(0x7FFFFFFF), ~u)
    return np.ascontiguousarray(u, dtype=U32).view(np.float32)


def conf_key(cf, j):
    return (score_to_key(cf).astype(U64) << U64(32)) | np.asarray(j).astype(U64)


def key_flat(keys):
    return (np.asarray(keys, dtype=U64) & U64(0xFFFFFFFF)).astype(np.int64)


def key_score(keys):
    return key_to_score((np.asarray(keys, dtype=U64) >> U64(32)).astype(U32))


# ---- slot tables (yolo_head.py:254-311 with with_nms=False) ---------------------------------------------------------
def slot_sizes(level_sizes, nms_pre):
    return [nms_pre if 0 < nms_pre < n else n for n in level_sizes]


def slots_ref(conf, level_sizes, nms_pre):
    """conf (N, total) float32 -> slots (N, S) int32 and the admission keys (N, num_levels) uint64: the k-th smallest
    conf_key of a cut level (what yv4_conf_topk_levels returns and yv4_topk_slots receives), all ones otherwise."""
    conf = np.asarray(conf, dtype=np.float32)
    N = conf.shape[0]
    assert conf.shape[1] == sum(level_sizes)
    ks = slot_sizes(level_sizes, nms_pre)
    slots = np.empty((N, sum(ks)), np.int32)
    keys = np.full((N, len(level_sizes)), ALL_ADMITTING, U64)
    for n in range(N):
        ab = sb = 0
        for l, (nl, k) in enumerate(zip(level_sizes, ks)):
            idx = np.arange(ab, ab + nl)
            if k < nl:
                order = np.lexsort((idx, -conf[n, idx].astype(np.float64)))[:k]
                idx = idx[order]
                keys[n, l] = np.sort(conf_key(conf[n, ab:ab + nl], np.arange(ab, ab + nl)))[k - 1]
                # the two statements of the order agree (they would not for -0.0 against +0.0: a sigmoid gives neither)
                assert keys[n, l] == conf_key(conf[n, idx[-1]], idx[-1])
            slots[n, sb:sb + k] = idx
            ab += nl
            sb += k
    return slots, keys


# ---- merge (dense_test_mixins.py:38-100 up to multiclass_nms) -------------------------------------------------------
def merge_ref(augs, meta, num_classes, score_thr):
    """augs: per augmentation a dict of boxes (N, total, 4), conf (N, total), cls (N, total, C), slots (N, S), flip
    (bit 0 mirrors x, bit 1 y); meta (num_augs, N, 6) float32 rows img_h, img_w, scale_factor[4].
    Returns boxes_out (N, S_total, 4) float32, the sorted uint64 keys per image and max_coord (N,) float32."""
    meta = np.asarray(meta, dtype=np.float32)
    thr = np.float32(score_thr)
    N, C = meta.shape[1], num_classes
    mapped, confs, clss = [], [], []
    for a, g in enumerate(augs):
        n_idx = np.arange(N)[:, None]
        sl = np.asarray(g['slots'])
        b = np.asarray(g['boxes'], dtype=np.float32)[n_idx, sl]                  # (N, S, 4)
        h, w = meta[a, :, 0][:, None], meta[a, :, 1][:, None]
        x1, y1, x2, y2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
        if g['flip'] & 1:
            x1, x2 = w - b[..., 2], w - b[..., 0]
        if g['flip'] & 2:
            y1, y2 = h - b[..., 3], h - b[..., 1]
        out = np.stack([x1, y1, x2, y2], -1).astype(np.float32) / meta[a, :, None, 2:6]
        assert out.dtype == np.float32
        mapped.append(out)
        confs.append(np.asarray(g['conf'], dtype=np.float32)[n_idx, sl])
        clss.append(np.asarray(g['cls'], dtype=np.float32)[n_idx, sl].reshape(N, sl.shape[1], C))
    boxes_out = np.concatenate(mapped, 1)
    conf, cls = np.concatenate(confs, 1), np.concatenate(clss, 1)
    score = cls * conf[..., None]
    assert score.dtype == np.float32
    keys, max_coord = [], np.full(N, -np.inf, np.float32)
    for n in range(N):
        m, c = np.nonzero(cls[n] > thr)
        flat = (m * C + c).astype(U64)
        keys.append(np.sort((score_to_key(score[n, m, c]).astype(U64) << U64(32)) | flat))
        if m.size:
            max_coord[n] = boxes_out[n, np.unique(m)].max()
    return boxes_out, keys, max_coord


# ---- decode (include/yv4.h, csrc/postproc.hip, oracle/) in float64 --------------------------------------------------
def base_anchors(base_sizes, strides):
    """anchor_generator.py:639-665: centre stride / 2, python-float arithmetic, then fp32."""
    return [np.array([[s / 2. - 0.5 * w, s / 2. - 0.5 * h, s / 2. + 0.5 * w, s / 2. + 0.5 * h] for w, h in per],
                     dtype=np.float32) for per, s in zip(base_sizes, strides)]


def decode_ref(preds, A, num_classes, strides, base, v3, scale_factor=None):
    """preds: per level (N, H, W, A * (5 + C)) NHWC logits.  Box j of a level is (y * W + x) * A + a.  Returns float64
    boxes (N, total, 4), conf (N, total), cls (N, total, C)."""
    attr = 5 + num_classes
    boxes, confs, clss = [], [], []
    for p, stride, ba in zip(preds, strides, base):
        N, H, W, _ = p.shape
        m = np.asarray(p, dtype=np.float64).reshape(N, H, W, A, attr)
        s = 1.0 / (1.0 + np.exp(-m))
        ba = np.asarray(ba, dtype=np.float64)[:A]
        gx = (np.arange(W, dtype=np.float64) * stride)[None, None, :, None]
        gy = (np.arange(H, dtype=np.float64) * stride)[None, :, None, None]
        ax1, ay1, ax2, ay2 = ba[:, 0] + gx, ba[:, 1] + gy, ba[:, 2] + gx, ba[:, 3] + gy
        xc, yc, aw, ah = (ax1 + ax2) * 0.5, (ay1 + ay2) * 0.5, ax2 - ax1, ay2 - ay1
        if v3:                              # yolo_bbox_coder.py:76-83
            xcp = (s[..., 0] - 0.5) * stride + xc
            ycp = (s[..., 1] - 0.5) * stride + yc
            wp, hp = np.exp(m[..., 2]) * aw, np.exp(m[..., 3]) * ah
        else:                               # yolocsp_head.py:273-275, yolov4_bbox_coder.py:51-66
            xcp = (s[..., 0] * 2.0 - 1.0) * stride + xc
            ycp = (s[..., 1] * 2.0 - 1.0) * stride + yc
            wp, hp = (s[..., 2] * 2.0) ** 2 * aw, (s[..., 3] * 2.0) ** 2 * ah
        b = np.stack([xcp - wp / 2, ycp - hp / 2, xcp + wp / 2, ycp + hp / 2], -1).reshape(N, -1, 4)
        boxes.append(b)
        confs.append(s[..., 4].reshape(N, -1))
        clss.append(s[..., 5:].reshape(N, H * W * A, num_classes))
    boxes = np.concatenate(boxes, 1)
    if scale_factor is not None:
        boxes = boxes / np.asarray(scale_factor, dtype=np.float64)[:, None, :]
    return boxes, np.concatenate(confs, 1), np.concatenate(clss, 1)


def candidates_from(conf, cls, score_thr, v3, level_sizes=None, topk_keys=None, conf_thr=0.0):
    """The exact candidate keys of yv4_decode_filter (v3 = False) / yv4_decode_filter_v3 from given float32 conf
    (N, total) and cls (N, total, C), or cls None for the class-agnostic head.  The score is cls * conf (one fp32
    product); the threshold test `> score_thr` is on cls * conf (CSP head) or on cls (v3).  topk_keys: (N,) admission
    keys per image, or (N, num_levels) per level: a box is admitted when conf_key(conf, j) <= its key.  v3 with
    conf_thr > 0: boxes with conf >= conf_thr only.
    Returns the sorted keys per image and the admitted mask (N, total)."""
    conf = np.asarray(conf, dtype=np.float32)
    thr = np.float32(score_thr)
    N, total = conf.shape
    j = np.arange(total)
    admitted = np.ones((N, total), bool)
    if topk_keys is not None:
        tk = np.asarray(topk_keys, dtype=U64).reshape(N, -1)
        if tk.shape[1] > 1:
            assert tk.shape[1] == len(level_sizes)
            tk = np.repeat(tk, level_sizes, axis=1)
        admitted &= conf_key(conf, np.broadcast_to(j, conf.shape)) <= tk
    if v3 and conf_thr > 0:
        admitted &= conf >= np.float32(conf_thr)
    keys = []
    for n in range(N):
        if cls is None:
            b = np.nonzero(admitted[n] & (conf[n] > thr))[0]
            keys.append(np.sort(conf_key(conf[n, b], b)))
            continue
        c_n = np.asarray(cls[n], dtype=np.float32)
        C = c_n.shape[1]
        score = c_n * conf[n][:, None]
        assert score.dtype == np.float32
        b, c = np.nonzero(((c_n if v3 else score) > thr) & admitted[n][:, None])
        keys.append(np.sort((score_to_key(score[b, c]).astype(U64) << U64(32)) | (b * C + c).astype(U64)))
    return keys, admitted


# ---- comparator: the first differing element, by name ---------------------------------------------------------------
def _where(index, sizes, names):
    """index into a concatenation of segments -> 'level 1 slot 17' (names = ('level', 'slot'))."""
    base = 0
    for s, n in enumerate(sizes):
        if index < base + n:
            return f'{names[0]} {s} {names[1]} {index - base}'
        base += n
    return f'{names[1]} {index} (past the last {names[0]})'


def diff_slots(got, want, seg_sizes):
    """Slot tables (N, S): None, or the first differing slot as 'image n level l slot s'."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f'slot tables of shape {got.shape} and {want.shape}'
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    n, s = bad[0]
    return f'image {n} {_where(s, seg_sizes, ("level", "slot"))}: got anchor {got[n, s]}, want {want[n, s]}'


def diff_keys(got, want, num_classes, seg_sizes, names=('augmentation', 'slot'), image=0):
    """Two key sets of one image, each a uint64 array in any order: None, or the first difference in ascending key
    order, named as image, segment (level or augmentation), box (slot) and class."""
    got, want = np.sort(np.asarray(got, dtype=U64)), np.sort(np.asarray(want, dtype=U64))
    C = max(num_classes, 1)

    def name(k):
        flat = int(key_flat(k))
        return (f'image {image} {_where(flat // C, seg_sizes, names)} class {flat % C} '
                f'(score {float(key_score(k).reshape(-1)[0])!r}, key {int(k):#018x})')
    n = min(got.size, want.size)
    bad = np.nonzero(got[:n] != want[:n])[0]
    if not bad.size:
        if got.size == want.size:
            return None
        return (f'{got.size} keys, want {want.size}: ' +
                (f'missing {name(want[n])}' if want.size > n else f'unexpected {name(got[n])}'))
    i = bad[0]
    g, w = got[i], want[i]
    if key_flat(g) == key_flat(w):
        return f'score differs: got {name(g)}, want {name(w)}'
    if w < g:                       # the expected key is absent from got (or present later with another score)
        same = got[key_flat(got) == key_flat(w)]
        if same.size:
            return f'score differs: got {name(same[0])}, want {name(w)}'
        return f'missing {name(w)}'
    same = want[key_flat(want) == key_flat(g)]
    if same.size:
        return f'score differs: got {name(g)}, want {name(same[0])}'
    return f'unexpected {name(g)}'


def diff_bits(got, want, what):
    """float32 arrays compared by bits (leading axis = image): None or the first differing element."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f'{what} of shape {got.shape} and {want.shape}'
    bad = np.argwhere(got.view(U32) != want.view(U32))
    if not bad.size:
        return None
    i = tuple(bad[0])
    rest = f' element {tuple(int(v) for v in i[1:])}' if len(i) > 1 else ''
    return (f'{what} image {i[0]}{rest}: got {float(got[i])!r} ({int(got.view(U32)[i]):#010x}), '
            f'want {float(want[i])!r} ({int(want.view(U32)[i]):#010x})')
