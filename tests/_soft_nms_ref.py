"""Host restatement of soft-NMS (mmcv-full 1.3.x softnms_cpu, offset 0) and of batched_nms / multiclass_nms around it,
as defined in include/yv4.h and DESIGN 12.  numpy float32 throughout, in the C loop's operation order.

Two forms of the op: ``soft_nms_loop`` is the literal loop; ``soft_nms_fast`` runs one step at a time over whole arrays
and replaces the end swaps of a step by the compaction rule (the k-th discarded position from the left below the new end
receives the k-th surviving entry from the right at or above it).  tests/test_soft_nms_host.py checks the two forms
against each other.
"""
import numpy as np

METHODS = {'naive': 0, 'linear': 1, 'gaussian': 2}
F32 = np.float32


def _weight(ovr, method, thr, sigma):
    if method == 0:
        return np.where(ovr >= thr, F32(0), F32(1)).astype(F32)
    if method == 1:
        return np.where(ovr >= thr, F32(1) - ovr, F32(1)).astype(F32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.exp(-(ovr * ovr) / sigma).astype(F32)


def _ovr(bi, ai, b, a):
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        xx1 = np.maximum(bi[0], b[..., 0])
        yy1 = np.maximum(bi[1], b[..., 1])
        xx2 = np.minimum(bi[2], b[..., 2])
        yy2 = np.minimum(bi[3], b[..., 3])
        w = np.maximum(F32(0), xx2 - xx1)
        h = np.maximum(F32(0), yy2 - yy1)
        inter = w * h
        return (inter / (ai + a - inter)).astype(F32)


def _prep(boxes, scores, iou_threshold, sigma, min_score, method):
    b = np.ascontiguousarray(boxes, dtype=F32).reshape(-1, 4).copy()
    s = np.ascontiguousarray(scores, dtype=F32).reshape(-1).copy()
    if isinstance(method, str):
        method = METHODS[method]
    return b, s, F32(iou_threshold), F32(sigma), F32(min_score), int(method)


def soft_nms_loop(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', max_out=-1):
    """The literal loop.  Returns (dets (k,5) float32: box as given + current score at selection, inds (k,) int64)."""
    b, s, thr, sig, ms, m = _prep(boxes, scores, iou_threshold, sigma, min_score, method)
    n = b.shape[0]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    idx = np.arange(n, dtype=np.int64)
    dets, inds = [], []
    i, nb = 0, n
    while i < nb and (max_out <= 0 or i < max_out):
        mp = i
        for pos in range(i + 1, nb):
            if s[mp] < s[pos]:
                mp = pos
        for arr in (b, s, area, idx):
            arr[[i, mp]] = arr[[mp, i]]
        dets.append(np.concatenate([b[i], s[i:i + 1]]))
        inds.append(idx[i])
        bi, ai = b[i].copy(), area[i]
        pos = i + 1
        while pos < nb:
            ovr = _ovr(bi, ai, b[pos], area[pos])
            s[pos] = s[pos] * _weight(ovr, m, thr, sig)
            if s[pos] < ms:
                for arr in (b, s, area, idx):
                    arr[pos] = arr[nb - 1]
                nb -= 1
                continue
            pos += 1
        i += 1
    return np.asarray(dets, dtype=F32).reshape(-1, 5), np.asarray(inds, dtype=np.int64)


def compact(order, discarded, nb):
    """The end swaps of one step as the compaction rule.  ``order``: entries at positions [0, nb) (any array);
    ``discarded``: bool per position (only positions > the step's winner).  Returns the array of the new length."""
    d = int(discarded.sum())
    nb2 = nb - d
    holes = np.nonzero(discarded[:nb2])[0]                      # ascending
    movers = np.nonzero(~discarded[nb2:nb])[0][::-1] + nb2      # surviving positions >= nb2, from the right
    out = order[:nb2].copy()
    out[holes] = order[movers]
    return out


def soft_nms_fast(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', max_out=-1):
    """The same loop, one vectorised step at a time (same selections, same permutation)."""
    b, s, thr, sig, ms, m = _prep(boxes, scores, iou_threshold, sigma, min_score, method)
    n = b.shape[0]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    perm = np.arange(n, dtype=np.int64)           # perm[pos] = entry at position pos
    dets, inds = [], []
    i, nb = 0, n
    while i < nb and (max_out <= 0 or i < max_out):
        mp = i + int(np.argmax(s[perm[i:nb]]))     # first position of the maximum
        perm[[i, mp]] = perm[[mp, i]]
        w = perm[i]
        dets.append(np.concatenate([b[w], s[w:w + 1]]))
        inds.append(w)
        rest = perm[i + 1:nb]
        if rest.size:
            s[rest] = s[rest] * _weight(_ovr(b[w], area[w], b[rest], area[rest]), m, thr, sig)
            disc = np.zeros(nb, dtype=bool)
            disc[i + 1:nb] = s[rest] < ms
            if disc.any():
                perm = np.concatenate([compact(perm[:nb], disc, nb), perm[nb:]])
                nb -= int(disc.sum())
        i += 1
    return np.asarray(dets, dtype=F32).reshape(-1, 5), np.asarray(inds, dtype=np.int64)


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', max_out=-1):
    n = np.asarray(boxes).reshape(-1, 4).shape[0]
    f = soft_nms_loop if n <= 200 else soft_nms_fast
    return f(boxes, scores, iou_threshold, sigma, min_score, method, max_out)


def _resort(keep, scores):
    """(score desc, index asc)."""
    order = np.lexsort((keep, -scores.astype(np.float64)))
    return keep[order], scores[order]


def batched_soft_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv batched_nms with type='soft_nms', the decayed split form (scores_after_nms).  numpy in/out.
    Returns (dets (k,5), keep (k,) int64)."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    assert cfg.pop('type', 'soft_nms') == 'soft_nms'
    split_thr = cfg.pop('split_thr', 10000)
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=F32).reshape(-1)
    idxs = np.asarray(idxs).reshape(-1)
    if class_agnostic:
        bfn = boxes
    else:
        off = (idxs.astype(F32) * (boxes.max() + F32(1))).astype(F32)
        bfn = (boxes + off[:, None]).astype(F32)
    if bfn.shape[0] < split_thr:
        if 'max_num' in cfg:
            raise TypeError("soft_nms() got an unexpected keyword argument 'max_num'")
        dets, keep = soft_nms(bfn, scores, **cfg)
        return np.concatenate([boxes[keep], dets[:, 4:5]], 1), keep
    max_num = cfg.pop('max_num', -1)
    mask = np.zeros(scores.shape[0], dtype=bool)
    after = np.zeros(scores.shape[0], dtype=F32)
    for cid in np.unique(idxs):
        sel = np.nonzero(idxs == cid)[0]
        dets, k = soft_nms(bfn[sel], scores[sel], **cfg)
        mask[sel[k]] = True
        after[sel[k]] = dets[:, 4]
    keep = np.nonzero(mask)[0]
    keep, sc = _resort(keep, after[keep])
    if max_num > 0:
        keep, sc = keep[:max_num], sc[:max_num]
    return np.concatenate([boxes[keep], sc[:, None]], 1).astype(F32), keep


def multiclass_soft_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """bbox_nms.py:7-93 around batched_soft_nms.  Returns (dets, labels, flat index of every survivor)."""
    multi_bboxes = np.asarray(multi_bboxes, dtype=F32)
    multi_scores = np.asarray(multi_scores, dtype=F32)
    C = multi_scores.shape[1] - 1
    bboxes = np.broadcast_to(multi_bboxes[:, None], (multi_scores.shape[0], C, 4)).reshape(-1, 4)
    scores = multi_scores[:, :-1].reshape(-1)
    labels = np.broadcast_to(np.arange(C), (multi_scores.shape[0], C)).reshape(-1)
    valid = scores > F32(score_thr)
    if score_factors is not None:
        scores = (scores * np.repeat(np.asarray(score_factors, dtype=F32), C)).astype(F32)
    inds = np.nonzero(valid)[0]
    if inds.size == 0:                            # the reference returns the (0, 4) boxes here (bbox_nms.py:75-82)
        return np.zeros((0, 4), F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    dets, keep = batched_soft_nms(bboxes[inds], scores[inds], labels[inds], nms_cfg)
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    return dets, labels[inds][keep].astype(np.int64), inds[keep]
