"""Plain-numpy statement of the proposal recall this package computes on the GPU (recall_eval.py, csrc/recall.hip), and
the writing and reading of tests/golden/recall.npz.

Written from the rules, not from any implementation.  tests/test_recall_host.py holds it bit for bit against the
fixture, which the reference's own ``eval_recalls`` produced under numpy 2; tests/test_gpu_recall.py holds the kernel
against both.

Ordering: an ``(n, 5)`` array is visited by descending score, equal scores in input order (stable: the one stated
difference from the reference, whose ``np.argsort(scores)[::-1]`` is an unstable sort, reversed); an ``(n, 4)`` array
keeps its order.  Per image ``cols = min(n, proposal_nums[-1])`` -- the last entry, as ``recall.py:96`` has it -- and the
IoU block is ``_map_ref.overlaps(gts, proposals[:cols, :4])``.  Per proposal number and image, on the block's first
``min(cols, pn)`` columns, the ``G`` steps of ``recall.py:24-31`` taken literally.  ``counts[k, t]`` compares the float32
value, widened, with the float64 threshold; ``recalls = counts / float(total_gt)``.  The reference's sort of the
recorded values (``recall.py:35``) changes no count and is not made: ``gt_ious`` here are in recording order.
"""
import numpy as np

import _map_ref as R

SETS = ('main', 'hand', 'hand_unsorted', 'wide')


def visiting_order(p):
    """One image's proposals (n, 4) or (n, 5) -> (n, 4) float32 in visiting order."""
    p = R.f32(p)
    if p.size == 0:
        return np.zeros((0, 4), np.float32)
    assert p.ndim == 2 and p.shape[1] in (4, 5), p.shape
    if p.shape[1] == 5:
        p = p[np.argsort(-p[:, 4], kind='stable')]
    return p[:, :4]


def greedy(ious):
    """recall.py:24-31 on a copy of the (G, c) block, c >= 1: G recorded values, float32."""
    ious = ious.copy()
    G = ious.shape[0]
    out = np.zeros(G, np.float32)
    rows = np.arange(G)
    for j in range(G):
        arg = ious.argmax(axis=1)                  # first occurrence
        best = ious[rows, arg]
        g = best.argmax()                          # the first row holding the largest maximum
        out[j] = best[g]
        b = arg[g]
        ious[g, :] = -1
        ious[:, b] = -1
    return out


def gt_ious(gts, proposals, proposal_nums):
    """(M, total_gt) float32: per proposal number, image by image, the recorded values in recording order."""
    nums = [int(n) for n in np.asarray(proposal_nums).reshape(-1)]
    rows = [[] for _ in nums]
    for g, p in zip(gts, proposals):
        if g is None or np.asarray(g).size == 0:
            continue                                # an image without gts records nothing
        g = R.f32(g).reshape(-1, 4)
        p = visiting_order(p)
        cols = min(len(p), nums[-1])
        block = R.overlaps(g, p[:cols])
        for k, pn in enumerate(nums):
            c = min(cols, pn)
            rows[k].append(greedy(block[:, :c]) if c > 0 else np.zeros(len(g), np.float32))
    return np.stack([np.concatenate(r) if r else np.zeros(0, np.float32) for r in rows]).astype(np.float32)


def recalls(gts, proposals, proposal_nums, iou_thrs, return_ious=False):
    """(M, T) float64 (and the (M, total_gt) recorded values)."""
    v = gt_ious(gts, proposals, proposal_nums)
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    counts = np.stack([(v.astype(np.float64) >= t).sum(axis=1) for t in thrs], axis=1).astype(np.int64)
    with np.errstate(all='ignore'):
        out = counts / float(v.shape[1])
    return (out, v) if return_ious else out


def concat_classes(results):
    """A detector's results (per image a per-class list) -> per image one (n, 5) array, classes in order."""
    return [np.concatenate([R.f32(c).reshape(-1, 5) for c in per_cls], axis=0) for per_cls in results]


def flat_form(proposals):
    """Per-image (n, 5) arrays -> (dets (D, 5), labels (D,), img_index (D,))."""
    dets = np.concatenate([np.zeros((0, 5), np.float32)] + [R.f32(p).reshape(-1, 5) for p in proposals], axis=0)
    idx = np.repeat(np.arange(len(proposals), dtype=np.int64), [len(p) for p in proposals])
    return dets, np.zeros(len(dets), np.int64), idx


# ---- the fixture: per set the inputs flat, the parameters, the reference's recalls and its sorted _ious ---------------
def store_set(out, name, gts, proposals, proposal_nums, iou_thrs, recalls_ref, sorted_ious):
    gl = [np.zeros((0, 4), np.float32) if g is None else np.asarray(g, np.float32).reshape(-1, 4) for g in gts]
    out[f'{name}/gt'] = np.concatenate(gl, axis=0)
    out[f'{name}/ng'] = np.array([len(g) for g in gl], np.int64)
    out[f'{name}/gt_none'] = np.array([g is None for g in gts], bool)
    width = np.array([0 if np.asarray(p).size == 0 else np.asarray(p).shape[1] for p in proposals], np.int64)
    out[f'{name}/width'] = width
    out[f'{name}/nd'] = np.array([0 if np.asarray(p).size == 0 else len(p) for p in proposals], np.int64)
    flat = [np.asarray(p, np.float32).reshape(-1) for p in proposals]
    out[f'{name}/det'] = np.concatenate([np.zeros(0, np.float32)] + flat)
    out[f'{name}/proposal_nums'] = np.asarray(proposal_nums, np.int64)
    out[f'{name}/iou_thrs'] = np.asarray(iou_thrs, np.float64)
    out[f'{name}/recalls'] = np.asarray(recalls_ref, np.float64)
    out[f'{name}/sorted_ious'] = np.asarray(sorted_ious, np.float32)


def load_set(z, name):
    """(gts, proposals, proposal_nums, iou_thrs, recalls, sorted_ious)."""
    ng, nd, width = z[f'{name}/ng'], z[f'{name}/nd'], z[f'{name}/width']
    none = z[f'{name}/gt_none']
    gts = [None if none[i] else g for i, g in enumerate(np.split(z[f'{name}/gt'], np.cumsum(ng)[:-1]))]
    sizes = nd * width
    proposals = [d.reshape(-1, w) if w else np.zeros((0, 4), np.float32)
                 for d, w in zip(np.split(z[f'{name}/det'], np.cumsum(sizes)[:-1]), width)]
    return (gts, proposals, [int(n) for n in z[f'{name}/proposal_nums']], z[f'{name}/iou_thrs'], z[f'{name}/recalls'],
            z[f'{name}/sorted_ious'])
