"""Plain-numpy statement of the VOC-style mAP this package computes on the GPU (map_eval.py): box overlaps, the
two true/false-positive rules, and the per-class accumulation into recall / precision / AP.

Written from the rules, not from any implementation: tests/test_map_host.py holds it bit for bit against
tests/golden/map_eval.npz (what the reference produced under numpy 2), and tests/test_gpu_map_eval.py holds the
kernels against it on inputs the fixture does not cover (score ties, odd shapes).

Number formats, as the rules in map_eval.py's docstring state them: boxes, IoUs, thresholds and area bounds are
float32 and compared in float32; the cumulative tp / fp counts are float32; recall is float64 (a float32 count over
an int64 gt count), precision and ap are float32.
"""
import numpy as np

F32_EPS = np.finfo(np.float32).eps


def f32(a):
    return np.asarray(a, dtype=np.float32)


def areas(b):
    b = f32(b)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def overlaps(b1, b2, mode='iou', eps=1e-6):
    """(n, 4+) x (k, 4+) -> (n, k) float32: intersection over max(union, eps); 'iof' divides by b1's area."""
    assert mode in ('iou', 'iof')
    b1, b2 = f32(b1), f32(b2)
    n, k = len(b1), len(b2)
    if n == 0 or k == 0:
        return np.zeros((n, k), np.float32)
    a1, a2 = areas(b1)[:, None], areas(b2)[None, :]
    w = np.maximum(np.minimum(b1[:, None, 2], b2[None, :, 2]) - np.maximum(b1[:, None, 0], b2[None, :, 0]), np.float32(0))
    h = np.maximum(np.minimum(b1[:, None, 3], b2[None, :, 3]) - np.maximum(b1[:, None, 1], b2[None, :, 1]), np.float32(0))
    inter = w * h
    denom = (a1 + a2) - inter if mode == 'iou' else np.broadcast_to(a1, inter.shape)
    out = inter / np.maximum(denom, np.float32(eps))
    assert out.dtype == np.float32
    return out


def _ranges(area_ranges):
    """None / [(None, None)] -> [None]; else float32 (lo, hi) pairs."""
    if area_ranges is None:
        return [None]
    return [None if lo is None else (np.float32(lo), np.float32(hi)) for lo, hi in area_ranges]


def _inside(a, rng):
    return np.ones(len(a), bool) if rng is None else (a >= rng[0]) & (a < rng[1])


def _outside(a, rng):
    return np.zeros(len(a), bool) if rng is None else (a < rng[0]) | (a >= rng[1])


def _stack_gts(gts, ignored):
    gts = f32(gts).reshape(-1, 4)
    ignored = np.zeros((0, 4), np.float32) if ignored is None else f32(ignored).reshape(-1, 4)
    return np.concatenate([gts, ignored]), np.concatenate([np.zeros(len(gts), bool), np.ones(len(ignored), bool)])


def tpfp_default(dets, gts, ignored=None, iou_thr=0.5, area_ranges=None):
    """One (image, class).  A detection is judged by the gt it overlaps most (first one on a tie): below the
    threshold it is a false positive if its own area is in range; at or above it, it is nothing when that gt is
    ignored or out of range, the true positive when it is the first in score order to claim the gt, and a false
    positive after that.  Returns (tp, fp), float32 (num_ranges, num_dets), columns in the detections' own order."""
    dets = f32(dets)
    gt, ign = _stack_gts(gts, ignored)
    rngs = _ranges(area_ranges)
    tp = np.zeros((len(rngs), len(dets)), np.float32)
    fp = np.zeros_like(tp)
    det_area, gt_area = areas(dets), areas(gt)
    if len(gt) == 0:
        for k, r in enumerate(rngs):
            fp[k, _inside(det_area, r)] = 1
        return tp, fp
    iou = overlaps(dets, gt)
    best, which = iou.max(axis=1), iou.argmax(axis=1)
    thr = np.float32(iou_thr)
    visit = np.argsort(-dets[:, -1])
    for k, r in enumerate(rngs):
        dead = ign | _outside(gt_area, r)
        free = np.ones(len(gt), bool)
        inside = _inside(det_area, r)
        for d in visit:
            if best[d] >= thr:
                g = which[d]
                if dead[g]:
                    continue
                (tp if free[g] else fp)[k, d] = 1
                free[g] = False
            elif inside[d]:
                fp[k, d] = 1
    return tp, fp


def tpfp_imagenet(dets, gts, ignored=None, iou_thr=0.5, area_ranges=None):
    """One (image, class), ImageNet rule.  Overlaps are taken against the gts moved by -1; gt j asks for
    min(w*h / ((w+10)*(h+10)), iou_thr).  In score order every detection takes the free gt it overlaps most among
    those whose own threshold it reaches (first one on a tie) and uses it up -- ignored or not; it is a true positive
    if that gt is neither ignored nor out of range, nothing otherwise, and without a gt a false positive if its own
    area is in range."""
    dets = f32(dets)
    gt, ign = _stack_gts(gts, ignored)
    rngs = _ranges(area_ranges)
    tp = np.zeros((len(rngs), len(dets)), np.float32)
    fp = np.zeros_like(tp)
    det_area = areas(dets)
    if len(gt) == 0:
        for k, r in enumerate(rngs):
            fp[k, _inside(det_area, r)] = 1
        return tp, fp
    iou = overlaps(dets, gt - np.float32(1))
    w, h = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    need = np.minimum((w * h) / ((w + np.float32(10)) * (h + np.float32(10))), np.float32(iou_thr))
    gt_area = w * h
    visit = np.argsort(-dets[:, -1])
    for k, r in enumerate(rngs):
        dead = ign | _outside(gt_area, r)
        free = np.ones(len(gt), bool)
        inside = _inside(det_area, r)
        for d in visit:
            ok = free & (iou[d] >= need)
            if ok.any():
                cand = np.where(ok, iou[d], np.float32(-np.inf))
                g = int(cand.argmax())
                free[g] = False
                if not dead[g]:
                    tp[k, d] = 1
            elif inside[d]:
                fp[k, d] = 1
    return tp, fp


def average_precision(recall, precision, mode='area'):
    """One curve: the area under the precision envelope (over the steps of recall, curve closed with (0, 0) and
    (1, 0)), or the mean over recall levels 0, 0.1 .. 1 of the best precision at or beyond the level.  float32."""
    ap = np.zeros(1, np.float32)
    if mode == 'area':
        r = np.concatenate([np.zeros(1, recall.dtype), recall, np.ones(1, recall.dtype)])
        p = np.concatenate([np.zeros(1, recall.dtype), precision, np.zeros(1, recall.dtype)])
        p = np.maximum.accumulate(p[::-1])[::-1]
        step = np.flatnonzero(r[1:] != r[:-1])
        ap[0] = np.sum((r[step + 1] - r[step]) * p[step + 1])
    else:
        for level in np.arange(0, 1 + 1e-3, 0.1):
            reach = precision[recall >= level]
            ap[0] += reach.max() if reach.size else 0
        ap /= 11
    return ap[0]


def class_problem(det_results, annotations, c):
    """Per image the class's detections, gts and ignored gts."""
    out = []
    for dets, ann in zip(det_results, annotations):
        gts = f32(ann['bboxes']).reshape(-1, 4)[np.asarray(ann['labels']) == c]
        if ann.get('labels_ignore') is not None:
            ign = f32(ann['bboxes_ignore']).reshape(-1, 4)[np.asarray(ann['labels_ignore']) == c]
        else:
            ign = np.zeros((0, 4), np.float32)
        out.append((f32(dets[c]), gts, ign))
    return out


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None, rule=None):
    """(mean_ap, per-class dicts num_gts / num_dets / recall / precision / ap) for one threshold."""
    rule = rule or (tpfp_imagenet if dataset in ('det', 'vid') else tpfp_default)
    area_ranges = None if scale_ranges is None else [(lo ** 2, hi ** 2) for lo, hi in scale_ranges]
    rngs = _ranges(area_ranges)
    results = []
    for c in range(len(det_results[0])):
        probs = class_problem(det_results, annotations, c)
        flags = [rule(d, g, i, iou_thr, area_ranges) for d, g, i in probs]
        num_gts = np.zeros(len(rngs), dtype=int)
        for _, g, _ in probs:
            for k, r in enumerate(rngs):
                num_gts[k] += np.sum(_inside(areas(g), r))
        dets = np.concatenate([d for d, _, _ in probs])
        by_score = np.argsort(-dets[:, -1])
        tp = np.cumsum(np.concatenate([f[0] for f in flags], axis=1)[:, by_score], axis=1)
        fp = np.cumsum(np.concatenate([f[1] for f in flags], axis=1)[:, by_score], axis=1)
        recall = tp / np.maximum(num_gts[:, None], F32_EPS)
        precision = tp / np.maximum(tp + fp, F32_EPS)
        assert recall.dtype == np.float64 and precision.dtype == np.float32
        mode = '11points' if dataset == 'voc07' else 'area'
        ap = np.array([average_precision(r, p, mode) for r, p in zip(recall, precision)], np.float32)
        if scale_ranges is None:
            recall, precision, ap, num_gts = recall[0], precision[0], ap[0], num_gts.item()
        results.append(dict(num_gts=num_gts, num_dets=len(dets), recall=recall, precision=precision, ap=ap))
    if scale_ranges is None:
        aps = [r['ap'] for r in results if r['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    else:
        ap = np.stack([r['ap'] for r in results])
        n = np.stack([r['num_gts'] for r in results])
        mean_ap = [ap[n[:, k] > 0, k].mean() if (n[:, k] > 0).any() else 0.0 for k in range(ap.shape[1])]
    return mean_ap, results
