"""Plain-numpy statement of the VOC-style mAP of the FLAT form (map_eval.py, "The flat form"): the detections come as
one table ``(dets (D, 5), labels (D,), img_index (D,))`` and everything the list path leaves to the host -- problem
keys, the two orders, the accumulation -- is defined here without reference to any implementation.

The two true/false-positive rules are tests/_map_ref.py's.  They visit a problem's detections by ``np.argsort`` of the
negated score, whose tie order is not defined; here the order IS defined (descending score, stable: ties keep the flat
table's order), so a problem's detections are handed to the rules already in visiting order with the score column
replaced by a strictly descending stand-in.  The rules read the scores for nothing else.

Accumulation: integer cumulative tp / fp, recall float64 (a float32 count over max(int64 num_gts, float32 eps)),
precision float32, AP float32.  The float64 sum of the 'area' AP is ONE accumulator in rank order: np.cumsum(terms)[-1]
(np.sum adds pairwise).  tests/test_map_flat_host.py holds all of this bit for bit against tests/golden/map_eval.npz,
whose scores are pairwise distinct within every class.
"""
import numpy as np

import _map_ref as R

F32_EPS = R.F32_EPS


def stable_desc(scores):
    """Positions by descending score, stable; +0 and -0 are equal."""
    return np.argsort(-(np.asarray(scores, np.float32) + np.float32(0)), kind='stable')


def problem_keys(labels, img_index, num_imgs, num_classes):
    """(takes part, label * N + img_index): a label outside [0, C) or an image outside [0, N) takes no part."""
    labels, img_index = np.asarray(labels, np.int64).reshape(-1), np.asarray(img_index, np.int64).reshape(-1)
    part = (labels >= 0) & (labels < num_classes) & (img_index >= 0) & (img_index < num_imgs)
    return part, labels * num_imgs + img_index


def average_precision(recall, precision, mode='area'):
    ap = np.zeros(1, np.float32)
    if mode == 'area':
        r = np.concatenate([np.zeros(1, np.float64), recall, np.ones(1, np.float64)])
        p = np.concatenate([np.zeros(1, np.float64), precision.astype(np.float64), np.zeros(1, np.float64)])
        p = np.maximum.accumulate(p[::-1])[::-1]
        step = np.flatnonzero(r[1:] != r[:-1])
        terms = (r[step + 1] - r[step]) * p[step + 1]
        assert terms.dtype == np.float64 and len(terms)          # 0 -> 1 always holds a step
        ap[0] = np.cumsum(terms)[-1]
    else:
        for level in np.arange(0, 1 + 1e-3, 0.1):
            reach = precision[recall >= level]
            ap[0] += reach.max() if reach.size else 0
        ap /= 11
    return ap[0]


def accumulate(tp, fp, num_gts, mode):
    """tp / fp (K, n) flags in the per-class order, num_gts (K,) int -> recall (K, n) float64, precision (K, n)
    float32, ap (K,) float32."""
    ctp = np.cumsum(tp.astype(np.int64), axis=1).astype(np.float32)
    cfp = np.cumsum(fp.astype(np.int64), axis=1).astype(np.float32)
    recall = ctp / np.maximum(np.asarray(num_gts)[:, None], F32_EPS)
    precision = ctp / np.maximum(ctp + cfp, F32_EPS)
    assert recall.dtype == np.float64 and precision.dtype == np.float32
    ap = np.array([average_precision(r, p, mode) for r, p in zip(recall, precision)], np.float32)
    return recall, precision, ap


def eval_map_flat(flat, annotations, num_classes, scale_ranges=None, iou_thr=0.5, dataset=None, rule=None):
    """(mean_ap, per-class dicts num_gts / num_dets / recall / precision / ap) for one threshold, full curves."""
    dets, labels, img_index = flat
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    N, C = len(annotations), num_classes
    part, key = problem_keys(labels, img_index, N, C)
    rule = rule or (R.tpfp_imagenet if dataset in ('det', 'vid') else R.tpfp_default)
    area_ranges = None if scale_ranges is None else [(lo ** 2, hi ** 2) for lo, hi in scale_ranges]
    rngs = R._ranges(area_ranges)
    mode = '11points' if dataset == 'voc07' else 'area'
    results = []
    for c in range(C):
        rows = np.flatnonzero(part & (key // N == c))            # the class's rows in flat order
        tp = np.zeros((len(rngs), len(dets)), np.float32)        # columns: flat rows
        fp = np.zeros_like(tp)
        num_gts = np.zeros(len(rngs), dtype=int)
        for i, ann in enumerate(annotations):
            gts = R.f32(ann['bboxes']).reshape(-1, 4)[np.asarray(ann['labels']).reshape(-1) == c]
            ign = np.zeros((0, 4), np.float32)
            if ann.get('labels_ignore') is not None:
                ign = R.f32(ann['bboxes_ignore']).reshape(-1, 4)[np.asarray(ann['labels_ignore']).reshape(-1) == c]
            for k, r in enumerate(rngs):
                num_gts[k] += np.sum(R._inside(R.areas(gts), r))
            mine = rows[key[rows] == c * N + i]
            visit = mine[stable_desc(dets[mine, 4])]             # flat rows in visiting order
            d = dets[visit].copy()
            d[:, 4] = -np.arange(len(d), dtype=np.float32)       # the order, made explicit
            a, b = rule(d, gts, ign, iou_thr, area_ranges)
            tp[:, visit], fp[:, visit] = a, b
        by_score = rows[stable_desc(dets[rows, 4])]
        recall, precision, ap = accumulate(tp[:, by_score], fp[:, by_score], num_gts, mode)
        if scale_ranges is None:
            recall, precision, ap, num_gts = recall[0], precision[0], ap[0], num_gts.item()
        results.append(dict(num_gts=num_gts, num_dets=len(rows), recall=recall, precision=precision, ap=ap))
    if scale_ranges is None:
        aps = [r['ap'] for r in results if r['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    else:
        ap = np.stack([r['ap'] for r in results])
        n = np.stack([r['num_gts'] for r in results])
        mean_ap = [ap[n[:, k] > 0, k].mean() if (n[:, k] > 0).any() else 0.0 for k in range(ap.shape[1])]
    return mean_ap, results


def flatten(det_results):
    """Per image a per-class list of (n, 5) arrays -> the flat form, rows in (image, class, row) order."""
    dets, labels, img = [np.zeros((0, 5), np.float32)], [], []
    for i, per_cls in enumerate(det_results):
        for c, d in enumerate(per_cls):
            dets.append(np.asarray(d, np.float32).reshape(-1, 5))
            labels += [c] * len(d)
            img += [i] * len(d)
    return np.concatenate(dets), np.array(labels, np.int64), np.array(img, np.int64)
