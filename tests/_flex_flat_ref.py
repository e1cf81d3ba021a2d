"""Plain-numpy statement of metric='fast-bbox' (eval_map_flexible) for the FLAT form (eval_utils.py, "The flat path"):
the detections come as one table ``(dets (D, 5), labels (D,), img_index (D,))`` and everything the list path does per
(image, class) problem on the host -- problem keys, the two stable orders, the breakdown mask, the accumulation -- is
defined here without reference to any implementation.

The IoU and the greedy matching are the oracle's ``iou_coco`` / ``match_coco`` (oracle/eval_oracle.py), called per problem
with the detections already in visiting order: descending score, stable, so ties keep the flat table's order (the list
path's ties follow ``argsort()[::-1]``: the one stated difference).

Accumulation: over the class's detections by descending score (stable), the mask compacts the list; integer cumulative
counts; precision = ctp / k and recall = ctp / num_gt (/ 1e-7 when num_gt == 0) in float64; the AP is the sum of
(recall_m - recall_prev) * envelope_m over the positions where recall changes, ONE float64 accumulator in rank order
(np.cumsum(terms)[-1]; np.sum adds pairwise), rounded to float32.  tests/test_flex_flat_host.py holds this bit for bit
against the oracle's eval_map_flexible on inputs without score ties.
"""
import numpy as np

from _map_flat_ref import flatten, problem_keys, stable_desc  # noqa: F401  (flatten: for the tests)
from oracle import eval_oracle as E


def breakdown_names(scale_ranges):
    return ['All'] + list(scale_ranges or {})


def det_rows(boxes, bounds):
    """(B, n) own breakdown flags of detections: row 0 always, row b: lo <= area < hi, all in float32."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    area = w * h
    assert area.dtype == np.float32 and bounds.dtype == np.float32
    rows = np.ones((1 + len(bounds), len(boxes)), bool)
    for b, (lo, hi) in enumerate(bounds):
        rows[1 + b] = (area >= lo) & (area < hi)
    return rows


def single_sum(recall, precision):
    """The AP of one compacted curve (float64 in, float32 out): the single accumulator."""
    if len(recall) == 0:
        return np.float32(0)
    env = np.maximum.accumulate(precision[::-1])[::-1]
    prev = np.concatenate([np.zeros(1, np.float64), recall[:-1]])
    step = recall != prev
    terms = (recall[step] - prev[step]) * env[step]
    assert terms.dtype == np.float64
    return np.float32(np.cumsum(terms)[-1]) if len(terms) else np.float32(0)


def eval_flex_flat(flat, annotations, num_classes, iou_thrs, scale_ranges=None, shared_tp=True):
    """dict of num_det (C, B, T) int64, num_gt (C, B) int64, recall (C, B, T) float64, mAP (C, B, T) float32."""
    dets, labels, img_index = flat
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    N, C = len(annotations), num_classes
    names = breakdown_names(scale_ranges)
    ranges = [(lo * lo, hi * hi) for lo, hi in (scale_ranges or {}).values()]
    bounds = np.array(ranges, np.float32).reshape(-1, 2)            # rounded to float32 once
    B, T, D = len(names), len(iou_thrs), len(dets)
    thrs = np.array(iou_thrs, np.float32)
    part, key = problem_keys(labels, img_index, N, C)
    out = dict(num_det=np.zeros((C, B, T), np.int64), num_gt=np.zeros((C, B), np.int64),
               recall=np.zeros((C, B, T), np.float64), mAP=np.zeros((C, B, T), np.float32))
    for c in range(C):
        rows = np.flatnonzero(part & (key // N == c))               # the class's rows in flat order
        tp = np.zeros((B, T, D), bool)                              # columns: flat rows
        msk = np.zeros((B, T, D), bool)
        for i, anno in enumerate(annotations):
            m = np.asarray(anno['gt_labels']).reshape(-1) == c
            gb = np.asarray(anno['gt_bboxes'], np.float32).reshape(-1, 4)[m]
            ga = {k: np.asarray(v)[m] for k, v in (anno.get('gt_attrs') or {}).items()}
            crowd = ga['iscrowd'].astype(bool) if 'iscrowd' in ga else np.zeros(len(gb), bool)
            gt_bkd = E._breakdown_rows(gb, ga, ranges, True)        # ignore applied
            out['num_gt'][c] += gt_bkd.sum(axis=1)
            mine = rows[key[rows] == c * N + i]
            visit = mine[stable_desc(dets[mine, 4])]                # flat rows in visiting order
            db = dets[visit, :4]
            own_flag = det_rows(db, bounds)
            if len(gb) and len(db):
                iou = E.iou_coco(db, gb, crowd)
                mg = np.stack([E.match_coco(iou, thrs, ~gt_bkd[b], crowd) for b in range(B)])      # (B, T, nd)
            else:
                mg = np.full((B, T, len(db)), -1, np.int32)         # a problem with no ground truth matches nothing
            for b in range(B):
                own = mg[b]
                tp[b][:, visit] = (mg[B - 1] if shared_tp else own) > -1
                inn = np.broadcast_to(own_flag[b], own.shape).copy()
                hit = own > -1
                inn[hit] = gt_bkd[b][own[hit]]
                msk[b][:, visit] = inn
        by_score = rows[stable_desc(dets[rows, 4])]
        for b in range(B):
            num_gt = int(out['num_gt'][c, b])
            den = np.float64(num_gt) if num_gt >= 1 else np.float64(1e-7)
            for t in range(T):
                sel = msk[b, t, by_score]
                ctp = np.cumsum(tp[b, t, by_score][sel].astype(np.int64))
                n = len(ctp)
                precision = ctp.astype(np.float64) / np.arange(1, n + 1, dtype=np.int64).astype(np.float64)
                recall = ctp.astype(np.float64) / den
                out['num_det'][c, b, t] = n
                out['recall'][c, b, t] = recall[-1] if n else 0.0
                out['mAP'][c, b, t] = single_sum(recall, precision)
    return out


def flatten_as_visited(det_results):
    """The flat table of per-image lists with the rows of a class in the order the LIST path ranks them: per problem
    ``argsort()[::-1]``, the problems concatenated in image order, ``argsort()[::-1]`` again (statistics_single and
    statistics_accumulate).  The flat definition keeps the table's order among equal scores, and this table reproduces
    tests/golden/eval.npz, whose scores hold ties.  No general recipe: the flat path visits a problem's tied detections
    in this class-level order restricted to the problem, the list path in the problem's own ``argsort()[::-1]`` order;
    where the two differ the greedy matching does too.  On the fixture they do not."""
    rows, labels, imgs = [np.zeros((0, 5), np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for c in range(len(det_results[0])):
        parts, im = [], []
        for i, det in enumerate(det_results):
            d = np.asarray(det[c], np.float32).reshape(-1, 5)
            parts.append(d[d[:, -1].argsort()[::-1]])
            im += [i] * len(d)
        cat, im = np.concatenate(parts), np.array(im, np.int64)
        rank = cat[:, -1].argsort()[::-1]
        rows.append(cat[rank])
        imgs.append(im[rank])
        labels.append(np.full(len(rank), c, np.int64))
    return np.concatenate(rows), np.concatenate(labels), np.concatenate(imgs)


def as_list(out, classes, scale_ranges, iou_thrs):
    """The (key, value) list of FlexibleStatisticsEval.statistics_eval: class, breakdown, threshold."""
    names = breakdown_names(scale_ranges)
    res = []
    for c in range(out['mAP'].shape[0]):
        for b, name in enumerate(names):
            for t, thr in enumerate(iou_thrs):
                res.append((dict(class_name=classes[c], breakdown=name, iou_threshold=thr),
                            dict(num_det=int(out['num_det'][c, b, t]), num_gt=int(out['num_gt'][c, b]),
                                 recall=out['recall'][c, b, t], mAP=out['mAP'][c, b, t])))
    return res


def report(res, report_config):
    return {name: np.mean([v['mAP'] for k, v in res if cond(k) and v['num_gt'] > 0]) for name, cond in report_config}


def table(res):
    """(num_det, num_gt, recall, mAP) arrays of a (key, value) list, in its order."""
    return (np.array([v['num_det'] for _, v in res], np.int64), np.array([v['num_gt'] for _, v in res], np.int64),
            np.array([v['recall'] for _, v in res], np.float64), np.array([v['mAP'] for _, v in res], np.float32))


def keys(res):
    return [(k['class_name'], k['breakdown'], k['iou_threshold']) for k, _ in res]


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def _boxes(rng, n):
    xy = rng.uniform(0, 400, (n, 2))
    wh = rng.uniform(4, 160, (n, 2)) * rng.choice([0.15, 0.5, 1.0], (n, 1))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def synth(seed=0, num_img=40, num_cls=5, quant=None, clutter=60):
    """Detections that are noisy copies of the gts (three qualities) plus clutter; some gts ignored, some crowd, the
    ``area`` attribute now and then unlike the box; every 7th image without gts, every 11th without detections; the
    last class never among the gts.  Scores: pairwise distinct within a class, or (``quant``) drawn from that many
    values.  Returns (per-image lists, annotations, class names)."""
    rng = np.random.default_rng(seed)
    dets, annos = [], []
    for i in range(num_img):
        ng = int(rng.integers(0, 9)) if i % 7 else 0
        gb = _boxes(rng, ng)
        gl = rng.integers(0, max(num_cls - 1, 1), ng).astype(np.int64)
        wh = gb[:, 2:] - gb[:, :2]
        area = (wh[:, 0] * wh[:, 1] * rng.choice([1.0, 1.0, 0.3], ng)).astype(np.float32)
        crowd = rng.random(ng) < 0.15
        ignore = crowd | (rng.random(ng) < 0.15)
        attrs = dict(ignore=ignore, iscrowd=crowd, area=area)
        if i % 5 == 1:
            attrs = dict(ignore=ignore)                       # no crowd flags, areas from the boxes
        if i % 5 == 2:
            attrs = {}
        per_cls = []
        for c in range(num_cls):
            mine = gb[gl == c]
            reps = [mine + rng.normal(0, s, mine.shape).astype(np.float32) for s in (1.0, 6.0, 20.0)]
            cand = np.concatenate(reps + [_boxes(rng, int(rng.integers(0, clutter)))], 0)
            cand = cand[rng.random(len(cand)) < 0.8]
            if i % 11 == 3:
                cand = cand[:0]
            per_cls.append(cand.astype(np.float32))
        dets.append(per_cls)
        annos.append(dict(gt_bboxes=gb, gt_labels=gl, gt_attrs=attrs))
    for c in range(num_cls):
        n = sum(len(d[c]) for d in dets)
        if quant is None:
            sc = (rng.choice(50000, size=n, replace=False) / 50000).astype(np.float32)
            assert len(np.unique(sc)) == n
        else:
            sc = (rng.integers(0, quant, n) / quant).astype(np.float32)
        lo = 0
        for d in dets:
            m = len(d[c])
            d[c] = np.concatenate([d[c], sc[lo:lo + m, None]], 1).astype(np.float32)
            lo += m
    return dets, annos, [f'c{c}' for c in range(num_cls)]
