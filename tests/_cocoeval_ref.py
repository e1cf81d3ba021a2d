"""A numpy restatement of COCOeval (iouType='bbox', useCats=1, pycocotools 2.0.x) as the docstring of
mmdet_yolov4_amd/coco_eval.py defines it: straight loops, float64, kind='mergesort'.  Host only; the GPU tests hold the
kernels to it bit for bit, tests/test_coco_eval_host.py holds IT to hand-computed values.

``coco_eval(dataset, dets, labels, img_index, cat_ids, img_ids, ...)`` returns ``precision`` / ``scores`` (T, R, K, A, M),
``recall`` (T, K, A, M), ``counts`` (K, A), ``stats`` (12), ``bits`` (the per-detection matched / ignored flags of the
detections kept by maxDets[-1], in (problem, rank) order) and ``events``, counters of the definition's corner cases."""
from collections import defaultdict

import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']
EVENTS = ('crowd_rematch', 'stop_rule', 'equal_iou_replace', 'iou_equals_threshold', 'area_on_bound', 'search_past_end',
          'problems_cut')


def det_box(b):
    """xyxy2xywh of coco.py:175-193 on a float32 row: the subtraction in float64, after the conversion."""
    return [float(b[0]), float(b[1]), float(b[2]) - float(b[0]), float(b[3]) - float(b[1])]


def iou_pair(d, g, crowd):
    dx, dy, dw, dh = d
    gx, gy, gw, gh = g
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if h <= 0:
        return 0.0
    inter = w * h
    da, ga = dw * dh, gw * gh
    union = da if crowd else da + ga - inter
    return inter / union


def default_iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def coco_eval(dataset, dets, labels, img_index, cat_ids, img_ids, iou_thrs=None, max_dets=(100, 300, 1000),
              params_cat_ids=None, params_img_ids=None):
    ev = dict.fromkeys(EVENTS, 0)
    iou_thrs = default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    max_dets = sorted(int(m) for m in max_dets)
    imgIds = [int(i) for i in np.unique(img_ids if params_img_ids is None else params_img_ids)]
    catIds = [int(c) for c in np.unique(cat_ids if params_cat_ids is None else params_cat_ids)]
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(catIds), len(AREA_RNG), len(max_dets)
    N = len(imgIds)
    img_set, cat_set = set(imgIds), set(catIds)

    # _prepare
    gts, dts = defaultdict(list), defaultdict(list)
    for ann in dataset['annotations']:
        if ann['image_id'] in img_set and ann['category_id'] in cat_set:
            crowd = bool(ann.get('iscrowd', 0))
            gts[ann['image_id'], ann['category_id']].append(
                dict(box=[float(v) for v in ann['bbox']], area=float(ann['area']), crowd=crowd, ignore=crowd))
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    for n in range(len(dets)):
        img, cat = int(img_ids[int(img_index[n])]), int(cat_ids[int(labels[n])])
        if img in img_set and cat in cat_set:
            box = det_box(dets[n])
            dts[img, cat].append(dict(box=box, score=float(dets[n, 4]), area=box[2] * box[3], index=n))

    # computeIoU + evaluateImg
    bounds = {float(v) for rng in AREA_RNG for v in rng} - {0.0, 1e10}
    evals = {}                                             # (k, a, i) -> dict
    bits = dict(index=[], problem=[], rank=[], matched=[], ignored=[])
    for i, img in enumerate(imgIds):
        for k, cat in enumerate(catIds):
            gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
            if not gt and not dt:
                continue
            inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
            dt = [dt[j] for j in inds]
            if len(dt) > max_dets[-1]:
                ev['problems_cut'] += 1
                dt = dt[:max_dets[-1]]
            ious = [[iou_pair(d['box'], g['box'], g['crowd']) for g in gt] for d in dt]
            ev['area_on_bound'] += sum(g['area'] in bounds for g in gt) + sum(d['area'] in bounds for d in dt)
            ev['iou_equals_threshold'] += sum(v in iou_thrs for row in ious for v in row)
            dtm_all = np.zeros((A, T, len(dt)), bool)
            dtig_all = np.zeros((A, T, len(dt)), bool)
            for a, (lo, hi) in enumerate(AREA_RNG):
                g_ig = [1 if (g['ignore'] or g['area'] < lo or g['area'] > hi) else 0 for g in gt]
                gtind = np.argsort(g_ig, kind='mergesort')
                gt_s = [gt[j] for j in gtind]
                gt_ig = [g_ig[j] for j in gtind]
                crowd = [g['crowd'] for g in gt_s]
                iou_s = [[row[j] for j in gtind] for row in ious]
                G, D = len(gt_s), len(dt)
                gtm = np.zeros((T, G), bool)
                dtm = np.zeros((T, D), bool)
                dtig = np.zeros((T, D), bool)
                if G and D:
                    for tind, t in enumerate(iou_thrs):
                        taken = [False] * G
                        for dind in range(D):
                            best = min(t, 1 - 1e-10)
                            m = -1
                            row = iou_s[dind]
                            for gind in range(G):
                                if taken[gind] and not crowd[gind]:
                                    continue
                                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                                    ev['stop_rule'] += 1
                                    break
                                if row[gind] < best:
                                    continue
                                if m > -1 and row[gind] == best:
                                    ev['equal_iou_replace'] += 1
                                if taken[gind]:
                                    ev['crowd_rematch'] += 1
                                best = row[gind]
                                m = gind
                            if m == -1:
                                continue
                            dtig[tind, dind] = gt_ig[m]
                            dtm[tind, dind] = True
                            taken[m] = True
                        gtm[tind] = taken
                d_out = np.array([d['area'] < lo or d['area'] > hi for d in dt], bool).reshape(1, D)
                dtig = dtig | (~dtm & d_out)
                evals[k, a, i] = dict(scores=np.array([d['score'] for d in dt], np.float64), dtm=dtm, dtig=dtig,
                                      gt_ig=np.array(gt_ig, bool))
                dtm_all[a], dtig_all[a] = dtm, dtig
            bits['index'] += [d['index'] for d in dt]
            bits['problem'] += [i * K + k] * len(dt)
            bits['rank'] += list(range(len(dt)))
            bits['matched'].append(dtm_all)
            bits['ignored'].append(dtig_all)
    bits = dict(index=np.array(bits['index'], np.int64), problem=np.array(bits['problem'], np.int64),
                rank=np.array(bits['rank'], np.int64),
                matched=np.concatenate(bits['matched'] + [np.zeros((A, T, 0), bool)], axis=2),
                ignored=np.concatenate(bits['ignored'] + [np.zeros((A, T, 0), bool)], axis=2))

    # accumulate
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    counts = np.zeros((K, A), np.int64)
    for k in range(K):
        for a in range(A):
            E = [evals[k, a, i] for i in range(N) if (k, a, i) in evals]
            counts[k, a] = sum(int(np.count_nonzero(~e['gt_ig'])) for e in E)
            for m, max_det in enumerate(max_dets):
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e['scores'][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                sorted_scores = dt_scores[inds]
                dtm = np.concatenate([e['dtm'][:, 0:max_det] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e['dtig'][:, 0:max_det] for e in E], axis=1)[:, inds]
                npig = int(counts[k, a])
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    # for i in range(nd - 1, 0, -1): if pr[i] > pr[i - 1]: pr[i - 1] = pr[i]  -- a running maximum from
                    # the right (a maximum rounds nothing, so the vectorised form gives the same bits)
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    where = np.searchsorted(rc, rec_thrs, side='left')
                    for ri, pi in enumerate(where):
                        if pi >= nd:
                            ev['search_past_end'] += 1
                            break
                        q[ri] = pr[pi]
                        ss[ri] = sorted_scores[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    out = dict(precision=precision, recall=recall, scores=scores, counts=counts, bits=bits, events=ev,
               iou_thrs=iou_thrs, max_dets=max_dets, cat_ids=catIds, img_ids=imgIds)
    out['stats'] = summarize(out)
    return out


def _summarize(res, ap=1, iou_thr=None, area='all', max_dets=100):
    aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
    mind = [i for i, m in enumerate(res['max_dets']) if m == max_dets]
    s = res['precision'] if ap == 1 else res['recall']
    if iou_thr is not None:
        s = s[np.where(iou_thr == res['iou_thrs'])[0]]
    s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
    return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])


def summarize(res):
    md = res['max_dets']
    stats = np.zeros((12,))
    stats[0] = _summarize(res, 1)
    stats[1] = _summarize(res, 1, iou_thr=.5, max_dets=md[2])
    stats[2] = _summarize(res, 1, iou_thr=.75, max_dets=md[2])
    stats[3] = _summarize(res, 1, area='small', max_dets=md[2])
    stats[4] = _summarize(res, 1, area='medium', max_dets=md[2])
    stats[5] = _summarize(res, 1, area='large', max_dets=md[2])
    stats[6] = _summarize(res, 0, max_dets=md[0])
    stats[7] = _summarize(res, 0, max_dets=md[1])
    stats[8] = _summarize(res, 0, max_dets=md[2])
    stats[9] = _summarize(res, 0, area='small', max_dets=md[2])
    stats[10] = _summarize(res, 0, area='medium', max_dets=md[2])
    stats[11] = _summarize(res, 0, area='large', max_dets=md[2])
    return stats


def evaluate_bbox(res, metric_items=None):
    """The reference's result dict (coco.py:626-640) from a restatement result."""
    names = {'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5, 'AR@100': 6, 'AR@300': 7,
             'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10, 'AR_l@1000': 11}
    out = {}
    for item in metric_items or ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']:
        out[f'bbox_{item}'] = float(f'{res["stats"][names[item]]:.3f}')
    ap = res['stats'][:6]
    out['bbox_mAP_copypaste'] = f'{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} {ap[4]:.3f} {ap[5]:.3f}'
    return out


# ---- the shared cases of the host and GPU tests -----------------------------------------------------------------------
def _ann(aid, img, cat, box, area=None, iscrowd=0, **extra):
    return dict(id=aid, image_id=img, category_id=cat, bbox=list(box), area=box[2] * box[3] if area is None else area,
                iscrowd=iscrowd, **extra)


def _dataset(n_img, cats, anns):
    return dict(images=[dict(id=i, width=640, height=640, file_name=f'{i}.jpg') for i in n_img],
                categories=[dict(id=c, name=f'c{c}') for c in cats], annotations=anns)


def _flat(rows):
    """rows: (img_index, label, x1, y1, x2, y2, score)"""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return rows[:, 2:].astype(np.float32), rows[:, 1].astype(np.int64), rows[:, 0].astype(np.int64)


def case_a():
    ds = _dataset([1], [1], [_ann(1, 1, 1, (0, 0, 100, 100)), _ann(2, 1, 1, (200, 200, 100, 100))])
    return ds, _flat([(0, 0, 0, 0, 100, 100, .9), (0, 0, 400, 400, 500, 500, .8), (0, 0, 200, 200, 300, 300, .7)]), {}


def case_b():
    ds = _dataset([1], [1], [_ann(1, 1, 1, (0, 0, 100, 100)), _ann(2, 1, 1, (200, 200, 200, 200), iscrowd=1)])
    return ds, _flat([(0, 0, 210, 210, 260, 260, .95), (0, 0, 300, 300, 380, 380, .9), (0, 0, 0, 0, 100, 100, .5)]), {}


def case_c():
    ds = _dataset([1], [1, 2], [_ann(1, 1, 1, (0, 0, 100, 100))])
    return ds, _flat([(0, 0, 0, 0, 100, 100, .9), (0, 1, 10, 10, 60, 60, .8)]), {}


def case_d():
    ds = _dataset([1], [1], [_ann(1, 1, 1, (0, 0, 100, 100))])
    dets = _flat([(0, 0, 300, 300, 400, 400, .9), (0, 0, 500, 300, 600, 400, .8), (0, 0, 0, 0, 100, 100, .7),
                  (0, 0, 300, 500, 400, 600, .6)])
    return ds, dets, dict(max_dets=(2, 3, 5))


CASES = dict(A=case_a, B=case_b, C=case_c, D=case_d)


def run_case(name):
    ds, (dets, labels, img_index), kw = CASES[name]()
    cat_ids = [c['id'] for c in ds['categories']]
    img_ids = [im['id'] for im in ds['images']]
    return ds, (dets, labels, img_index), cat_ids, img_ids, kw


def seeded_dataset(seed=0, n_img=48, n_cat=5):
    """48 images x 5 categories (ids unsorted on purpose) that reach every corner of the definition: scores quantised to
    1/64, boxes on an 8-pixel grid (equal IoUs, IoUs of exactly 0.5 and 0.75), crowd gts, an `ignore` field without
    iscrowd (which COCOeval overwrites), areas of exactly 32^2 and 96^2, images without gts / dets / both, category 3
    without gts, category 4 without dets, and one problem of 1 003 detections (cut at maxDets[-1] = 1000)."""
    rng = np.random.default_rng(seed)
    img_ids = [int(v) for v in rng.permutation(np.arange(100, 100 + n_img))]
    cat_ids = [7, 3, 11, 5, 2][:n_cat]
    anns, rows = [], []
    aid = 1

    def grid_box(lo=0, hi=560, smin=8, smax=200):
        x, y = rng.integers(lo // 8, hi // 8, 2) * 8
        w, h = rng.integers(smin // 8, smax // 8 + 1, 2) * 8
        return float(x), float(y), float(w), float(h)
    for ii, img in enumerate(img_ids):
        no_gt, no_dt = ii % 11 == 3 or ii % 13 == 5, ii % 7 == 2 or ii % 13 == 5
        for lab, cat in enumerate(cat_ids):
            boxes = []
            if not no_gt and lab != 3:
                for _ in range(int(rng.integers(0, 5))):
                    b = grid_box()
                    kind = rng.integers(0, 10)
                    if kind >= 8 and boxes:                        # a duplicate gt: equal IoUs, the later one wins
                        b = boxes[-1]
                    elif kind == 0:
                        b = (b[0], b[1], 32.0, 32.0)
                    elif kind == 1:
                        b = (b[0], b[1], 96.0, 96.0)
                    extra = dict(ignore=1) if rng.integers(0, 6) == 0 else {}
                    anns.append(_ann(aid, img, cat, b, iscrowd=int(rng.integers(0, 5) == 0), **extra))
                    aid += 1
                    boxes.append(b)
            if no_dt or lab == 4:
                continue
            for _ in range(int(rng.integers(0, 9))):
                score = int(rng.integers(1, 65)) / 64.0
                if boxes and rng.integers(0, 3) > 0:
                    x, y, w, h = boxes[int(rng.integers(0, len(boxes)))]
                    kind = rng.integers(0, 6)
                    if kind == 0:                                  # the gt itself
                        pass
                    elif kind == 1:                                # half of it: IoU 0.5 (crowd: 1)
                        w = w / 2
                    elif kind == 2 and w % 32 == 0:                # three quarters: IoU 0.75
                        w = w * 3 / 4
                    elif kind == 3:                                # inside, shifted
                        x, w = x + 8, max(w - 8, 8)
                    else:                                          # shifted by a grid step
                        x, y = x + 8 * int(rng.integers(-2, 3)), y + 8 * int(rng.integers(-2, 3))
                else:
                    x, y, w, h = grid_box()
                    if rng.integers(0, 8) == 0:
                        w = h = 32.0
                rows.append((ii, lab, x, y, x + w, y + h, score))
    # one crowded problem: 1 003 detections over two gts (image 0, label 0)
    img0 = img_ids[0]
    anns.append(_ann(aid, img0, cat_ids[0], (0.0, 0.0, 64.0, 64.0)))
    anns.append(_ann(aid + 1, img0, cat_ids[0], (320.0, 320.0, 128.0, 128.0), iscrowd=1))
    for n in range(1003):
        x, y = float(8 * (n % 50)), float(8 * (n // 50 % 50))
        rows.append((0, 0, x, y, x + 64.0, y + 64.0, int(rng.integers(1, 65)) / 64.0))
    order = rng.permutation(len(rows))                             # the flat table in no particular order
    ds = _dataset(img_ids, cat_ids, anns)
    return ds, _flat([rows[j] for j in order]), cat_ids, img_ids
