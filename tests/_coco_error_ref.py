"""The reference's COCO error analysis (tools/analysis_tools/coco_error_analysis.py:173-304, iou_type='bbox') restated
literally on tests/_cocoeval_ref.py: the per-category loop, the deep copy and relabelling of the annotations, the
detections filtered to the category, the stacking, the ``== -1`` / ``> 0`` / ``1.0`` steps and makeplot's means.  Host only;
1 + 2 K runs of ``R.coco_eval``.  The GPU tests hold the one-pass kernel to it bit for bit, tests/test_coco_error_host.py
holds IT to hand-computed values.

Two stated differences from the reference's tool, the package's own: the K axis is the sorted category ids (what
COCOeval uses; the tool indexes by file order), and a category without ``supercategory`` shares it with nobody (the
tool raises KeyError).

``events`` is a second, direct walk with the origin of every ground truth kept, which only COUNTS the corner cases a
test input must contain; it decides nothing about the expected values."""
import contextlib
import copy

import numpy as np

import _cocoeval_ref as R

TYPES = ('C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN')


def area_ranges(areas):
    return [[0 ** 2, areas[2]], [0 ** 2, areas[0]], [areas[0], areas[1]], [areas[1], areas[2]]]


@contextlib.contextmanager
def _area_rng(areas):
    """``cocoEval.params.areaRng = ...``: R reads its module constant, swapped for the duration of the call."""
    keep = R.AREA_RNG
    if areas:
        R.AREA_RNG = area_ranges(areas)
    try:
        yield
    finally:
        R.AREA_RNG = keep


def child_cat_ids(dataset, cat_id):
    """``gt.getCatIds(supNms=[nm['supercategory']])``."""
    cats = {c['id']: c for c in dataset['categories']}
    nm = cats.get(cat_id, {})
    if 'supercategory' not in nm:
        return [cat_id] if cat_id in cats else []
    return [c['id'] for c in dataset['categories'] if c.get('supercategory', object()) == nm['supercategory']]


def relabelled(dataset, cat_id, which):
    """The deep copy of the annotation file with the annotations of ``which`` ('sim': c's supercategory, 'oth': every
    category) that are not c turned into ignored crowds of c."""
    gt = copy.deepcopy(dataset)
    child = child_cat_ids(dataset, cat_id)
    for idx, ann in enumerate(gt['annotations']):
        hit = ann['category_id'] in child if which == 'sim' else True
        if hit and ann['category_id'] != cat_id:
            gt['annotations'][idx]['ignore'] = 1
            gt['annotations'][idx]['iscrowd'] = 1
            gt['annotations'][idx]['category_id'] = cat_id
    return gt


def error_analysis(dataset, dets, labels, img_index, cat_ids, img_ids, areas=None, iou_thrs=(0.75, 0.5, 0.1), conf_thr=0.1,
                   max_det=100):
    """-> ``ps`` (T + 4, R, K, A, 1), ``counts`` (K, A), ``bits`` (matched / ignored (A, T + 2, n) in (problem, rank)
    order, Sim at T and Oth at T + 1), ``cat_ids`` (sorted) and the per-run counts."""
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    labels, img_index = np.asarray(labels, np.int64).reshape(-1), np.asarray(img_index, np.int64).reshape(-1)
    md = (max_det, max_det, max_det)              # R.summarize reads max_dets[2]; the three columns are identical
    T = len(iou_thrs)
    with _area_rng(areas):
        base = R.coco_eval(dataset, dets, labels, img_index, cat_ids, img_ids, iou_thrs=list(iou_thrs), max_dets=md)
        ps = base['precision'][..., :1]
        ps = np.vstack([ps, np.zeros((4, *ps.shape[1:]))])
        catIds = base['cat_ids']
        K = len(catIds)
        bb = base['bits']
        n = len(bb['index'])
        A = bb['matched'].shape[0]
        matched, ignored = np.zeros((A, T + 2, n), bool), np.zeros((A, T + 2, n), bool)
        matched[:, :T], ignored[:, :T] = bb['matched'], bb['ignored']
        det_cat = np.array([cat_ids[int(v)] if 0 <= v < len(cat_ids) else None for v in labels], dtype=object)
        counts_run = {}
        for k, catId in enumerate(catIds):
            sel = np.flatnonzero(det_cat == catId)             # dt.dataset['annotations'] of this category only
            pos = np.flatnonzero(bb['problem'] % K == k)
            for row, which in ((T, 'sim'), (T + 1, 'oth')):
                gt = relabelled(dataset, catId, which)
                res = R.coco_eval(gt, dets[sel], labels[sel], img_index[sel], cat_ids, img_ids, iou_thrs=[conf_thr],
                                  max_dets=md)
                ps[row, :, k, :, :] = res['precision'][0, :, k, :, :1]
                rb = res['bits']
                assert np.array_equal(sel[rb['index']], bb['index'][pos]) and np.array_equal(rb['problem'], bb['problem'][pos])
                matched[:, row, pos], ignored[:, row, pos] = rb['matched'][:, 0], rb['ignored'][:, 0]
                counts_run[which, k] = res['counts'][k]
            ps[ps == -1] = 0
            ps[T + 2, :, k, :, :] = ps[T + 1, :, k, :, :] > 0
            ps[T + 3, :, k, :, :] = 1.0
    return dict(ps=ps, counts=base['counts'], cat_ids=catIds, counts_run=counts_run, rec_thrs=np.linspace(0, 1, 101),
                bits=dict(index=bb['index'], problem=bb['problem'], rank=bb['rank'], matched=matched, ignored=ignored))


def aps(ps, k=None):
    """makeplot's ``aps`` for every area range -> (T + 4, A): ``ps[:, :, k]`` of a class, or all of ``ps``."""
    ps = ps if k is None else ps[:, :, k]
    out = []
    for i in range(ps.shape[-2]):
        area_ps = ps[..., i, 0]
        out.append([ps_.mean() for ps_ in area_ps])
    return np.array(out, dtype=np.float64).T


# ---- the corner cases an input contains ------------------------------------------------------------------------------
EVENTS = ('foreign_match_sim', 'foreign_match_oth_only', 'foreign_rematch', 'stop_rule_before_foreign',
          'equal_iou_own_ignored_then_foreign', 'equal_iou_foreign_then_own_ignored', 'own_crowd_beside_foreign',
          'iou_equals_conf_thr', 'category_without_gt', 'category_without_det', 'image_without_gt')


def events(dataset, dets, labels, img_index, cat_ids, img_ids, conf_thr=0.1, max_det=100):
    """Counters over the Sim and Oth walks in the area range 'all' of the default areas."""
    ev = dict.fromkeys(EVENTS, 0)
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    imgIds, catIds = [int(i) for i in np.unique(img_ids)], [int(c) for c in np.unique(cat_ids)]
    per_img = {i: [] for i in imgIds}
    for ann in dataset['annotations']:
        if ann['image_id'] in per_img:
            per_img[ann['image_id']].append(ann)
    dts = {}
    for n in range(len(dets)):
        dts.setdefault((int(img_ids[int(img_index[n])]), int(cat_ids[int(labels[n])])), []).append(n)
    gt_cats = {a['category_id'] for a in dataset['annotations']}
    ev['category_without_gt'] = sum(c not in gt_cats for c in catIds)
    ev['category_without_det'] = sum(not any(k[1] == c for k in dts) for c in catIds)
    ev['image_without_gt'] = sum(not per_img[i] for i in imgIds)
    thr = min(conf_thr, 1 - 1e-10)
    for (img, cat), rows in dts.items():
        if img not in per_img or cat not in catIds:
            continue
        rows = [rows[j] for j in np.argsort([-float(dets[n, 4]) for n in rows], kind='mergesort')][:max_det]
        child = child_cat_ids(dataset, cat)
        foreign_of = {}
        for mode in ('sim', 'oth'):
            gts = []
            for ann in per_img[img]:
                own = ann['category_id'] == cat
                if own or mode == 'oth' or ann['category_id'] in child:
                    crowd = bool(ann.get('iscrowd', 0)) if own else True
                    gts.append(dict(box=[float(v) for v in ann['bbox']], own=own, crowd=crowd, ig=crowd))
            gts = [gts[j] for j in np.argsort([g['ig'] for g in gts], kind='mergesort')]
            if mode == 'oth' and any(g['own'] and g['crowd'] for g in gts) and any(not g['own'] for g in gts):
                ev['own_crowd_beside_foreign'] += 1
            taken = [0] * len(gts)
            for n in rows:
                row = [R.iou_pair(R.det_box(dets[n]), g['box'], g['crowd']) for g in gts]
                if mode == 'oth':
                    ev['iou_equals_conf_thr'] += sum(v == conf_thr and not g['own'] for v, g in zip(row, gts))
                best, m = thr, -1
                for gi, g in enumerate(gts):
                    if taken[gi] and not g['crowd']:
                        continue
                    if m > -1 and not gts[m]['ig'] and g['ig']:
                        if gts[m]['own'] and any(not h['own'] and v >= thr for h, v in zip(gts[gi:], row[gi:])):
                            ev['stop_rule_before_foreign'] += 1
                        break
                    if row[gi] < best:
                        continue
                    if m > -1 and row[gi] == best and gts[m]['ig'] and g['ig']:
                        if gts[m]['own'] and not g['own']:
                            ev['equal_iou_own_ignored_then_foreign'] += 1
                        if not gts[m]['own'] and g['own']:
                            ev['equal_iou_foreign_then_own_ignored'] += 1
                    best, m = row[gi], gi
                foreign = m > -1 and not gts[m]['own']
                if foreign:
                    if taken[m]:
                        ev['foreign_rematch'] += 1
                    taken[m] += 1
                elif m > -1:
                    taken[m] += 1
                if mode == 'sim':
                    foreign_of[n] = foreign
                    ev['foreign_match_sim'] += foreign
                elif foreign and not foreign_of[n]:
                    ev['foreign_match_oth_only'] += 1
    return ev


# ---- the shared cases of the host and GPU tests ----------------------------------------------------------------------
SUPER5 = {7: 'a', 3: 'a', 11: 'b', 5: 'b', 2: 'a'}


def with_supercategories(dataset, sup=SUPER5):
    """``R.seeded_dataset()``'s annotation file with a supercategory on every category."""
    ds = copy.deepcopy(dataset)
    for c in ds['categories']:
        if c['id'] in sup:
            c['supercategory'] = sup[c['id']]
    return ds


def hand_case():
    """One image, categories 1 (A) and 2 (B) in supercategory 'x', 3 (C) in 'y', one gt each; four detections of A: on
    B's gt, on C's gt, on nothing, and with IoU 0.3 on A's own gt."""
    ds = R._dataset([1], [1, 2, 3], [R._ann(1, 1, 1, (0, 0, 100, 100)), R._ann(2, 1, 2, (200, 200, 100, 100)),
                                    R._ann(3, 1, 3, (400, 400, 100, 100))])
    for c, s in zip(ds['categories'], 'xxy'):
        c['supercategory'] = s
    flat = R._flat([(0, 0, 200, 200, 300, 300, .9), (0, 0, 400, 400, 500, 500, .8), (0, 0, 0, 300, 50, 350, .7),
                    (0, 0, 0, 0, 100, 30, .6)])
    return ds, flat, [1, 2, 3], [1]


def confusion_dataset(seed=3, n_img=20):
    """A seeded set made for the confusion walks: six categories (ids unsorted) in two supercategories plus one without
    a supercategory, annotations of a category the file does not list, boxes on an 8-pixel grid.  Detections sit on gts
    of ANY category of the image (exactly, on a half, shifted, or overlapping a tenth of their own area: a confusion IoU
    of exactly 0.1), own crowd gts are duplicated as foreign gts before and after them (equal IoUs in both annotation
    orders), category 5 has no gts, category 2 no detections, some images no gts."""
    rng = np.random.default_rng(seed)
    img_ids = [int(v) for v in rng.permutation(np.arange(500, 500 + n_img))]
    cat_ids = [7, 3, 11, 5, 2, 9]
    sup = {7: 'a', 3: 'a', 11: 'b', 5: 'b', 2: 'a'}
    anns, rows, aid = [], [], 1

    def grid_box():
        x, y = rng.integers(0, 60, 2) * 8
        w, h = rng.integers(2, 20, 2) * 8
        return float(x), float(y), float(w), float(h)
    for ii, img in enumerate(img_ids):
        boxes = []                                         # (box, category) of the image, in annotation order
        if ii % 7 != 4:
            for _ in range(int(rng.integers(2, 9))):
                cat = [7, 3, 11, 2, 9, 42][int(rng.integers(0, 6))]
                b = grid_box()
                kind = int(rng.integers(0, 8))
                crowd = int(rng.integers(0, 4) == 0)
                if kind <= 1 and boxes:                    # the same box again under another category, either order
                    b, other = boxes[int(rng.integers(0, len(boxes)))]
                    cat = [c for c in (7, 3, 11) if c != other][int(rng.integers(0, 2))]
                    crowd = int(kind == 0)
                anns.append(R._ann(aid, img, cat, b, iscrowd=crowd))
                aid += 1
                boxes.append((b, cat))
                if crowd and rng.integers(0, 2):           # an own crowd gt followed by its foreign twin
                    cat2 = [c for c in (7, 3, 11) if c != cat][int(rng.integers(0, 2))]
                    anns.append(R._ann(aid, img, cat2, b))
                    aid += 1
                    boxes.append((b, cat2))
        if ii % 5 == 3:
            continue
        for lab, cat in enumerate(cat_ids):
            if cat == 2:
                continue
            for _ in range(int(rng.integers(0, 7))):
                score = int(rng.integers(1, 33)) / 32.0
                if boxes and rng.integers(0, 5) > 0:
                    (x, y, w, h), _c = boxes[int(rng.integers(0, len(boxes)))]
                    kind = int(rng.integers(0, 6))
                    if kind == 1:
                        w = w / 2
                    elif kind == 2:                        # ten columns wide, one of them on the gt: inter / area = 0.1
                        x, w = x + w - 8, 80.0
                    elif kind == 3:
                        x, w = x + 8, max(w - 8, 8)
                    elif kind >= 4:
                        x, y = x + 8 * int(rng.integers(-2, 3)), y + 8 * int(rng.integers(-2, 3))
                else:
                    x, y, w, h = grid_box()
                rows.append((ii, lab, x, y, x + w, y + h, score))
    order = rng.permutation(len(rows))
    ds = R._dataset(img_ids, cat_ids, anns)
    for c in ds['categories']:
        if c['id'] in sup:
            c['supercategory'] = sup[c['id']]
    return ds, R._flat([rows[j] for j in order]), cat_ids, img_ids
