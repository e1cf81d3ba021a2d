"""Shared helpers of the VOC-style mAP tests: synthetic datasets, and reading tests/golden/map_eval.npz back."""
import numpy as np

SCALE_RANGES = [(0, 32), (32, 96), (96, 1e5)]
#: the fixture's evaluation cases: name -> eval_map keyword arguments ('empty' runs on the dataset without detections)
CASES = dict(thr50=dict(iou_thr=0.5),
             thr70_scales=dict(iou_thr=0.7, scale_ranges=SCALE_RANGES),
             voc07=dict(iou_thr=0.5, dataset='voc07'),
             det=dict(iou_thr=0.5, dataset='det'),
             empty=dict(iou_thr=0.5))
#: cases whose per-(image, class) tp / fp flags the fixture stores as well
TPFP_CASES = ('thr50', 'thr70_scales', 'det')


def boxes(rng, n, scale=400., max_side=160.):
    xy = rng.uniform(0, scale, (n, 2))
    wh = rng.uniform(2, max_side, (n, 2)) * rng.choice([0.15, 0.5, 1.0], (n, 1))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _f(rows, cols=4):
    return np.array(rows, np.float32).reshape(-1, cols)


def synth_dataset(rng, num_img, num_cls, distinct_scores=True, crafted=True):
    """Detections that are noisy copies of the gts (three qualities: several detections per gt) plus clutter; ignored
    gts on two images of three (the third has no ignore keys at all); every 7th image without gts, every 11th without
    detections; the last class never occurs among the gts.  ``crafted`` appends four hand-made images (see below).
    ``distinct_scores``: scores drawn without replacement per class; otherwise rounded to two decimals (ties)."""
    dets, annos = [], []
    for i in range(num_img):
        ng = int(rng.integers(0, 9)) if i % 7 else 0
        gb = boxes(rng, ng)
        gl = rng.integers(0, num_cls - 1, ng)
        ign = rng.random(ng) < 0.2
        anno = dict(bboxes=gb[~ign], labels=gl[~ign].astype(np.int64))
        if i % 3:
            anno.update(bboxes_ignore=gb[ign], labels_ignore=gl[ign].astype(np.int64))
        per_cls = []
        for c in range(num_cls):
            mine = gb[gl == c]
            reps = [mine + rng.normal(0, s, mine.shape).astype(np.float32) for s in (1.0, 6.0, 20.0)]
            cand = np.concatenate(reps + [boxes(rng, int(rng.integers(0, 4)))], 0)
            cand = cand[rng.random(len(cand)) < 0.8]
            if i % 11 == 3:
                cand = cand[:0]
            per_cls.append(cand.astype(np.float32))
        dets.append(per_cls)
        annos.append(anno)
    if crafted:
        empty = [np.zeros((0, 4), np.float32) for _ in range(num_cls)]

        def image(cls_boxes, **anno):
            per_cls = list(empty)
            for c, b in cls_boxes.items():
                per_cls[c] = _f(b)
            dets.append(per_cls)
            annos.append({k: (_f(v) if k.startswith('bboxes') else np.array(v, np.int64)) for k, v in anno.items()})
        # IoU exactly float32(0.7): 70 / ((70 + 100) - 70)
        image({0: [[0, 0, 10, 7]]}, bboxes=[[0, 0, 10, 10]], labels=[0])
        # two gts tied for the first detection's maximum (0.6 each: the first one is its argmax); the second detection
        # prefers the second gt
        image({1: [[25, 20, 45, 40], [31, 20, 50, 40]]}, bboxes=[[20, 20, 40, 40], [30, 20, 50, 40]], labels=[1, 1])
        # best gt ignored (0.9896) while the regular gt passes too (0.96); a second detection on the regular gt
        image({2: [[100, 100, 200, 192], [100, 102, 200, 200]]}, bboxes=[[100, 100, 200, 200]], labels=[2],
              bboxes_ignore=[[100, 100, 200, 190]], labels_ignore=[2])
        # areas exactly on the 32^2 and 96^2 bounds: an unmatched detection, a matched pair
        image({0: [[300, 300, 332, 332], [0, 100, 96, 196]]}, bboxes=[[0, 100, 96, 196]], labels=[0])
    # scores
    for c in range(num_cls):
        n = sum(len(d[c]) for d in dets)
        if distinct_scores:
            sc = (rng.choice(20000, size=n, replace=False) / 20000).astype(np.float32)
            assert len(np.unique(sc)) == n
        else:
            sc = np.round(rng.random(n), 2).astype(np.float32)
        lo = 0
        for d in dets:
            m = len(d[c])
            d[c] = np.concatenate([d[c], sc[lo:lo + m, None]], 1).astype(np.float32)
            lo += m
    return dets, annos


def without_detections(dets):
    return [[np.zeros((0, 5), np.float32) for _ in per_cls] for per_cls in dets]


def store_dataset(out, dets, annos):
    out['ds/num_img'], out['ds/num_cls'] = np.int64(len(dets)), np.int64(len(dets[0]))
    for i, (det, anno) in enumerate(zip(dets, annos)):
        for c, d in enumerate(det):
            out[f'ds/det/{i}/{c}'] = d
        for k, v in anno.items():
            out[f'ds/{k}/{i}'] = v


def load_dataset(z):
    ni, nc = int(z['ds/num_img']), int(z['ds/num_cls'])
    dets = [[z[f'ds/det/{i}/{c}'] for c in range(nc)] for i in range(ni)]
    annos = [{k: z[f'ds/{k}/{i}'] for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore')
              if f'ds/{k}/{i}' in z.files} for i in range(ni)]
    return dets, annos


def store_result(out, name, mean_ap, results):
    out[f'{name}/mean_ap'] = np.asarray(mean_ap, np.float64)
    out[f'{name}/num_gts'] = np.array([r['num_gts'] for r in results], np.int64)
    out[f'{name}/num_dets'] = np.array([r['num_dets'] for r in results], np.int64)
    out[f'{name}/ap'] = np.array([r['ap'] for r in results])
    for c, r in enumerate(results):
        out[f'{name}/recall/{c}'], out[f'{name}/precision/{c}'] = r['recall'], r['precision']


def assert_result_equals_fixture(z, name, mean_ap, results):
    """Bit for bit, dtypes included."""
    got = {}
    store_result(got, name, mean_ap, results)
    keys = [k for k in z.files if k.startswith(name + '/') and not k.startswith(name + '/tpfp/')]
    assert sorted(keys) == sorted(got), (sorted(keys), sorted(got))
    for k in keys:
        assert got[k].dtype == z[k].dtype and got[k].shape == z[k].shape, (k, got[k].dtype, z[k].dtype, got[k].shape, z[k].shape)
        np.testing.assert_array_equal(got[k], z[k], err_msg=k)
    for r in results:
        assert r['recall'].dtype == np.float64 and r['precision'].dtype == np.float32
        assert np.asarray(r['ap']).dtype == np.float32


def class_major_problems(dets, annos):
    """(class, image, detections, gts, ignored gts) in the order the fixture's tp / fp flags are concatenated."""
    import _map_ref as R
    for c in range(len(dets[0])):
        for i, (d, g, ign) in enumerate(R.class_problem(dets, annos, c)):
            yield c, i, d, g, ign
