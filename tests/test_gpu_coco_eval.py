"""COCO bbox evaluation on the MI355X against the numpy restatement (tests/_cocoeval_ref.py).  Every comparison is exact
equality of precision / recall / scores, the gt counts, the per-detection matched / ignored bits and stats.  That is
derived, not measured: every device operation is a single IEEE float64 operation (or an integer one) in the
restatement's order, compiled without contraction; np.mean in summarize runs on the host in both."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import coco_eval as CE
from conftest import state_dict_from
import _cocoeval_ref as R

pytestmark = pytest.mark.gpu


def run_pkg(ds, results, cat_ids, img_ids, iou_thrs=None, max_dets=(100, 300, 1000)):
    ev = pkg.COCOeval(pkg.CocoGt(ds), results, 'bbox', cat_ids=cat_ids, img_ids=img_ids)
    ev.params.maxDets = list(max_dets)
    if iou_thrs is not None:
        ev.params.iouThrs = np.asarray(iou_thrs, dtype=np.float64)
    ev.evaluate()
    bits = ev.det_bits()
    ev.accumulate()
    ev.summarize(out=lambda line: None)
    return ev, bits


def assert_equal(ev, bits, ref):
    for key in ('index', 'problem', 'rank', 'matched', 'ignored'):
        np.testing.assert_array_equal(bits[key], ref['bits'][key], err_msg=key)
    np.testing.assert_array_equal(ev.eval['counts'], ref['counts'])
    for key in ('recall', 'precision', 'scores'):
        assert ev.eval[key].dtype == np.float64 and ev.eval[key].shape == ref[key].shape
        np.testing.assert_array_equal(ev.eval[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(ev.stats, ref['stats'])


def check(ds, flat, cat_ids, img_ids, **kw):
    ref = R.coco_eval(ds, *flat, cat_ids, img_ids, **kw)
    ev, bits = run_pkg(ds, flat, cat_ids, img_ids, **kw)
    assert_equal(ev, bits, ref)
    return ev, ref


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_hand_cases_through_the_kernels(gpu_device, name):
    ds, flat, cat_ids, img_ids, kw = R.run_case(name)
    check(ds, flat, cat_ids, img_ids, **kw)


@pytest.fixture(scope='module')
def seeded():
    return R.seeded_dataset()


@pytest.mark.parametrize('kw', [dict(), dict(iou_thrs=[0.3, 0.5, 0.75], max_dets=(1, 10, 100))], ids=['default', 'custom'])
def test_seeded_dataset(gpu_device, seeded, kw):
    ds, flat, cat_ids, img_ids = seeded
    ref = R.coco_eval(ds, *flat, cat_ids, img_ids, **kw)
    if not kw:
        for name, n in ref['events'].items():                        # a condition on the inputs
            assert n > 0, (name, ref['events'])
    ev, bits = run_pkg(ds, flat, cat_ids, img_ids, **kw)
    assert_equal(ev, bits, ref)
    # a subset of the categories and images in params, as a caller may set them
    sub = dict(params_cat_ids=cat_ids[1:4], params_img_ids=img_ids[::2])
    ref = R.coco_eval(ds, *flat, cat_ids, img_ids, **kw, **sub)
    e2 = pkg.COCOeval(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids)
    e2.params.catIds, e2.params.imgIds = sub['params_cat_ids'], sub['params_img_ids']
    e2.params.maxDets = list(kw.get('max_dets', (100, 300, 1000)))
    if 'iou_thrs' in kw:
        e2.params.iouThrs = np.asarray(kw['iou_thrs'], np.float64)
    e2.evaluate()
    b2 = e2.det_bits()
    e2.accumulate()
    e2.summarize(out=lambda line: None)
    assert_equal(e2, b2, ref)


def _boxes(rng, n, grid=False):
    xy = rng.integers(0, 400, (n, 2)).astype(np.float64)
    wh = rng.integers(8, 160, (n, 2)).astype(np.float64)
    if not grid:
        xy, wh = xy + rng.random((n, 2)), wh + rng.random((n, 2))
    return np.concatenate([xy, wh], 1)


def _problem_dataset(shapes, seed, ties=True, crowds=True):
    """One image per (D, G) pair, one category: G gts, D detections of which min(D, G) sit near a gt."""
    rng = np.random.default_rng(seed)
    anns, rows, aid = [], [], 1
    for i, (D, G) in enumerate(shapes):
        g = _boxes(rng, G, grid=True)
        for b in g:
            anns.append(R._ann(aid, i, 1, [float(v) for v in b], iscrowd=int(crowds and rng.integers(0, 12) == 0)))
            aid += 1
        d = _boxes(rng, D)
        n = min(D, G)
        d[:n] = g[rng.permutation(G)[:n]] + rng.normal(0, 3, (n, 4))
        d[:, 2:] = np.maximum(d[:, 2:], 1.0)
        s = rng.integers(1, 257, D) / 256.0 if ties else rng.random(D)
        rows += [(i, 0, b[0], b[1], b[0] + b[2], b[1] + b[3], sc) for b, sc in zip(d, s)]
    return R._dataset(range(len(shapes)), [1], anns), R._flat(rows), [1], list(range(len(shapes)))


def test_more_detections_than_max_dets(gpu_device):
    """D = 1 001 against maxDets[-1] = 1 000, G = 1: the lowest-ranked detection takes no part."""
    ds, flat, cat_ids, img_ids = _problem_dataset([(1001, 1)], 1, ties=False, crowds=False)
    ev, ref = check(ds, flat, cat_ids, img_ids)
    assert ref['events']['problems_cut'] == 1 and len(ref['bits']['index']) == 1000


def test_iou_block_beyond_lds_takes_the_workspace(gpu_device):
    """D = 3, G = 700: 2 100 doubles, beyond the 2 048 that sit in LDS."""
    ds, flat, cat_ids, img_ids = _problem_dataset([(3, 700)], 2)
    check(ds, flat, cat_ids, img_ids, iou_thrs=[0.5, 0.75])


def test_wave_sized_problems(gpu_device):
    shapes = [(63, 2), (64, 3), (65, 1), (2, 63), (3, 64), (1, 65), (64, 64), (65, 65), (0, 64), (64, 0), (33, 513)]
    ds, flat, cat_ids, img_ids = _problem_dataset(shapes, 3)
    check(ds, flat, cat_ids, img_ids, iou_thrs=[0.5, 0.55, 0.75])


def test_one_category_of_70000_detections(gpu_device):
    """700 images x 100 detections of one category: the sorts cross 69 tiles and the scan 1 094 chunks; every score of
    the odd images is the same, so half of the global order is decided by (image, rank) alone."""
    rng = np.random.default_rng(4)
    n_img, per = 700, 100
    gts = _boxes(rng, n_img, grid=True)
    anns = [R._ann(i + 1, i, 1, [float(v) for v in gts[i]]) for i in range(n_img)]
    b = _boxes(rng, n_img * per)
    b[::per] = gts + rng.normal(0, 2, (n_img, 4))
    b[:, 2:] = np.maximum(b[:, 2:], 1.0)
    img = np.repeat(np.arange(n_img), per)
    score = rng.integers(1, 1025, n_img * per) / 1024.0
    score[img % 2 == 1] = 0.5
    dets = np.concatenate([b[:, :2], b[:, :2] + b[:, 2:], score[:, None]], 1).astype(np.float32)
    perm = rng.permutation(len(dets))
    flat = (dets[perm], np.zeros(len(dets), np.int64), img[perm])
    ds = R._dataset(range(n_img), [1], anns)
    check(ds, flat, [1], list(range(n_img)), iou_thrs=[0.5, 0.75])


def test_more_than_65535_problems_take_the_64_bit_sort(gpu_device):
    """1 000 images x 70 categories = 70 000 problems: the problem index no longer fits the 16 key bits of the 6-pass
    sort, so yv4_coco_rank sorts all 64 bits (the shape of a real dataset: 5 000 x 80).  Sparse: 400 detections and
    150 gts, tied scores, image and category ids unsorted."""
    rng = np.random.default_rng(5)
    n_img, n_cat = 1000, 70
    img_ids = [int(v) for v in rng.permutation(n_img) + 10]
    cat_ids = [int(v) for v in rng.permutation(n_cat) + 1]
    gi, gc = rng.integers(0, n_img, 150), rng.integers(0, n_cat, 150)
    gb = _boxes(rng, 150, grid=True)
    anns = [R._ann(j + 1, img_ids[gi[j]], cat_ids[gc[j]], [float(v) for v in gb[j]], iscrowd=int(j % 17 == 0))
            for j in range(150)]
    src = rng.integers(0, 150, 400)
    b = gb[src] + rng.normal(0, 4, (400, 4))
    b[:, 2:] = np.maximum(b[:, 2:], 1.0)
    di, dc = gi[src].copy(), gc[src].copy()
    stray = rng.random(400) < 0.3                                   # detections in problems without gts
    di[stray], dc[stray] = rng.integers(0, n_img, int(stray.sum())), rng.integers(0, n_cat, int(stray.sum()))
    di[:3], dc[:3] = n_img - 1, n_cat - 1                           # the last problem of the table is occupied
    score = rng.integers(1, 17, 400) / 16.0
    dets = np.concatenate([b[:, :2], b[:, :2] + b[:, 2:], score[:, None]], 1).astype(np.float32)
    ds = R._dataset(img_ids, cat_ids, anns)
    ev, ref = check(ds, (dets, dc.astype(np.int64), di.astype(np.int64)), cat_ids, img_ids, iou_thrs=[0.5, 0.75])
    assert ev.eval['precision'].shape[2] * len(img_ids) >= 65535 and (ref['counts'] > 0).any()


def _as_list_form(flat, n_img, n_cls):
    dets, labels, img_index = flat
    return [[dets[(img_index == i) & (labels == c)] for c in range(n_cls)] for i in range(n_img)]


def test_result_forms_and_repeatability(gpu_device, seeded):
    ds, flat, cat_ids, img_ids = seeded
    results = _as_list_form(flat, len(img_ids), len(cat_ids))
    flat_np = CE.flatten_results(results)
    flat_gpu = tuple(torch.from_numpy(a).to(gpu_device) for a in flat_np)
    runs = [run_pkg(ds, r, cat_ids, img_ids) for r in (results, flat_np, flat_gpu, flat_gpu)]
    ref = R.coco_eval(ds, *flat_np, cat_ids, img_ids)
    assert_equal(*runs[0], ref)
    e0, b0 = runs[0]
    for e, b in runs[1:]:
        for key in ('precision', 'recall', 'scores', 'counts'):
            assert e.eval[key].tobytes() == e0.eval[key].tobytes(), key
        for key in b0:
            assert b[key].tobytes() == b0[key].tobytes(), key
        assert e.stats.tobytes() == e0.stats.tobytes()


def test_empty_and_foreign_detections(gpu_device):
    """No detection at all, and detections whose label or image lies outside the tables: recall 0, precision 0 where a
    category has gts; nothing faults."""
    ds, flat, cat_ids, img_ids, _ = R.run_case('A')
    none = (np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    ev, ref = check(ds, none, cat_ids, img_ids)
    assert (ev.eval['recall'][:, 0, 0] == 0).all() and (ev.eval['precision'][:, :, 0, 0] == 0).all()
    dets, labels, img_index = flat
    foreign = (np.concatenate([dets, dets]), np.concatenate([labels, labels + 5]), np.concatenate([img_index, img_index]))
    ev2, _ = run_pkg(ds, foreign, cat_ids, img_ids)
    want = R.coco_eval(ds, *flat, cat_ids, img_ids)
    np.testing.assert_array_equal(ev2.eval['precision'], want['precision'])
    np.testing.assert_array_equal(ev2.stats, want['stats'])


def test_tiny_detector_through_single_gpu_test_and_evaluate_bbox(golden, gpu_device, capsys):
    g = golden('tiny_v4')
    stages = [str(s) for s in g['meta_stages']]
    reps = [None if r < 0 else int(r) for r in g['meta_reps']]
    chans = [int(c) for c in g['meta_channels']]
    neck_out = [int(c) for c in g['meta_neck_out']]
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[stages, reps, chans], out_indices=[int(i) for i in g['meta_out_indices']]),
        neck=dict(type='YOLOV4Neck', in_channels=[int(c) for c in g['meta_neck_in']], out_channels=neck_out,
                  csp_repetition=int(g['meta_csp_rep'])),
        bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=neck_out), train_cfg=None,
        test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65),
                      max_per_img=300)))
    det.load_state_dict(state_dict_from(g), strict=True)
    det = det.eval().to(gpu_device)
    metas = [dict(scale_factor=g['scale_factors'][i]) for i in range(2)]
    results = pkg.single_gpu_test(det, [dict(img=torch.from_numpy(g['img']), img_metas=metas)])
    assert len(results) == 2 and len(results[0]) == 80
    # hand-made gts: a few of the reference's own detections (whole pixels), one of them a crowd, one elsewhere
    cat_ids, img_ids = list(range(1, 81)), [17, 5]
    anns, aid = [], 1
    for n in range(2):
        rd, rl = g[f'dets{n}'], g[f'labels{n}']
        for j in range(0, min(len(rd), 40), 5):
            x1, y1, x2, y2 = [float(np.round(v)) for v in rd[j, :4]]
            anns.append(R._ann(aid, img_ids[n], cat_ids[int(rl[j])], (x1, y1, max(x2 - x1, 1.0), max(y2 - y1, 1.0)),
                               iscrowd=int(j == 10)))
            aid += 1
        anns.append(R._ann(aid, img_ids[n], 3, (1.0, 2.0, 30.0, 20.0)))
        aid += 1
    ds = R._dataset(img_ids, cat_ids, anns)
    got = pkg.evaluate_bbox(results, ds, logger='silent', classwise=True)
    printed = capsys.readouterr().out
    assert printed.count('Average Precision') == 6 and printed.count('Average Recall') == 6
    assert ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ' in printed
    ref = R.coco_eval(ds, *CE.flatten_results(results), cat_ids, img_ids)
    assert got == R.evaluate_bbox(ref)
    assert sum(map(len, results[0])) + sum(map(len, results[1])) > 0 and ref['counts'].sum() > 0
    flat = tuple(torch.from_numpy(a).to(gpu_device) for a in CE.flatten_results(results))
    assert pkg.evaluate_bbox(flat, ds, logger='silent', metric_items=['AR@1000']) == R.evaluate_bbox(ref, ['AR@1000'])
