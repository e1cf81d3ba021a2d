"""VOC-style mAP on the GPU: bbox_overlaps / tpfp_default / tpfp_imagenet / eval_map / evaluate_map through the C ABI
(yv4_bbox_overlaps_batched, yv4_tpfp_batched) against the reference-made fixture (tests/golden/map_eval.npz) and, where
the fixture does not reach (score ties, odd shapes), against the numpy restatement tests/_map_ref.py, which
tests/test_map_host.py holds against the same fixture.  Tolerance: none -- every comparison is exact, dtypes included.
Ties: both sides order them with this host's np.argsort(-scores)."""
import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib as L
from mmdet_yolov4_amd import map_eval as ME
import _map_ref as R
from _map_data import (CASES, SCALE_RANGES, TPFP_CASES, assert_result_equals_fixture, boxes, class_major_problems,
                       load_dataset, synth_dataset, without_detections)

pytestmark = pytest.mark.gpu

AREAS3 = [(lo ** 2, hi ** 2) for lo, hi in SCALE_RANGES]
E4 = np.zeros((0, 4), np.float32)


@pytest.fixture(scope='module')
def z(golden):
    return golden('map_eval')


@pytest.fixture(scope='module')
def data(z):
    return load_dataset(z)


def _same_results(got, want):
    (ma, ra), (mb, rb) = got, want
    assert type(ma) is type(mb) and np.array_equal(np.asarray(ma), np.asarray(mb)), (ma, mb)
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        assert a.keys() == b.keys()
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), k


def _tpfp_both(det, gt, ign, thr, area_ranges):
    """Both rules of one problem, package against restatement, exact."""
    for mine, ref in ((pkg.tpfp_default, R.tpfp_default), (pkg.tpfp_imagenet, R.tpfp_imagenet)):
        tp, fp = mine(det, gt, ign, thr, area_ranges)
        rtp, rfp = ref(det, gt, ign, thr, area_ranges)
        assert tp.dtype == np.float32 and tp.shape == rtp.shape and fp.shape == rfp.shape
        np.testing.assert_array_equal(tp, rtp)
        np.testing.assert_array_equal(fp, rfp)
    return tp, fp


def _random_problem(rng, nd, ng, nign, round_scores=True):
    gt, ign = boxes(rng, ng), boxes(rng, nign)
    allg = np.concatenate([gt, ign])
    det = boxes(rng, nd)
    if len(allg):
        src = allg[rng.integers(0, len(allg), nd)]
        near = rng.random(nd) < 0.7
        det[near] = (src + rng.normal(0, 6, src.shape).astype(np.float32))[near]
    sc = rng.random(nd)
    sc = np.round(sc, 2) if round_scores else sc
    return np.concatenate([det, sc[:, None]], 1).astype(np.float32), gt, ign


# ---- against the reference-made fixture ----------------------------------------------------------------------------------
def test_bbox_overlaps_against_fixture(z):
    for k in range(int(z['ov/n'])):
        a, b = z[f'ov{k}/b1'], z[f'ov{k}/b2']
        for key, kw in (('iou', {}), ('iof', dict(mode='iof')), ('iou_eps1e-3', dict(eps=1e-3))):
            got = pkg.bbox_overlaps(a, b, **kw)
            assert got.dtype == np.float32 and got.shape == (len(a), len(b))
            np.testing.assert_array_equal(got, z[f'ov{k}/{key}'], err_msg=f'ov{k}/{key}')


def test_bbox_overlaps_swap_changes_no_bit():
    """The reference swaps its operands for rows > cols; the kernel does not.  Both orientations of the same pairs are
    the transpose of one another, bit for bit, and equal the restatement."""
    rng = np.random.default_rng(3)
    a, b = boxes(rng, 700), boxes(rng, 70)
    b[:70] = a[:70] + rng.normal(0, 5, (70, 4)).astype(np.float32)
    ab, ba = pkg.bbox_overlaps(a, b), pkg.bbox_overlaps(b, a)
    np.testing.assert_array_equal(ab, ba.T)
    np.testing.assert_array_equal(ab, R.overlaps(a, b))
    np.testing.assert_array_equal(pkg.bbox_overlaps(a, b, 'iof'), R.overlaps(a, b, 'iof'))
    np.testing.assert_array_equal(pkg.bbox_overlaps(b, a, 'iof'), R.overlaps(b, a, 'iof'))
    assert pkg.bbox_overlaps(a[:0], b).shape == (0, 70) and pkg.bbox_overlaps(a, b[:0]).shape == (700, 0)
    np.testing.assert_array_equal(pkg.bbox_overlaps(np.concatenate([a, a[:, :1]], 1), b), ab)    # (n, 5) detections


@pytest.mark.parametrize('name', TPFP_CASES)
def test_tpfp_ops_against_fixture(z, data, name):
    dets, annos = data
    kw = CASES[name]
    fn = pkg.tpfp_imagenet if kw.get('dataset') == 'det' else pkg.tpfp_default
    sr = kw.get('scale_ranges')
    area_ranges = None if sr is None else [(lo ** 2, hi ** 2) for lo, hi in sr]
    want_tp, want_fp = z[f'{name}/tpfp/tp'], z[f'{name}/tpfp/fp']
    lo = 0
    for n, (c, i, d, g, ign) in enumerate(class_major_problems(dets, annos)):
        if n % 3 == 0 or i >= 60:                                 # a third of the problems and every hand-made image
            tp, fp = fn(d, g, ign, kw['iou_thr'], area_ranges)
            assert tp.dtype == np.float32 and fp.dtype == np.float32
            np.testing.assert_array_equal(tp, want_tp[:, lo:lo + len(d)], err_msg=f'{name} class {c} image {i}')
            np.testing.assert_array_equal(fp, want_fp[:, lo:lo + len(d)], err_msg=f'{name} class {c} image {i}')
        lo += len(d)
    assert lo == want_tp.shape[1]


@pytest.mark.parametrize('name', list(CASES))
def test_eval_map_against_fixture(z, data, name):
    dets, annos = data
    mean_ap, results = pkg.eval_map(without_detections(dets) if name == 'empty' else dets, annos, logger='silent',
                                    **CASES[name])
    assert_result_equals_fixture(z, name, mean_ap, results)


def test_threshold_pair_matches_at_float32_0_7():
    det, gt = np.array([[0, 0, 10, 7, .9]], np.float32), np.array([[0, 0, 10, 10]], np.float32)
    assert pkg.bbox_overlaps(det, gt)[0, 0] == np.float32(0.7)
    tp, fp = pkg.tpfp_default(det, gt, E4, 0.7)
    assert tp.tolist() == [[1.0]] and fp.tolist() == [[0.0]]
    tp, fp = pkg.tpfp_default(det, gt, E4, 0.7000001)
    assert tp.tolist() == [[0.0]] and fp.tolist() == [[1.0]]


# ---- against the restatement: ties everywhere -------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(iou_thr=0.5), dict(iou_thr=0.6, scale_ranges=SCALE_RANGES), dict(iou_thr=0.5, dataset='voc07'),
                                dict(iou_thr=0.5, dataset='vid'), dict(iou_thr=0.4, dataset='det', scale_ranges=SCALE_RANGES)],
                         ids=['default', 'scales', 'voc07', 'vid', 'det-scales'])
def test_eval_map_with_tied_scores_against_restatement(kw):
    dets, annos = synth_dataset(np.random.default_rng(77), 40, 5, distinct_scores=False)
    sc = np.concatenate([d[0][:, 4] for d in dets])
    assert len(np.unique(sc)) < len(sc)
    _same_results(pkg.eval_map(dets, annos, logger='silent', **kw), R.eval_map(dets, annos, **kw))


def test_tied_ious_and_tied_scores_per_problem():
    """IoU matrices with many exact ties (boxes on a coarse grid) under tied scores, both rules, K = 1 and 3."""
    rng = np.random.default_rng(5)
    for it in range(12):
        nd, ng, ni = int(rng.integers(1, 40)), int(rng.integers(1, 9)), int(rng.integers(0, 4))
        det, gt, ign = _random_problem(rng, nd, ng, ni)
        det[:, :4], gt, ign = np.round(det[:, :4] / 16) * 16, np.round(gt / 16) * 16, np.round(ign / 16) * 16
        _tpfp_both(det, gt, ign, [0.3, 0.5, 0.75][it % 3], AREAS3 if it % 2 else None)


def test_five_thresholds_in_one_call_equal_five_calls(data):
    dets, annos = data
    thrs = [0.3, 0.5, 0.6, 0.7, 0.9]
    for kw in (dict(), dict(scale_ranges=SCALE_RANGES), dict(dataset='det')):
        many = pkg.eval_map(dets, annos, iou_thr=thrs, logger='silent', **kw)
        assert isinstance(many, list) and len(many) == 5
        for thr, got in zip(thrs, many):
            _same_results(got, pkg.eval_map(dets, annos, iou_thr=thr, logger='silent', **kw))
    _same_results(many[1], R.eval_map(dets, annos, iou_thr=0.5, dataset='det'))


def test_evaluate_map_returns_the_loop_of_custom_dataset_evaluate(data):
    dets, annos = data
    thrs = [0.5, 0.7, 0.75]
    got = pkg.evaluate_map(dets, annos, classes=[f'c{i}' for i in range(6)], iou_thr=thrs, logger='silent')
    want, mean_aps = {}, []
    for thr in thrs:                                              # datasets/custom.py:313-325
        mean_ap, _ = R.eval_map(dets, annos, iou_thr=thr)
        mean_aps.append(mean_ap)
        want[f'AP{int(thr * 100):02d}'] = round(mean_ap, 3)
    want['mAP'] = sum(mean_aps) / len(mean_aps)
    assert list(got.items()) == list(want.items()) and list(got) == ['AP50', 'AP70', 'AP75', 'mAP']
    single = pkg.evaluate_map(dets, annos, iou_thr=0.5, logger='silent')
    assert list(single) == ['AP50', 'mAP'] and single['mAP'] == mean_aps[0]


# ---- shapes where the thread maps can break ------------------------------------------------------------------------------------
def test_degenerate_shapes():
    rng = np.random.default_rng(9)
    det, gt, ign = _random_problem(rng, 7, 3, 2)
    for ar in (None, AREAS3):
        K = 1 if ar is None else 3
        for fn in (pkg.tpfp_default, pkg.tpfp_imagenet):
            tp, fp = fn(det[:0], gt, ign, 0.5, ar)                # nd == 0
            assert tp.shape == (K, 0) and fp.shape == (K, 0) and tp.dtype == np.float32
        _tpfp_both(det, E4, E4, 0.5, ar)                          # ng == 0: every in-range detection is a false positive
        _tpfp_both(det, E4, None, 0.5, ar)
        tp, fp = _tpfp_both(det, E4, ign, 0.5, ar)                # only ignored gts
        assert tp.sum() == 0
        _tpfp_both(det[:1], gt[:1], E4, 0.5, ar)                  # 1 x 1
        _tpfp_both(np.concatenate([gt[:1], [[0.5]]], 1).astype(np.float32), gt[:1], E4, 0.5, ar)
    tp, fp = pkg.tpfp_default(det, E4, E4, 0.5)
    assert tp.sum() == 0 and fp.sum() == 7


def test_one_large_problem_700_by_70():
    """More than one workgroup of detections and of pairs, rows > cols, both rules, five thresholds at once."""
    rng = np.random.default_rng(21)
    det, gt, ign = _random_problem(rng, 700, 60, 10)
    ann = dict(bboxes=gt, labels=np.zeros(60, np.int64), bboxes_ignore=ign, labels_ignore=np.zeros(10, np.int64))
    thrs = [0.1, 0.3, 0.5, 0.7, 0.9]
    tab = ME.MapTables([[det]], [ann]).sort()
    for mode, ref in ((L.TPFP_DEFAULT, R.tpfp_default), (L.TPFP_IMAGENET, R.tpfp_imagenet)):
        tp, fp = ME.tpfp_batched(tab, mode, thrs, AREAS3)
        assert tp.shape == (5, 3, 700) and tp.dtype == np.uint8
        for t, thr in enumerate(thrs):
            rtp, rfp = ref(det, gt, ign, thr, AREAS3)
            np.testing.assert_array_equal(tp[t], rtp)
            np.testing.assert_array_equal(fp[t], rfp)
        assert tp.sum() > 0 and fp.sum() > 0


def test_3000_one_detection_problems():
    """The problem lookup across many workgroups: 3 000 images x 1 class, one detection each, 0-2 gts."""
    rng = np.random.default_rng(33)
    dets, annos = [], []
    for i in range(3000):
        g = boxes(rng, i % 3)
        d = (g[:1] + rng.normal(0, 4, (1, 4)).astype(np.float32)) if len(g) and i % 5 else boxes(rng, 1)
        dets.append([np.concatenate([d, [[np.round(rng.random(), 2)]]], 1).astype(np.float32)])
        annos.append(dict(bboxes=g, labels=np.zeros(len(g), np.int64)))
    for kw in (dict(iou_thr=0.5), dict(iou_thr=0.5, dataset='det', scale_ranges=SCALE_RANGES)):
        _same_results(pkg.eval_map(dets, annos, logger='silent', **kw), R.eval_map(dets, annos, **kw))


def test_all_detections_on_one_gt_contend_for_one_minimum():
    rng = np.random.default_rng(41)
    gt = np.array([[100, 100, 220, 200], [400, 400, 420, 420]], np.float32)
    det = gt[:1] + rng.normal(0, 3, (600, 4)).astype(np.float32)
    det = np.concatenate([det, np.round(rng.random((600, 1)), 2)], 1).astype(np.float32)
    for thr in (0.5, 0.9):
        tp, fp = _tpfp_both(det, gt, E4, thr, None)
    tp, fp = pkg.tpfp_default(det, gt, E4, 0.5)
    assert tp.sum() == 1 and tp[0, np.argsort(-det[:, 4])[0]] == 1 and fp.sum() == 599


def test_detection_exactly_on_an_area_bound():
    """K = 3: areas 32*32 and 96*96 belong to the range they open, not the one they close."""
    det = np.array([[0, 0, 32, 32, .9], [50, 50, 146, 146, .8], [200, 200, 231, 232, .7]], np.float32)
    gt = np.array([[50, 50, 146, 146]], np.float32)
    tp, fp = _tpfp_both(det, gt, E4, 0.5, AREAS3)
    assert fp.tolist() == [[0, 0, 1], [1, 0, 0], [0, 0, 0]] and tp.tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 0]]
    tp, fp = _tpfp_both(det, E4, E4, 0.5, AREAS3)
    assert fp.tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]


def test_two_runs_give_identical_bytes():
    dets, annos = synth_dataset(np.random.default_rng(78), 30, 4, distinct_scores=False)
    tab = ME.MapTables(dets, annos).sort()
    for mode in (L.TPFP_DEFAULT, L.TPFP_IMAGENET):
        a = ME.tpfp_batched(tab, mode, [0.3, 0.5, 0.7], AREAS3)
        b = ME.tpfp_batched(tab, mode, [0.3, 0.5, 0.7], AREAS3)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    r1 = pkg.eval_map(dets, annos, iou_thr=[0.5, 0.75], logger='silent')
    r2 = pkg.eval_map(dets, annos, iou_thr=[0.5, 0.75], logger='silent')
    for x, y in zip(r1, r2):
        _same_results(x, y)
