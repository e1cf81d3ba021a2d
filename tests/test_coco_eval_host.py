"""COCO bbox evaluation, host side (no GPU): the numpy restatement (tests/_cocoeval_ref.py) against hand-computed
values, the float64 xyxy -> xywh rule, the CocoGt loader, the list and flat result forms, evaluate_bbox's keys, rounding
and errors on stubbed stats, and the argument validation of the C-ABI calls."""
import ctypes
import json
import logging

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import coco_eval as CE
import _cocoeval_ref as R


def near(x, want):
    """pr = tp / (fp + tp + 2^-52) is within 2^-52 (relative) of the hand value tp / (fp + tp), and np.mean sums up to
    1 010 such values pairwise (~log2(1010) * 2^-53 relative): 2e-15 covers both."""
    return bool(np.all(np.abs(np.asarray(x, np.float64) - want) <= 2e-15))


def _run(name):
    ds, (dets, labels, img_index), cat_ids, img_ids, kw = R.run_case(name)
    return R.coco_eval(ds, dets, labels, img_index, cat_ids, img_ids, **kw)


def test_case_a_two_gts_one_false_positive_between():
    res = _run('A')
    want = (51 + 100 / 3) / 101
    assert want == 0.8349834983498351
    s = res['stats']
    assert near(s[0:3], want) and near(s[5], want)
    assert s[3] == -1 and s[4] == -1
    assert (s[6:9] == 1).all() and s[9] == -1 and s[10] == -1 and s[11] == 1
    # the envelope: 1 up to recall 0.5, then 2/3
    np.testing.assert_array_equal(res['precision'][0, :51, 0, 0, 2], 1 / (1 + np.spacing(1)))
    np.testing.assert_array_equal(res['precision'][0, 51:, 0, 0, 2], 2 / (1 + 2 + np.spacing(1)))
    np.testing.assert_array_equal(res['scores'][0, :51, 0, 0, 2], np.float64(np.float32(.9)))
    np.testing.assert_array_equal(res['scores'][0, 51:, 0, 0, 2], np.float64(np.float32(.7)))
    np.testing.assert_array_equal(res['counts'], [[2, 0, 0, 2]])


def test_case_b_detections_inside_a_crowd_are_ignored():
    res = _run('B')
    s = res['stats']
    assert near(s[[0, 1, 2, 5]], 1) and s[8] == 1 and s[11] == 1
    one = 1 / (1 + np.spacing(1))                                  # a perfect precision, as pycocotools divides it
    assert (res['precision'][:, :, 0, [0, 3]] == one).all() and (res['recall'][:, 0, [0, 3]] == 1).all()
    assert (res['precision'][:, :, 0, [1, 2]] == -1).all()
    assert res['events']['crowd_rematch'] > 0
    b = res['bits']
    # rank 0 and 1 (inside the crowd): matched and ignored at every threshold; rank 2: matched, counted
    assert b['matched'][0].all() and b['ignored'][0][:, :2].all() and not b['ignored'][0][:, 2].any()
    np.testing.assert_array_equal(res['counts'], [[1, 0, 0, 1]])


def test_case_c_a_category_without_gts_stays_minus_one():
    res = _run('C')
    assert (res['precision'][:, :, 1] == -1).all() and (res['recall'][:, 1] == -1).all()
    assert (res['precision'][:, :, 0, 0] == 1 / (1 + np.spacing(1))).all()
    assert near(res['stats'][0], 1) and res['stats'][8] == 1


def test_case_d_max_dets_cut_and_the_literal_100():
    res = _run('D')
    s = res['stats']
    assert s[0] == -1                                            # no entry of maxDets equals 100
    assert near(s[1], 1 / 3)
    assert s[6] == 0 and s[7] == 1 and s[8] == 1
    np.testing.assert_array_equal(res['precision'][:, :, 0, 0, 0], 0.0)
    assert res['events']['search_past_end'] > 0


def test_xyxy_to_xywh_subtracts_in_float64():
    b = np.array([0.1, 0.3, 100.7, 50.9, 0.5], np.float32)
    w64 = float(b[2]) - float(b[0])
    assert w64 != float(b[2] - b[0])                              # the float32 subtraction rounds differently
    assert R.det_box(b) == [float(b[0]), float(b[1]), w64, float(b[3]) - float(b[1])]


def _dataset_with_ignore():
    ds = R._dataset([9, 4], [5, 2], [R._ann(1, 9, 5, (0, 0, 10, 10), ignore=1), R._ann(2, 4, 2, (0, 0, 20, 20), iscrowd=1),
                                     R._ann(3, 9, 5, (5, 5, 10, 10), area=77.5), R._ann(4, 4, 5, (1, 1, 4, 4))])
    return ds


def test_coco_gt_loader(tmp_path):
    ds = _dataset_with_ignore()
    path = tmp_path / 'ann.json'
    path.write_text(json.dumps(ds))
    for src in (ds, str(path)):
        gt = pkg.CocoGt(src)
        assert gt.get_img_ids() == [9, 4] and gt.get_cat_ids() == [5, 2]
        assert gt.get_cat_ids(cat_names=['c2']) == [2] and gt.load_cats([2])[0]['name'] == 'c2'
        np.testing.assert_array_equal(gt.ann_ignore, [0, 1, 0, 0])     # 'ignore' is overwritten by iscrowd
        np.testing.assert_array_equal(gt.ann_area, [100, 400, 77.5, 16])
        assert gt.ann_box.dtype == np.float64
    ev = pkg.COCOeval(gt, ([np.zeros((0, 5), np.float32)] * 2,) * 2)
    tab = ev.tables()
    assert list(tab['img_ids']) == [4, 9] and list(tab['cat_ids']) == [2, 5]         # sorted
    assert list(ev.params.imgIds) == [4, 9]
    # problems (image 4: cat 2, cat 5; image 9: cat 2, cat 5); annotation order inside (9, 5)
    np.testing.assert_array_equal(tab['gt_off'], [0, 1, 2, 2, 4])
    np.testing.assert_array_equal(tab['gt_area'], [400, 16, 100, 77.5])
    np.testing.assert_array_equal(tab['gt_flag'], [3, 0, 0, 0])
    np.testing.assert_array_equal(tab['kmap'], [1, 0])
    np.testing.assert_array_equal(tab['imap'], [1, 0])
    ev.params.catIds = [5]
    tab = ev.tables()
    np.testing.assert_array_equal(tab['gt_off'], [0, 1, 3])
    np.testing.assert_array_equal(tab['kmap'], [0, -1])


def test_list_and_flat_results_give_the_same_tables():
    rng = np.random.default_rng(0)
    results = [[rng.random((int(n), 5)).astype(np.float32) for n in rng.integers(0, 4, 3)] for _ in range(5)]
    results[2] = [np.zeros((0, 5), np.float32)] * 3
    dets, labels, img_index = CE.flatten_results(results)
    rows = [(i, c, r) for i, res in enumerate(results) for c, a in enumerate(res) for r in a]
    np.testing.assert_array_equal(dets, np.array([r for _, _, r in rows]))
    np.testing.assert_array_equal(labels, [c for _, c, _ in rows])
    np.testing.assert_array_equal(img_index, [i for i, _, _ in rows])
    gt = pkg.CocoGt(R._dataset(range(5), range(3), []))
    a = pkg.COCOeval(gt, results).flat_results()
    b = pkg.COCOeval(gt, (dets, labels.astype(np.int32), img_index)).flat_results()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
        assert x.dtype == y.dtype


class _Stub(CE.COCOeval):
    def evaluate(self):
        pass

    def accumulate(self):
        prec = -np.ones((10, 101, 2, 4, 3))
        prec[:, :, 1, 0, -1] = 0.25
        self.eval = dict(precision=prec)

    def summarize(self, out=print):
        self.stats = np.array([0.12345, 0.5, 0.75, -1, 0.3336, 0.9995, 0.1, 0.2, 0.3, -1, 0.4, 0.5])


def test_evaluate_bbox_keys_rounding_and_errors(monkeypatch):
    monkeypatch.setattr(CE, 'COCOeval', _Stub)
    gt = pkg.CocoGt(R._dataset([1], [1, 2], []))
    results = [[np.ones((1, 5), np.float32), np.zeros((0, 5), np.float32)]]
    out = pkg.evaluate_bbox(results, gt, logger='silent')
    assert list(out) == ['bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m', 'bbox_mAP_l',
                         'bbox_mAP_copypaste']
    assert out['bbox_mAP'] == 0.123 and out['bbox_mAP_s'] == -1.0 and out['bbox_mAP_m'] == 0.334 and out['bbox_mAP_l'] == 1.0
    assert out['bbox_mAP_copypaste'] == '0.123 0.500 0.750 -1.000 0.334 1.000'
    out = pkg.evaluate_bbox(results, gt, logger='silent', metric_items=['AR@100', 'mAP_50'], metric=['bbox'])
    assert list(out) == ['bbox_AR@100', 'bbox_mAP_50', 'bbox_mAP_copypaste'] and out['bbox_AR@100'] == 0.1
    assert pkg.evaluate_bbox(results, gt, logger='silent', metric_items='AR_l@1000')['bbox_AR_l@1000'] == 0.5
    with pytest.raises(KeyError, match='metric item mAP50 is not supported'):
        pkg.evaluate_bbox(results, gt, logger='silent', metric_items=['mAP50'])
    with pytest.raises(KeyError, match='metric mAP is not supported'):
        pkg.evaluate_bbox(results, gt, metric='mAP')
    for m in ('segm', 'proposal', 'proposal_fast'):
        with pytest.raises(NotImplementedError, match='no detector of this package'):
            pkg.evaluate_bbox(results, gt, metric=m)
    # classwise: idx runs over cat_ids as given; category 2 sits at K index 1
    lines = []
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    log = logging.getLogger('coco_eval_host_test')
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    pkg.evaluate_bbox(results, gt, logger=log, classwise=True)
    table = [ln for ln in lines if 'category' in ln][0]
    assert 'c1' in table and 'nan' in table and 'c2' in table and '0.250' in table
    # empty results: the reference's message, an empty dict
    del lines[:]
    empty = [[np.zeros((0, 5), np.float32)] * 2]
    assert pkg.evaluate_bbox(empty, gt, logger=log) == {}
    assert 'The testing results of the whole dataset is empty.' in lines
    assert pkg.evaluate_bbox((np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)), gt, logger=log) == {}


def test_unbuilt_variants_raise():
    gt = pkg.CocoGt(R._dataset([1], [1], []))
    with pytest.raises(NotImplementedError, match='segm'):
        pkg.COCOeval(gt, [], iou_type='segm')
    ev = pkg.COCOeval(gt, [[np.zeros((0, 5), np.float32)]])
    ev.params.useCats = 0
    with pytest.raises(NotImplementedError, match='useCats=0'):
        ev.evaluate()
    with pytest.raises(RuntimeError, match='evaluate'):
        pkg.COCOeval(gt, []).accumulate()


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    ds, flat, cat_ids, img_ids, _ = R.run_case('A')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.COCOeval(pkg.CocoGt(ds), flat).evaluate()


def test_seeded_dataset_reaches_every_corner():
    """A condition on the INPUTS of the GPU comparison: every event counter of the restatement is positive."""
    ds, (dets, labels, img_index), cat_ids, img_ids = R.seeded_dataset()
    res = R.coco_eval(ds, dets, labels, img_index, cat_ids, img_ids)
    assert set(res['events']) == set(R.EVENTS)
    for name, n in res['events'].items():
        assert n > 0, (name, res['events'])
    assert (res['counts'][res['cat_ids'].index(5)] == 0).all()          # label 3: no gt anywhere
    assert (res['recall'][:, res['cat_ids'].index(2)][..., -1] <= 0).all()   # label 4: no det anywhere


def test_c_abi_argument_validation():
    L = pkg._lib
    lib = L.lib()
    assert L.FEATURES['coco_eval'].symbols <= set(L.SIGNATURES) and L.has('coco_eval')
    one = ctypes.c_void_p(256)
    assert lib.yv4_coco_rank(None, None, 0, 0, 100, 40, one, one, one, one, one, one, None) == -1
    assert b'problem table' in lib.yv4_last_error()
    assert lib.yv4_coco_rank(None, None, 1 << 31, 1, 100, 40, one, one, one, one, one, one, None) == -1
    assert b'2^31' in lib.yv4_last_error()
    assert lib.yv4_coco_rank(None, None, 4, 1, 0, 40, one, one, one, one, one, one, None) == -1
    assert b'maxDets' in lib.yv4_last_error()
    assert lib.yv4_coco_match(None, None, one, None, None, None, one, 6, 4, 0, 100, one, 10, one, 4, None, 0, one, None,
                              one, None) == -1 and b'problem table' in lib.yv4_last_error()       # P % K != 0
    assert lib.yv4_coco_match(None, None, one, None, None, None, one, 4, 4, 0, 100, None, 10, one, 4, None, 0, one, None,
                              one, None) == -1 and b'thresholds' in lib.yv4_last_error()
    assert lib.yv4_coco_match(None, None, one, None, None, None, one, 4, 4, 0, 100, one, 10, one, 65, None, 0, one, None,
                              one, None) == -1 and b'area ranges' in lib.yv4_last_error()
    assert lib.yv4_coco_match(None, None, one, None, None, None, one, 4, 4, 3, 100, one, 10, one, 4, None, 0, one, None,
                              one, None) == -1 and b'null detection' in lib.yv4_last_error()
    md = (ctypes.c_int32 * 3)(100, 300, 1000)
    assert lib.yv4_coco_accumulate(None, None, None, one, None, one, 4, 4, 0, md, 17, 10, 4, one, 101, one, one, one, one,
                                   None) == -1 and b'maxDets' in lib.yv4_last_error()
    assert lib.yv4_coco_accumulate(None, None, None, one, None, one, 4, 4, 0, md, 3, 10, 4, one, 300, one, one, one, one,
                                   None) == -1 and b'recall thresholds' in lib.yv4_last_error()
    assert lib.yv4_coco_accumulate_work(-1, 4, 40) == 0
    assert lib.yv4_coco_accumulate_work(1000, 4, 40) >= 2 * 8000 + 4 * 4000 + 40 * 1000
    assert lib.yv4_coco_rank_work(1000) >= 2 * 8000 + 4000 + 1024
