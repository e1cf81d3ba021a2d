"""VOC-style mAP without a GPU: the numpy restatement (tests/_map_ref.py) against the reference's outputs in
tests/golden/map_eval.npz, bit for bit and with exact dtypes; the package's host side (tables, sorting, accumulation,
custom tpfp callables, misuse) and the argument validation of the new C-ABI calls."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _map_ref as R  # noqa: E402
from _map_data import (CASES, TPFP_CASES, assert_result_equals_fixture, class_major_problems, load_dataset,  # noqa: E402
                       without_detections)

import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd import map_eval as ME  # noqa: E402


@pytest.fixture(scope='module')
def z(golden):
    return golden('map_eval')


@pytest.fixture(scope='module')
def data(z):
    return load_dataset(z)


def _area_ranges(kw):
    sr = kw.get('scale_ranges')
    return None if sr is None else [(lo ** 2, hi ** 2) for lo, hi in sr]


def test_fixture_holds_what_the_issue_lists(z, data):
    dets, annos = data
    assert len(dets) >= 60 and len(dets[0]) == 6
    for c in range(6):                                           # scores pairwise distinct within every class
        sc = np.concatenate([d[c][:, 4] for d in dets])
        assert len(np.unique(sc)) == len(sc)
    assert any(len(a['bboxes']) == 0 for a in annos) and any(all(len(d) == 0 for d in per) for per in dets)
    assert any('labels_ignore' in a and len(a['labels_ignore']) for a in annos) and any('labels_ignore' not in a for a in annos)
    assert not any((a['labels'] == 5).any() for a in annos) and sum(len(d[5]) for d in dets) > 0
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'map_eval.npz')) < 1 << 20


def test_restated_overlaps_equal_the_reference(z):
    for k in range(int(z['ov/n'])):
        a, b = z[f'ov{k}/b1'], z[f'ov{k}/b2']
        for key, kw in (('iou', {}), ('iof', dict(mode='iof')), ('iou_eps1e-3', dict(eps=1e-3))):
            got = R.overlaps(a, b, **kw)
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, z[f'ov{k}/{key}'], err_msg=f'ov{k}/{key}')
    # rows > cols is among them, and the eps clamp is hit (0 / eps, and a union below eps)
    assert any(len(z[f'ov{k}/b1']) > len(z[f'ov{k}/b2']) for k in range(int(z['ov/n'])))
    assert z['ov4/iou'][0, 0] == 0 and 0 < z['ov4/iou'][2, 2] < 0.5 and z['ov4/iou'][3, 3] == 1


@pytest.mark.parametrize('name', TPFP_CASES)
def test_restated_tpfp_rules_equal_the_reference_per_problem(z, data, name):
    dets, annos = data
    kw = CASES[name]
    rule = R.tpfp_imagenet if kw.get('dataset') == 'det' else R.tpfp_default
    flags = [rule(d, g, ign, kw['iou_thr'], _area_ranges(kw)) for _, _, d, g, ign in class_major_problems(dets, annos)]
    assert all(f[0].dtype == np.float32 and f[1].dtype == np.float32 for f in flags)
    np.testing.assert_array_equal(np.concatenate([f[0] for f in flags], axis=1), z[f'{name}/tpfp/tp'])
    np.testing.assert_array_equal(np.concatenate([f[1] for f in flags], axis=1), z[f'{name}/tpfp/fp'])


@pytest.mark.parametrize('name', list(CASES))
def test_restated_eval_map_equals_the_reference(z, data, name):
    dets, annos = data
    mean_ap, results = R.eval_map(without_detections(dets) if name == 'empty' else dets, annos, **CASES[name])
    assert_result_equals_fixture(z, name, mean_ap, results)


def test_iou_equal_to_the_threshold_matches_in_float32():
    """gt [0,0,10,10] / det [0,0,10,7]: IoU is float32(0.7) exactly.  numpy 2 compares it with the Python float 0.7 in
    float32 (a match); in float64 float32(0.7) < 0.7."""
    det, gt = np.array([[0, 0, 10, 7, .9]], np.float32), np.array([[0, 0, 10, 10]], np.float32)
    iou = R.overlaps(det, gt)[0, 0]
    assert iou == np.float32(0.7) and iou >= 0.7 and not float(iou) >= 0.7
    tp, fp = R.tpfp_default(det, gt, None, 0.7)
    assert tp.tolist() == [[1.0]] and fp.tolist() == [[0.0]]
    tp, fp = R.tpfp_default(det, gt, None, 0.7000001)
    assert tp.tolist() == [[0.0]] and fp.tolist() == [[1.0]]


# ---- the package's host side ---------------------------------------------------------------------------------------------
def test_tables_are_class_major_and_ranks_invert_the_order(data):
    dets, annos = data
    tab = ME.MapTables(dets, annos).sort()
    probs = list(class_major_problems(dets, annos))
    assert len(probs) == len(tab.nd)
    for p, (c, i, d, g, ign) in enumerate(probs):
        np.testing.assert_array_equal(tab.det[tab.det_off[p]:tab.det_off[p + 1]], d.reshape(-1, 5))
        np.testing.assert_array_equal(tab.gt[tab.gt_off[p]:tab.gt_off[p + 1]], np.concatenate([g, ign]))
        np.testing.assert_array_equal(tab.gt_ignore[tab.gt_off[p]:tab.gt_off[p + 1]], [0] * len(g) + [1] * len(ign))
        order = tab.order[tab.det_off[p]:tab.det_off[p + 1]]
        np.testing.assert_array_equal(order, np.argsort(-d[:, 4]))
        np.testing.assert_array_equal(tab.rank[tab.det_off[p]:tab.det_off[p + 1]][order], np.arange(len(d)))


@pytest.mark.parametrize('name', TPFP_CASES)
def test_host_accumulation_reproduces_the_reference_from_its_flags(z, data, name):
    """The fixture's tp / fp flags through the package's own accumulation (and average_precision): every array of the
    case bit for bit -- float64 recall, float32 precision and ap."""
    dets, annos = data
    kw = CASES[name]
    tab = ME.MapTables(dets, annos).sort()
    area = ME._area_table(_area_ranges(kw))
    mean_ap, results = ME.accumulate(tab, z[f'{name}/tpfp/tp'], z[f'{name}/tpfp/fp'], ME._num_gts(tab, area),
                                     kw.get('scale_ranges'), kw.get('dataset'))
    assert_result_equals_fixture(z, name, mean_ap, results)


def test_average_precision_reproduces_the_reference_on_its_dtypes(z):
    for name in CASES:
        mode = '11points' if name == 'voc07' else 'area'
        for c in range(6):
            r, p = z[f'{name}/recall/{c}'], z[f'{name}/precision/{c}']
            ap = pkg.average_precision(r, p, mode)
            assert np.asarray(ap).dtype == np.float32
            np.testing.assert_array_equal(ap, z[f'{name}/ap'][c])


def test_custom_tpfp_callable_is_called_per_problem_on_the_host(z, data):
    dets, annos = data
    calls = []

    def rule(d, g, ign, thr, area_ranges):
        calls.append(thr)
        return R.tpfp_default(d, g, ign, thr, area_ranges)
    mean_ap, results = pkg.eval_map(dets, annos, iou_thr=0.5, tpfp_fn=rule, logger='silent')
    assert len(calls) == len(dets) * 6
    assert_result_equals_fixture(z, 'thr50', mean_ap, results)
    with pytest.raises(ValueError, match='tpfp_fn has to be a function'):
        pkg.eval_map(dets, annos, tpfp_fn='default', logger='silent')


def test_entry_points_raise_without_a_gpu(data, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    dets, annos = data
    b = np.array([[0, 0, 10, 10]], np.float32)
    d = np.array([[0, 0, 10, 7, .9]], np.float32)
    for call in (lambda: pkg.eval_map(dets, annos, logger='silent'),
                 lambda: pkg.eval_map(dets, annos, iou_thr=[0.5, 0.75], dataset='det', logger='silent'),
                 lambda: pkg.evaluate_map(dets, annos, logger='silent'),
                 lambda: pkg.bbox_overlaps(b, b),
                 lambda: pkg.tpfp_default(d, b),
                 lambda: pkg.tpfp_imagenet(d, b, np.zeros((0, 4), np.float32))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_recall_metric_is_refused_by_name(data):
    dets, annos = data
    with pytest.raises(NotImplementedError, match='RPN proposals'):
        pkg.evaluate_map(dets, annos, metric='recall')
    with pytest.raises(NotImplementedError, match='RPN proposals'):
        pkg.evaluate_map(dets, annos, metric=['recall'])
    with pytest.raises(KeyError, match='not supported'):
        pkg.evaluate_map(dets, annos, metric='bbox')


def test_summary_table_is_silent_on_request(z, data, capsys):
    dets, annos = data
    mean_ap, results = R.eval_map(dets, annos, iou_thr=0.5)
    pkg.print_map_summary(mean_ap, results, logger='silent')
    assert capsys.readouterr().out == ''
    pkg.print_map_summary(mean_ap, results, dataset=[f'c{i}' for i in range(6)])
    out = capsys.readouterr().out
    assert '| class' in out and '| c5 ' in out and f'{mean_ap:.3f}' in out and out.count('\n') >= 11
    mean_ap, results = R.eval_map(dets, annos, iou_thr=0.7, scale_ranges=CASES['thr70_scales']['scale_ranges'])
    pkg.print_map_summary(mean_ap, results, scale_ranges=[(0, 1024), (1024, 9216), (9216, 1e10)])
    assert capsys.readouterr().out.count('Scale range') == 3


def test_more_than_2_24_detections_per_class_are_refused():
    tab = ME.MapTables([[np.zeros((0, 5), np.float32)]], [dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64))])
    tab.det_off = np.array([0, 2 ** 24], np.int64)
    with pytest.raises(ValueError, match=r'2\*\*24'):
        ME.accumulate(tab, None, None, np.zeros((1, 1), int), None, None)


# ---- the C-ABI calls reject bad arguments before touching the device --------------------------------------------------------
def test_new_symbols_are_bound_and_validate_their_arguments():
    L = pkg._lib
    assert L.FEATURES['map_eval'].symbols <= set(L.SIGNATURES) and L.has('map_eval')
    lib = L.lib()
    one = ctypes.c_void_p(16)                                    # a non-null, 16-byte aligned placeholder: never read
    assert lib.yv4_bbox_overlaps_batched(None, None, None, None, None, 1, 0, 0, 1e-6, None, None) == -1
    assert b'problem table' in lib.yv4_last_error()
    assert lib.yv4_bbox_overlaps_batched(None, None, one, one, one, 1, 0, L.OVERLAPS_IOU, 1e-6, None, None) == 0   # no pairs
    assert lib.yv4_bbox_overlaps_batched(None, None, one, one, one, 1, 4, L.OVERLAPS_IOU, 1e-6, None, None) == -1
    assert b'null' in lib.yv4_last_error()
    assert lib.yv4_bbox_overlaps_batched(one, one, one, one, one, 1, 4, 7, 1e-6, one, None) == -1
    assert b'mode' in lib.yv4_last_error()

    def tpfp(mode=L.TPFP_DEFAULT, det=one, rank=one, order=one, P=1, D=4, G=0, thrs=one, T=1, area=None, K=1, work=one):
        return lib.yv4_tpfp_batched(mode, det, None, None, None, order, rank, one, one, one, P, D, G, None, thrs, T, area, K,
                                    work, one, one, None)
    assert tpfp(mode=5) == -1 and b'mode' in lib.yv4_last_error()
    assert tpfp(P=0) == -1 and b'problem table' in lib.yv4_last_error()
    assert tpfp(T=0) == -1 and b'thresholds' in lib.yv4_last_error()
    assert tpfp(K=3) == -1 and b'area_ranges' in lib.yv4_last_error()
    assert tpfp(D=0) == 0                                         # no detections: legal, nothing to do
    assert tpfp(det=None) == -1 and b'null' in lib.yv4_last_error()
    assert tpfp(rank=None) == -1 and b'rank' in lib.yv4_last_error()
    assert tpfp(mode=L.TPFP_IMAGENET, order=None) == -1 and b'order' in lib.yv4_last_error()
    assert tpfp(G=3) == -1 and b'ground-truth' in lib.yv4_last_error()
    assert tpfp(D=0x7f7f7f7f) == -1 and b'2^31' in lib.yv4_last_error()
    assert tpfp(det=ctypes.c_void_p(8)) == -1 and b'aligned' in lib.yv4_last_error()
    assert lib.yv4_tpfp_work(L.TPFP_DEFAULT, 100, 30, 5) == 4 * 100 + 4 * 5 * 30 + 8 * 100
    assert lib.yv4_tpfp_work(L.TPFP_IMAGENET, 100, 30, 5) == 4 * 100 + 4 * 5 * 100 + 5 * 30
    assert lib.yv4_tpfp_work(L.TPFP_DEFAULT, 100, 30, 0) == 0
