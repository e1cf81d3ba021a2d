"""VOC-style mAP from the flat table, without a GPU: the numpy restatement of the flat definition
(tests/_map_flat_ref.py: problem keys, stable orders, accumulation with a single float64 accumulator in rank order)
against the reference's outputs in tests/golden/map_eval.npz, bit for bit and with exact dtypes -- the fixture's scores
are pairwise distinct within every class, so the stable order and the reference's argsort visit alike -- and the host
side of the feature: CustomBBoxDataset, the binding, and the refusals that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _map_flat_ref as F  # noqa: E402
import _map_ref as R  # noqa: E402
from _map_data import CASES, assert_result_equals_fixture, load_dataset, without_detections  # noqa: E402

import mmdet_yolov4_amd as pkg  # noqa: E402
from mmdet_yolov4_amd import map_eval as ME  # noqa: E402
from mmdet_yolov4_amd.coco_eval import flatten_results  # noqa: E402


@pytest.fixture(scope='module')
def z(golden):
    return golden('map_eval')


@pytest.fixture(scope='module')
def data(z):
    return load_dataset(z)


@pytest.mark.parametrize('name', list(CASES))
def test_restated_flat_definition_equals_the_reference(z, data, name):
    dets, annos = data
    flat = F.flatten(without_detections(dets) if name == 'empty' else dets)
    mean_ap, results = F.eval_map_flat(flat, annos, 6, **CASES[name])
    assert_result_equals_fixture(z, name, mean_ap, results)


def test_flatten_agrees_with_the_package_and_shuffling_changes_nothing(z, data):
    dets, annos = data
    flat = F.flatten(dets)
    for a, b in zip(flat, flatten_results(dets)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    perm = np.random.default_rng(0).permutation(len(flat[0]))
    mean_ap, results = F.eval_map_flat(tuple(a[perm] for a in flat), annos, 6, **CASES['thr70_scales'])
    assert_result_equals_fixture(z, 'thr70_scales', mean_ap, results)


def test_restated_order_is_stable_and_out_of_range_rows_take_no_part():
    sc = np.array([.5, .9, .5, -0., 0., .9], np.float32)
    assert F.stable_desc(sc).tolist() == [1, 5, 0, 2, 3, 4]
    part, key = F.problem_keys([0, 2, -1, 1, 1], [0, 1, 0, 3, -1], num_imgs=3, num_classes=2)
    assert part.tolist() == [True, False, False, False, False] and key[0] == 0
    # the levels the kernel forms as j * 0.1 in float64 are np.arange's
    assert np.array_equal(np.arange(0, 1 + 1e-3, 0.1), np.arange(11) * 0.1)


def test_single_accumulator_and_pairwise_sum_are_different_orders():
    """Why the order is stated: np.sum and np.cumsum(...)[-1] are not the same float64 sum."""
    terms = np.random.default_rng(1).random(4096) * 1e-3
    seq = np.cumsum(terms)[-1]
    run = 0.0
    for v in terms:
        run += v
    assert seq == run                                            # cumsum is the single accumulator
    r = np.cumsum(np.full(300, 1 / 300))
    p = np.linspace(1, .3, 300).astype(np.float32)
    assert F.average_precision(r, p).dtype == np.float32
    assert abs(float(F.average_precision(r, p)) - float(R.average_precision(r, p))) <= 2 ** -23


def test_custom_bbox_dataset_on_the_host(data):
    dets, annos = data
    names = [f'c{i}' for i in range(6)]
    ds = pkg.CustomBBoxDataset(annos, names)
    assert ds.accepts_flat is True and ds.CLASSES == tuple(names) and len(ds) == len(annos)
    assert ds.get_ann_info(3) is annos[3]
    assert isinstance(ds.map_gt, pkg.MapGt) and ds.map_gt.num_classes == 6 and ds.map_gt.num_imgs == len(annos)
    flat = flatten_results(dets)
    for res in (dets, flat):
        with pytest.raises(KeyError, match='not supported'):
            ds.evaluate(res, metric='bbox')
        with pytest.raises(NotImplementedError, match='RPN proposals'):
            ds.evaluate(res, metric='recall')
    with pytest.raises(TypeError):
        ds.evaluate(dets, jsonfile_prefix='x')                    # no **kwargs: the signature is the reference's


def test_map_gt_holds_the_tables_the_list_path_builds(data):
    dets, annos = data
    tab, gt = ME.MapTables(dets, annos), pkg.MapGt(annos, 6)
    for name in ('gt', 'gt_ignore', 'ng', 'gt_off'):
        a, b = getattr(tab, name), getattr(gt, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    for area in (None, ME._area_table([(0, 1024.), (1024., 9216.), (9216., 1e10)])):
        assert np.array_equal(gt.num_gts(area), ME._num_gts(tab, area))
    m1, ratio = gt.imagenet_tables()
    assert m1.dtype == np.float32 and np.array_equal(m1, tab.gt - np.float32(1)) and ratio.shape == (len(tab.gt),)
    with pytest.raises(ValueError, match='at least one'):
        pkg.MapGt([], 3)


def test_foreign_tpfp_fn_with_flat_input_raises_before_any_device_call(data, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    dets, annos = data
    flat = flatten_results(dets)
    with pytest.raises(ValueError, match='tpfp_default and tpfp_imagenet only'):
        pkg.eval_map(flat, annos, tpfp_fn=R.tpfp_default, num_classes=6, logger='silent')
    with pytest.raises(ValueError, match='class count'):
        pkg.eval_map(flat, annos, logger='silent')
    with pytest.raises(RuntimeError, match='no CPU fallback'):    # the device path itself: no GPU, no fallback
        pkg.eval_map(flat, annos, num_classes=6, logger='silent')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.evaluate_map(flat, pkg.MapGt(annos, 6), logger='silent')


def test_flat_symbols_are_bound_and_validate_their_arguments():
    L = pkg._lib
    assert L.FEATURES['map_flat'].symbols == {'yv4_map_rank_work', 'yv4_map_rank', 'yv4_map_accumulate_work', 'yv4_map_accumulate'}
    assert L.FEATURES['map_flat'].symbols <= set(L.SIGNATURES) and L.has('map_flat')
    lib = L.lib()
    one = ctypes.c_void_p(256)                                   # non-null, aligned, never read

    def rank(D=4, N=2, C=3, gt_off=one, det=one, work=one, det4=one):
        return lib.yv4_map_rank(det, one, one, D, N, C, gt_off, work, det4, one, one, one, one, one, one, None)
    assert rank(N=0) == -1 and b'31 bits' in lib.yv4_last_error()
    assert rank(N=1 << 20, C=1 << 12) == -1 and b'31 bits' in lib.yv4_last_error()
    assert rank(gt_off=None) == -1 and b'problem table' in lib.yv4_last_error()
    assert rank(D=-1) == -1 and rank(D=0x7f7f7f7f) == -1 and b'2^31' in lib.yv4_last_error()
    assert rank(det=None) == -1 and b'null' in lib.yv4_last_error()
    assert rank(work=ctypes.c_void_p(4)) == -1 and rank(det4=ctypes.c_void_p(8)) == -1 and b'aligned' in lib.yv4_last_error()

    def acc(D=4, N=2, C=3, T=1, K=1, mode=L.MAP_AP_AREA, tp=one, rec=None, prec=None, ap=one):
        return lib.yv4_map_accumulate(tp, one, one, one, one, D, N, C, T, K, mode, one, ap, one, one, rec, prec, one, None)
    assert acc(C=0) == -1 and b'31 bits' in lib.yv4_last_error()
    assert acc(T=0) == -1 and acc(K=0) == -1 and b'area ranges' in lib.yv4_last_error()
    assert acc(mode=2) == -1 and b'mode' in lib.yv4_last_error()
    assert acc(ap=None) == -1 and acc(tp=None) == -1 and b'null' in lib.yv4_last_error()
    assert acc(rec=one) == -1 and b'pair' in lib.yv4_last_error()
    assert lib.yv4_map_rank_work(-1) == 0 and lib.yv4_map_rank_work(0) > 0
    assert lib.yv4_map_rank_work(100000) >= 2 * 8 * 100000 + 6 * 4 * 100000
    assert lib.yv4_map_accumulate_work(1000, 10, 3) >= 4 * 1000 * 30 and lib.yv4_map_accumulate_work(5, 0, 1) == 0
