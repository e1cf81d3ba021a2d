"""metric='fast-bbox' from the flat table, CPU: the numpy restatement of the flat definition (tests/_flex_flat_ref.py)
against the oracle's eval_map_flexible on inputs without score ties -- num_det, num_gt and recall exactly, the float32
bits of mAP exactly (the condition on the inputs: the single-accumulator sum and numpy's pairwise sum agree there) --
``FlexGt``'s tables on hand-built annotations, and what the flat path refuses."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import eval_utils as EU
import _flex_flat_ref as F
from _eval_data import REPORT, SCALES, THRS10, dataset
from oracle import eval_oracle as E


def _same(got, want):
    assert F.keys(got) == F.keys(want)
    for a, b, name in zip(F.table(got), F.table(want), ('num_det', 'num_gt', 'recall', 'mAP')):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=name)


@pytest.mark.parametrize('shared_tp', [True, False])
def test_restatement_equals_oracle_on_the_fixture(golden, shared_tp):
    """The fixture's scores hold ties (two decimals), so its table is handed over in the list path's own tie order."""
    dets, annos, classes = dataset(golden('eval'))
    _, want = E.eval_map_flexible(dets, annos, THRS10, SCALES, classes, REPORT, shared_tp=shared_tp)
    out = F.eval_flex_flat(F.flatten_as_visited(dets), annos, len(classes), THRS10, SCALES, shared_tp)
    got = F.as_list(out, classes, SCALES, THRS10)
    assert len(got) == 200
    _same(got, want)
    if shared_tp:
        z = golden('eval')
        np.testing.assert_array_equal(F.table(got)[3], z['res/mAP'])
        np.testing.assert_array_equal(F.table(got)[2], z['res/recall'])
        for name, _ in REPORT:
            assert float(F.report(got, REPORT)[name]) == float(z[f'report/{name}'])


@pytest.mark.parametrize('shared_tp', [True, False])
def test_restatement_equals_oracle_on_the_seeded_set(shared_tp):
    dets, annos, classes = F.synth(0)
    _, want = E.eval_map_flexible(dets, annos, THRS10, SCALES, classes, REPORT, shared_tp=shared_tp)
    out = F.eval_flex_flat(F.flatten(dets), annos, len(classes), THRS10, SCALES, shared_tp)
    got = F.as_list(out, classes, SCALES, THRS10)
    assert len(got) == 200 and np.count_nonzero(F.table(got)[3]) > 100
    _same(got, want)


def test_restatement_does_not_depend_on_the_table_order():
    dets, annos, classes = F.synth(0, num_img=12)
    flat = F.flatten(dets)
    perm = np.random.default_rng(1).permutation(len(flat[0]))
    a = F.eval_flex_flat(flat, annos, len(classes), [0.5, 0.75], SCALES)
    b = F.eval_flex_flat(tuple(x[perm] for x in flat), annos, len(classes), [0.5, 0.75], SCALES)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def _hand_annotations():
    f = lambda rows: np.array(rows, np.float32).reshape(-1, 4)      # noqa: E731
    return [
        # image 0: class 1 gt, a crowd gt of class 0 (ignored), a class-0 gt whose area attribute (20^2 = small) disagrees
        # with its 50 x 50 box, a label outside [0, C)
        dict(gt_bboxes=f([[0, 0, 40, 40], [10, 10, 110, 110], [0, 0, 50, 50], [5, 5, 9, 9]]),
             gt_labels=np.array([1, 0, 0, 7]),
             gt_attrs=dict(ignore=np.array([False, True, False, False]), iscrowd=np.array([False, True, False, False]),
                           area=np.array([1600, 10000, 400, 16], np.float32))),
        # image 1: no gts
        dict(gt_bboxes=f([]), gt_labels=np.zeros(0, np.int64), gt_attrs={}),
        # image 2: an ignored (not crowd) gt and a regular one, areas from the boxes: exactly 32^2 and 96^2
        dict(gt_bboxes=f([[0, 0, 32, 32], [0, 0, 96, 96], [1, 1, 2, 2]]), gt_labels=np.array([0, 0, -1]),
             gt_attrs=dict(ignore=np.array([True, False, False]))),
    ]


def test_flex_gt_tables():
    gt = pkg.FlexGt(_hand_annotations(), 2, SCALES)
    N, C, B = 3, 2, 4
    assert (gt.num_imgs, gt.num_classes, gt.num_bkd) == (N, C, B)
    assert gt.names == ['All', 'Scale_S', 'Scale_M', 'Scale_L']
    np.testing.assert_array_equal(gt.bounds, np.array([[0, 1024], [1024, 9216], [9216, 1e8]], np.float32))
    # class-major: class 0 -> image 0 (crowd, odd-area), image 2 (ignored, regular); class 1 -> image 0
    np.testing.assert_array_equal(gt.gt_off, [0, 2, 2, 4, 5, 5, 5])
    np.testing.assert_array_equal(gt.gt, np.array([[10, 10, 110, 110], [0, 0, 50, 50], [0, 0, 32, 32], [0, 0, 96, 96],
                                                   [0, 0, 40, 40]], np.float32))
    np.testing.assert_array_equal(gt.crowd, [1, 0, 0, 0, 0])
    np.testing.assert_array_equal(gt.gt_bkd, [[0, 1, 0, 1, 1],          # All: ignore applied
                                              [0, 1, 0, 0, 0],          # S: the area attribute (400), not the box (2500)
                                              [0, 0, 0, 0, 1],          # M: 1600
                                              [0, 0, 0, 1, 0]])         # L: 96^2 is the lower bound, included
    np.testing.assert_array_equal(gt.num_gt, [[2, 1, 0, 1], [1, 0, 1, 0]])
    # Q side: problem p's gts once per breakdown
    ng = np.diff(gt.gt_off)
    assert len(gt.q_gt_off) == N * C * B + 1 and gt.q_gt_off[-1] == B * 5
    for p in range(N * C):
        for b in range(B):
            q = p * B + b
            assert gt.q_gt_off[q] == B * gt.gt_off[p] + b * ng[p]
            sl = slice(gt.q_gt_off[q], gt.q_gt_off[q] + ng[p])
            np.testing.assert_array_equal(gt.q_ignore[sl], 1 - gt.gt_bkd[b, gt.gt_off[p]:gt.gt_off[p + 1]])
            np.testing.assert_array_equal(gt.q_crowd[sl], gt.crowd[gt.gt_off[p]:gt.gt_off[p + 1]])
    # equal to the list path's own flags per (image, class)
    sb = pkg.ScaleBreakdown(SCALES, ['a', 'b'])
    for i, anno in enumerate(_hand_annotations()):
        for c in range(C):
            m = anno['gt_labels'] == c
            attrs = {k: v[m] for k, v in anno['gt_attrs'].items()}
            p = c * N + i
            np.testing.assert_array_equal(gt.gt_bkd[1:, gt.gt_off[p]:gt.gt_off[p + 1]],
                                          sb.breakdown_flags(anno['gt_bboxes'][m], attrs))
    with pytest.raises(ValueError):
        pkg.FlexGt([], 2, SCALES)
    assert pkg.FlexGt(_hand_annotations(), 2).names == ['All']


_FLAT = (np.zeros((1, 5), np.float32), np.zeros(1, np.int64), np.zeros(1, np.int64))
_BK = [dict(type='ScaleBreakdown', scale_ranges=SCALES)]


def test_flat_path_refuses_what_it_does_not_know(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # raised before any device call
    gt = pkg.FlexGt(_hand_annotations(), 2, SCALES)

    @pkg.EVAL_MATCHER.register_module()
    class FlatHostMatcher(pkg.MatcherCoCo):
        pass

    @pkg.EVAL_IOU_CALCULATOR.register_module()
    class FlatHostIou(pkg.IOU2DCoCo):
        pass

    mk = lambda bk=_BK, iou='IOU2DCoCo', m='MatcherCoCo': pkg.FlexibleStatisticsEval(      # noqa: E731
        ['a', 'b'], [0.5], bk, dict(type=iou), dict(type=m), 0)
    with pytest.raises(NotImplementedError, match='FlatHostMatcher'):
        mk(m='FlatHostMatcher').statistics_eval(_FLAT, gt)
    with pytest.raises(NotImplementedError, match='FlatHostIou'):
        mk(iou='FlatHostIou').statistics_eval(_FLAT, gt)
    with pytest.raises(NotImplementedError, match='apply_to'):
        mk([dict(type='ScaleBreakdown', scale_ranges=SCALES, apply_to=['a'])]).statistics_eval(_FLAT, gt)
    with pytest.raises(ValueError, match='breakdowns'):               # a FlexGt built for other ranges
        mk().statistics_eval(_FLAT, pkg.FlexGt(_hand_annotations(), 2))
    with pytest.raises(ValueError, match='class'):
        pkg.FlexibleStatisticsEval(['a'], [0.5], _BK, dict(type='IOU2DCoCo'), dict(type='MatcherCoCo'),
                                   0).statistics_eval(_FLAT, gt)


def test_flat_path_without_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    gt = pkg.FlexGt(_hand_annotations(), 2, EU.FAST_BBOX_SCALE_RANGES)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.evaluate_fast_bbox(_FLAT, gt, ['a', 'b'])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.evaluate_fast_bbox(_FLAT, _hand_annotations(), ['a', 'b'])


def _coco_dict():
    return dict(images=[dict(id=7), dict(id=3)], categories=[dict(id=1, name='a'), dict(id=5, name='b'), dict(id=9, name='z')],
                annotations=[dict(id=1, image_id=3, category_id=5, bbox=[0, 0, 10, 20], area=150.0, iscrowd=0),
                             dict(id=2, image_id=7, category_id=1, bbox=[5, 5, 100, 100], area=10000.0, iscrowd=1),
                             dict(id=3, image_id=3, category_id=9, bbox=[1, 1, 4, 4], area=16.0, iscrowd=0),
                             dict(id=4, image_id=7, category_id=1, bbox=[2, 2, 40, 40], area=1500.0, iscrowd=0)])


def test_dataset_fast_bbox_ground_truth_and_the_combined_metric():
    ds = pkg.CocoBBoxDataset(_coco_dict(), classes=('a', 'b'))
    with pytest.raises(AssertionError, match='fast-bbox evaluation can only be used alone!'):
        ds.evaluate(_FLAT, metric=['bbox', 'fast-bbox'])
    with pytest.raises(AssertionError, match='fast-bbox evaluation can only be used alone!'):
        ds.evaluate(_FLAT, metric=('fast-bbox', 'bbox'))
    with pytest.raises(TypeError, match='classwise'):
        ds.evaluate(_FLAT, metric='fast-bbox', classwise=True)
    gt = ds.flex_gt()
    assert gt is ds.flex_gt() and gt.names == ['All', 'Scale_S', 'Scale_M', 'Scale_L']
    assert (gt.num_imgs, gt.num_classes) == (2, 2)              # img_ids order: 7, 3; the 'z' box takes no part
    np.testing.assert_array_equal(gt.gt_off, [0, 2, 2, 2, 3])
    np.testing.assert_array_equal(gt.gt, np.array([[5, 5, 105, 105], [2, 2, 42, 42], [0, 0, 10, 20]], np.float32))
    np.testing.assert_array_equal(gt.crowd, [1, 0, 0])
    np.testing.assert_array_equal(gt.gt_bkd, [[0, 1, 1], [0, 0, 1], [0, 1, 0], [0, 0, 0]])
    np.testing.assert_array_equal(gt.num_gt, [[1, 0, 1, 0], [1, 1, 0, 0]])
