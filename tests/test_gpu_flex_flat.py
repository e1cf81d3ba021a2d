"""metric='fast-bbox' from the flat table, on the GPU (csrc/flex_eval.hip through eval_utils.flex_flat_device): against
the reference-made fixture (tests/golden/eval.npz), the list path and the numpy restatement of the flat definition
(tests/_flex_flat_ref.py, held against the oracle in tests/test_flex_flat_host.py).  Tolerance: none -- num_det, num_gt
and recall exactly, mAP bit for bit."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd import eval_utils as EU
from mmdet_yolov4_amd import hooks as H
import _eval_hook_data as DATA
import _flex_flat_ref as F
from _eval_data import REPORT, SCALES, THRS10, dataset, result_table

pytestmark = pytest.mark.gpu
BK = [dict(type='ScaleBreakdown', scale_ranges=SCALES)]
THRS2 = [0.5, 0.75]


def _fse(classes, thrs, shared_tp=True, bk=BK):
    return pkg.FlexibleStatisticsEval(classes, thrs, bk, dict(type='IOU2DCoCo'), dict(type='MatcherCoCo'), 0,
                                      shared_tp=shared_tp)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_tables(got, want):
    for k in ('num_det', 'num_gt', 'recall', 'mAP'):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)


def _check(flat, annos, C, thrs=THRS2, scales=SCALES, shared_tp=True):
    """The device against the restatement; returns the device's tables."""
    got = EU.flex_flat_device(flat, pkg.FlexGt(annos, C, scales), thrs, shared_tp)
    _same_tables(got, F.eval_flex_flat(flat, annos, C, thrs, scales, shared_tp))
    return got


def _gpu(flat, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in flat)


def _same_lists(got, want):
    assert F.keys(got) == F.keys(want)
    for a, b, name in zip(F.table(got), F.table(want), ('num_det', 'num_gt', 'recall', 'mAP')):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=name)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['numpy', 'gpu'])
def test_fixture_from_the_flat_table(golden, gpu_device, form):
    """The fixture's scores hold ties, so its rows are handed over in the list path's own tie order."""
    z = golden('eval')
    dets, annos, classes = dataset(z)
    flat = F.flatten_as_visited(dets)
    if form == 'gpu':
        flat = _gpu(flat, gpu_device)
    gt = pkg.FlexGt(annos, len(classes), SCALES)
    res = _fse(classes, THRS10).statistics_eval(flat, gt)
    key, recall, ap = result_table(res, classes)
    assert np.array_equal(key, z['res/key'])
    assert np.array_equal(recall, z['res/recall'])
    assert np.array_equal(_bits(ap), _bits(z['res/mAP']))
    report = pkg.eval_map_flexible(flat, gt, iou_thrs=THRS10, breakdown=BK, classes=classes, report_config=REPORT, nproc=-1)
    assert list(report) == [n for n, _ in REPORT]
    for name, _ in REPORT:
        assert float(report[name]) == float(z[f'report/{name}'])
    fast = pkg.evaluate_fast_bbox(flat, pkg.FlexGt(annos, len(classes), EU.FAST_BBOX_SCALE_RANGES), classes)
    assert list(fast) == list(report) and all(float(fast[k]) == float(report[k]) for k in fast)
    # per-image annotation dicts with flat results: the FlexGt is built per call
    again = pkg.evaluate_fast_bbox(flat, annos, classes)
    assert all(float(again[k]) == float(report[k]) for k in fast)


@pytest.mark.parametrize('shared_tp', [True, False])
def test_shared_tp_quirk(golden, shared_tp):
    z = golden('eval')
    det, annos = [[z['quirk/det']]], [dict(gt_bboxes=z['quirk/gt'], gt_labels=np.array([0, 0]), gt_attrs={})]
    res = _fse(['a'], [0.95], shared_tp).statistics_eval(F.flatten(det), pkg.FlexGt(annos, 1, SCALES))
    if shared_tp:
        assert np.array_equal(np.array([v['mAP'] for _, v in res], np.float32), z['quirk/mAP'])
        assert np.array_equal([v['num_det'] for _, v in res], z['quirk/num_det'])
        assert z['quirk/mAP'][0] == 0.5
    else:
        assert res[0][1]['mAP'] == 1.0
    _same_lists(res, _fse(['a'], [0.95], shared_tp).statistics_eval(det, annos))


# ---- flat against list against the restatement --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tie_free():
    dets, annos, classes = F.synth(0)
    flat = F.flatten(dets)
    want = {st: F.eval_flex_flat(flat, annos, len(classes), THRS10, SCALES, st) for st in (True, False)}
    return dets, annos, classes, flat, want


@pytest.mark.parametrize('shared_tp', [True, False])
def test_flat_list_and_restatement_agree_without_ties(tie_free, shared_tp):
    dets, annos, classes, flat, want = tie_free
    got = _fse(classes, THRS10, shared_tp).statistics_eval(flat, pkg.FlexGt(annos, len(classes), SCALES))
    assert len(got) == 200 and np.count_nonzero(F.table(got)[3]) > 100
    _same_lists(got, F.as_list(want[shared_tp], classes, SCALES, THRS10))
    _same_lists(got, _fse(classes, THRS10, shared_tp).statistics_eval(dets, annos))
    assert [type(v['num_det']) for _, v in got[:1]] == [int] and got[0][1]['mAP'].dtype == np.float32


def test_shuffled_table_and_two_runs(tie_free, gpu_device):
    dets, annos, classes, flat, want = tie_free
    gt = pkg.FlexGt(annos, len(classes), SCALES)
    a = EU.flex_flat_device(flat, gt, THRS10)
    _same_tables(a, want[True])
    perm = np.random.default_rng(3).permutation(len(flat[0]))
    b = EU.flex_flat_device(_gpu(tuple(x[perm] for x in flat), gpu_device), gt, THRS10)
    c = EU.flex_flat_device(flat, gt, THRS10)
    for k in ('num_det', 'recall', 'mAP'):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_quantised_scores_against_the_restatement():
    dets, annos, classes = F.synth(2, num_img=16, quant=12)
    flat = F.flatten(dets)
    assert len(np.unique(flat[0][:, 4])) <= 12 < len(flat[0])
    for shared_tp in (True, False):
        _check(flat, annos, len(classes), THRS10, SCALES, shared_tp)


# ---- crafted inputs -----------------------------------------------------------------------------------------------------
def _boxes(rng, n, lo=4, hi=160):
    xy = rng.uniform(0, 400, (n, 2))
    return np.concatenate([xy, xy + rng.uniform(lo, hi, (n, 2))], 1).astype(np.float32)


def _scores(rng, n):
    sc = (rng.choice(1 << 20, size=n, replace=False) / (1 << 20)).astype(np.float32)
    assert len(np.unique(sc)) == n
    return sc


def test_class_sizes_around_the_chunk_and_the_wave():
    """One class each with 0 .. 5 003 detections: below, at and above a wave (64), a chunk (256) and four chunks."""
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5003]
    rng = np.random.default_rng(4)
    N, C = 6, len(sizes)
    annos, det, lab, img = [], [], [], []
    for i in range(N):
        ng = 2 * C
        gb = _boxes(rng, ng)
        annos.append(dict(gt_bboxes=gb, gt_labels=np.repeat(np.arange(C), 2).astype(np.int64),
                          gt_attrs=dict(ignore=rng.random(ng) < 0.2)))
    for c, n in enumerate(sizes):
        im = rng.integers(0, N, n)
        b = _boxes(rng, n)
        near = rng.random(n) < 0.5                               # half of them: noisy copies of one of the image's gts
        src = np.array([annos[i]['gt_bboxes'][2 * c + rng.integers(0, 2)] for i in im], np.float32).reshape(-1, 4)
        b[near] = (src + rng.normal(0, 4, src.shape).astype(np.float32))[near]
        det.append(np.concatenate([b, _scores(rng, n)[:, None]], 1))
        lab.append(np.full(n, c, np.int64))
        img.append(im.astype(np.int64))
    perm = rng.permutation(sum(sizes))
    flat = tuple(np.concatenate(x)[perm] for x in (det, lab, img))
    got = _check(flat, annos, C)
    kept = got['num_det'][:, 0, 0]                               # a detection on an ignored gt drops out of the count
    assert np.all(kept <= sizes) and np.all(kept >= np.array(sizes) * 0.9 - 1) and kept[-1] > 4096
    assert np.count_nonzero(got['mAP'][1:, 0]) >= 2 * (C - 2)


def _ranked_case(groups, gts_per_img, N=3, seed=6):
    """One class over N images; ``groups``: (count, side, matches) runs in descending-score order -- ``count`` detections
    of about ``side`` pixels, copies of the images' gts of that side when ``matches``."""
    rng = np.random.default_rng(seed)
    annos = []
    for i in range(N):
        gb = np.concatenate([np.array([[x, 10.0, x + s, 10.0 + s]], np.float32)
                             for x, s in zip(np.cumsum([0] + [s + 20 for s in gts_per_img[:-1]]), gts_per_img)])
        annos.append(dict(gt_bboxes=gb.astype(np.float32), gt_labels=np.zeros(len(gb), np.int64), gt_attrs={}))
    total = sum(g[0] for g in groups)
    score = np.sort(_scores(rng, total))[::-1]
    rows, img = [], []
    for count, side, matches in groups:
        im = rng.integers(0, N, count)
        if matches:
            pool = annos[0]['gt_bboxes'][np.isclose(annos[0]['gt_bboxes'][:, 2] - annos[0]['gt_bboxes'][:, 0], side)]
            b = pool[rng.integers(0, len(pool), count)] + rng.normal(0, 0.02 * side, (count, 4)).astype(np.float32)
        else:
            xy = rng.uniform(500, 900, (count, 2))
            b = np.concatenate([xy, xy + side + rng.uniform(0, 1, (count, 2))], 1)
        rows.append(b.astype(np.float32))
        img.append(im)
    dets = np.concatenate([np.concatenate(rows), score[:, None]], 1).astype(np.float32)
    return (dets, np.zeros(total, np.int64), np.concatenate(img).astype(np.int64)), annos


def test_mask_that_empties_whole_chunks():
    """300 large, 300 small, 300 large detections by score: the small range's list has no position in the first chunk or in
    the last, the medium range's list is empty, and the large range's skips a chunk in the middle."""
    flat, annos = _ranked_case([(300, 120, True), (212, 20, False), (88, 20, True), (300, 120, False)], [20, 120, 20])
    got = _check(flat, annos, 1)
    assert got['num_det'][0, 0, 0] == 900 and got['num_det'][0, 2, 0] == 0 and 0 < got['num_det'][0, 1, 0] <= 300
    assert got['mAP'][0, 1, 0] > 0 and got['mAP'][0, 3, 0] > 0 and got['mAP'][0, 2, 0] == 0
    _check(flat, annos, 1, shared_tp=False)


def test_true_positives_only_in_late_chunks():
    flat, annos = _ranked_case([(700, 50, False), (40, 50, True)], [50, 50])
    got = _check(flat, annos, 1)
    assert 0 < got['mAP'][0, 0, 0] < 0.05 and got['recall'][0, 0, 0] > 0


def test_no_ground_truth_and_no_detections():
    """Class 0: detections, no gt (num_gt == 0); class 1: neither; class 2: gts, no detections."""
    rng = np.random.default_rng(8)
    annos = [dict(gt_bboxes=_boxes(rng, 3), gt_labels=np.full(3, 2, np.int64), gt_attrs={}) for _ in range(2)]
    flat = (np.concatenate([_boxes(rng, 300), _scores(rng, 300)[:, None]], 1).astype(np.float32), np.zeros(300, np.int64),
            rng.integers(0, 2, 300).astype(np.int64))
    got = _check(flat, annos, 3)
    assert got['num_det'][0, 0, 0] == 300 and not got['num_det'][1:].any() and not got['mAP'].any()
    assert not got['recall'].any() and got['num_gt'][2, 0] == 6


def test_ignored_and_crowd_ground_truth():
    """Image 0: every gt ignored -- its matched detections drop out of the count.  Image 1: a crowd gt that is not ignored
    is matched again and again (recall above 1) beside an ignored crowd gt and a regular gt."""
    rng = np.random.default_rng(9)
    g0 = np.array([[10, 10, 110, 110], [200, 10, 260, 70]], np.float32)
    g1 = np.array([[10, 10, 210, 210], [300, 10, 400, 110], [10, 300, 70, 360]], np.float32)
    annos = [dict(gt_bboxes=g0, gt_labels=np.zeros(2, np.int64), gt_attrs=dict(ignore=np.array([True, True]))),
             dict(gt_bboxes=g1, gt_labels=np.zeros(3, np.int64),
                  gt_attrs=dict(ignore=np.array([False, True, False]), iscrowd=np.array([True, True, False])))]
    rows, img = [], []
    for i, g in enumerate((g0, g1)):
        for box in g:
            rows.append(box + rng.normal(0, 1.5, (6, 4)).astype(np.float32))
            img += [i] * 6
        inside = np.array([[20, 20, 60, 60], [100, 100, 180, 180]], np.float32)      # inside the crowd gt of image 1
        rows.append(inside)
        img += [i] * 2
    boxes = np.concatenate(rows)
    flat = (np.concatenate([boxes, _scores(rng, len(boxes))[:, None]], 1).astype(np.float32), np.zeros(len(boxes), np.int64),
            np.array(img, np.int64))
    for shared_tp in (True, False):
        got = _check(flat, annos, 1, shared_tp=shared_tp)
    assert got['num_det'][0, 0, 0] < len(boxes)                 # the detections on ignored gts are not counted
    assert got['num_gt'][0, 0] == 2 and got['recall'][0, 0, 0] > 1.0
    only_ignored = (flat[0][flat[2] == 0], flat[1][flat[2] == 0], flat[2][flat[2] == 0])
    got = _check(only_ignored, annos[:1], 1)
    assert got['num_gt'][0, 0] == 0 and got['num_det'][0, 0, 0] < len(only_ignored[0]) and got['mAP'][0, 0, 0] == 0


def test_more_ground_truths_than_lanes():
    rng = np.random.default_rng(10)
    gb = _boxes(rng, 70, 20, 120)
    annos = [dict(gt_bboxes=gb, gt_labels=np.zeros(70, np.int64), gt_attrs=dict(ignore=rng.random(70) < 0.1))]
    b = np.concatenate([gb + rng.normal(0, 3, gb.shape).astype(np.float32), _boxes(rng, 40)])
    flat = (np.concatenate([b, _scores(rng, len(b))[:, None]], 1).astype(np.float32), np.zeros(len(b), np.int64),
            np.zeros(len(b), np.int64))
    got = _check(flat, annos, 1)
    assert got['recall'][0, 0, 0] > 0.5


def test_rows_out_of_range_take_no_part(tie_free):
    dets, annos, classes, flat, want = tie_free
    N, C = len(annos), len(classes)
    rng = np.random.default_rng(12)
    extra = 40
    d = np.concatenate([flat[0], flat[0][:extra]])
    lab = np.concatenate([flat[1], np.array([-1, C, 0, 0] * (extra // 4), np.int64)])
    img = np.concatenate([flat[2], np.array([0, 0, -1, N] * (extra // 4), np.int64)])
    perm = rng.permutation(len(d))
    got = EU.flex_flat_device((d[perm], lab[perm], img[perm]), pkg.FlexGt(annos, C, SCALES), THRS10)
    _same_tables(got, want[True])


def test_one_image_one_class_and_the_empty_table(gpu_device):
    rng = np.random.default_rng(13)
    gb = _boxes(rng, 4)
    annos = [dict(gt_bboxes=gb, gt_labels=np.zeros(4, np.int64), gt_attrs={})]
    b = np.concatenate([gb + rng.normal(0, 2, gb.shape).astype(np.float32), _boxes(rng, 3)])
    flat = (np.concatenate([b, _scores(rng, 7)[:, None]], 1).astype(np.float32), np.zeros(7, np.int64), np.zeros(7, np.int64))
    got = _check(flat, annos, 1, thrs=[0.5], scales=None)       # N = C = B = T = 1
    assert got['mAP'].shape == (1, 1, 1) and got['mAP'][0, 0, 0] > 0
    empty = (np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    for tab in (empty, _gpu(empty, gpu_device)):
        got = EU.flex_flat_device(tab, pkg.FlexGt(annos, 1, SCALES), THRS2)
        assert not got['num_det'].any() and not got['recall'].any() and not got['mAP'].any()
        assert got['mAP'].shape == (1, 4, 2) and got['num_gt'][0, 0] == 4
    res = pkg.evaluate_fast_bbox(empty, annos, ['a'])
    assert float(res['map']) == 0.0


# ---- the table expansion --------------------------------------------------------------------------------------------------
def test_flex_tables_against_its_formulas(gpu_device):
    rng = np.random.default_rng(14)
    P, B, guard = 300, 4, -0x0123456789abcdf
    nd = rng.integers(0, 9, P) * (rng.random(P) < 0.7)
    ng = rng.integers(0, 5, P)
    det_off, iou_off = EU._offsets(nd), EU._offsets(nd * ng)
    Q = P * B
    outs = [torch.full((Q + 3,), guard, dtype=torch.int64, device=gpu_device) for _ in range(2)]
    t_do, t_io = (torch.from_numpy(x).to(gpu_device) for x in (det_off, iou_off))
    rc = _lib.lib().yv4_flex_tables(t_do.data_ptr(), t_io.data_ptr(), P, B, outs[0][1:].data_ptr(), outs[1][1:].data_ptr(), None)
    assert rc == 0
    q_det, q_iou = (o.cpu().numpy() for o in outs)
    for o in (q_det, q_iou):
        assert o[0] == guard and o[-1] == guard
    p, b = np.repeat(np.arange(P), B), np.tile(np.arange(B), P)
    np.testing.assert_array_equal(q_det[1:-2], B * det_off[p] + b * nd[p])
    np.testing.assert_array_equal(q_iou[1:-2], iou_off[p])
    assert q_det[-2] == B * det_off[P] and q_iou[-2] == iou_off[P]
    # and the matching kernel runs straight off them: problem q's block is (T, nd) at q_det_off[q] * T
    assert np.all(np.diff(q_det[1:-1]) == nd[p])


def test_entry_points_refuse_bad_arguments(gpu_device):
    lib = _lib.lib()
    t = torch.zeros(16, dtype=torch.int64, device=gpu_device)
    p = t.data_ptr()
    assert lib.yv4_flex_tables(None, p, 1, 1, p, p, None) == -1
    assert lib.yv4_flex_tables(p, p, -1, 1, p, p, None) == -1
    assert lib.yv4_flex_tables(p, p, 1, 0, p, p, None) == -1
    assert lib.yv4_flex_accumulate(p, p, p, p, p, p, p, p, -1, 0, 1, 1, 1, 1, 1, p, p, p, p, None) == -1
    assert lib.yv4_flex_accumulate(p, p, p, None, p, p, p, p, 0, 0, 1, 1, 1, 1, 1, p, p, p, p, None) == -1
    assert lib.yv4_flex_accumulate(None, p, p, p, p, p, p, p, 4, 0, 1, 1, 1, 1, 1, p, p, p, p, None) == -1
    assert lib.yv4_flex_accumulate_work(-1, 1, 1) == 0 and lib.yv4_flex_accumulate_work(10, 2, 4) == 8 * 10 * 2 * 4


# ---- the hooks ----------------------------------------------------------------------------------------------------------
def test_eval_hook_scores_fast_bbox_from_the_flat_loop(gpu_device):
    det = DATA.tiny_v4(DATA.make_test_cfg(), gpu_device)
    pipe = pkg.FusedTestPipeline(img_scale=(128, 128), device=gpu_device)
    imgs = DATA.images()
    DATA.lift_head(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    lists = pkg.single_gpu_test(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    received = []

    class Recording(pkg.CocoBBoxDataset):
        def evaluate(self, results, **kw):
            received.append(results)
            return super().evaluate(results, **kw)
    ds = Recording(DATA.synthetic_gt(lists, imgs), classes=[f'c{c}' for c in DATA.CAT_IDS])
    loader = DATA.Loader(pipe, imgs, range(DATA.SIZE), dataset=ds)
    flat = pkg.single_gpu_test(det, loader, flat=True)
    want = ds.evaluate(lists, metric='fast-bbox', logger='silent')
    assert list(want) == ['map', 'map50', 'map75', 's_map', 'm_map', 'l_map'] and float(want['map']) > 0
    got = ds.evaluate(flat, metric='fast-bbox', logger='silent')
    assert all(float(got[k]) == float(want[k]) or (np.isnan(got[k]) and np.isnan(want[k])) for k in want)
    assert ds.flex_gt() is ds.flex_gt()
    del received[:]
    outs = []
    for kw in (dict(), dict(flat=False)):
        runner = H.Runner(det, None, max_epochs=1)
        H.EvalHook(loader, interval=1, metric='fast-bbox', **kw).after_train_epoch(runner)
        outs.append(dict(runner.log_buffer.output))
    assert isinstance(received[0], tuple) and all(t.is_cuda for t in received[0])      # flat by default
    assert isinstance(received[1], list)
    for k in want:
        a, b = float(outs[0][k]), float(outs[1][k])
        assert a == b == float(want[k]) or (np.isnan(a) and np.isnan(b))
    with pytest.raises(AssertionError, match='fast-bbox evaluation can only be used alone!'):
        ds.evaluate(flat, metric=['fast-bbox', 'bbox'])
