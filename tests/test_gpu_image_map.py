"""The per-image mAP on the GPU (analysis.py, csrc/map_image.hip): ``image_maps`` and ``bbox_map_eval`` against what the
reference's ``bbox_map_eval`` produced (tests/golden/image_map.npz), against this package's own ``eval_map`` loop, and
against the numpy restatement (tests/_image_map_ref.py) at the boundaries of the kernel's thread map."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import analysis as A

import _image_map_ref as I
import _map_data as MD

pytestmark = pytest.mark.gpu

_SETS = {}


def _set(golden, name):
    """A set of the fixture with its flat form, loaded once and left unchanged."""
    if name not in _SETS:
        dets, annos, maps, per_thr = I.load_set(golden('image_map'), name)
        _SETS[name] = dict(dets=dets, annos=annos, maps=maps, per_thr=per_thr, flat=pkg.flatten_results(dets), C=len(dets[0]))
    return _SETS[name]


def _check(got, got_thr, s):
    assert got.dtype == np.float64 and got_thr.dtype == np.float32
    np.testing.assert_array_equal(got_thr, s['per_thr'])
    np.testing.assert_array_equal(got, s['maps'])


@pytest.mark.parametrize('name', I.SETS)
def test_image_maps_equals_the_reference_fixture(name, golden, gpu_device):
    s = _set(golden, name)
    _check(*pkg.image_maps(s['dets'], s['annos'], per_threshold=True), s)                                   # lists
    _check(*pkg.image_maps(s['flat'], s['annos'], num_classes=s['C'], per_threshold=True), s)               # flat numpy
    gt = pkg.MapGt(s['annos'], s['C'])
    dev = tuple(torch.from_numpy(a).to(gpu_device) for a in s['flat'])
    first = pkg.image_maps(dev, gt, per_threshold=True)                                                       # GPU tensors
    _check(*first, s)
    again = pkg.image_maps(dev, gt, per_threshold=True)                                                       # cached MapGt
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    table = pkg.DeviceResults(s['C'], gpu_device, capacity=16)
    table.append_lists(s['dets'])
    _check(*pkg.image_maps(table, gt, per_threshold=True), s)                                                 # DeviceResults
    np.testing.assert_array_equal(pkg.image_maps(s['dets'], s['annos']), s['maps'])
    with pytest.raises(ValueError, match='class count'):
        pkg.image_maps(s['flat'], s['annos'])


def test_flat_rows_in_another_order_and_rows_outside_take_no_part(golden, gpu_device):
    s = _set(golden, 'main')
    dets, labels, img = s['flat']
    N, C = len(s['dets']), s['C']
    perm = np.random.default_rng(3).permutation(len(dets))            # scores are distinct inside a problem: any order
    junk = np.array([[0, 0, 10, 10, 0.99]] * 4, np.float32)
    d = np.concatenate([junk[:2], dets[perm], junk[2:]])
    lab = np.concatenate([[C, -1], labels[perm], [0, 0]])
    im = np.concatenate([[0, 0], img[perm], [N, -1]])
    _check(*pkg.image_maps((d, lab, im), s['annos'], num_classes=C, per_threshold=True), s)


@pytest.mark.parametrize('name', I.SETS)
def test_bbox_map_eval_equals_the_reference_fixture(name, golden, gpu_device):
    s = _set(golden, name)
    for i, (d, a) in enumerate(zip(s['dets'], s['annos'])):
        got = pkg.bbox_map_eval(d, a)
        assert type(got) is float and got == s['maps'][i], (i, got, s['maps'][i])
    assert pkg.bbox_map_eval((s['dets'][0], None), s['annos'][0]) == s['maps'][0]       # a (bbox, segm) tuple


def test_equals_this_packages_eval_map_loop(golden, gpu_device):
    """Five images against ``eval_map([dets_i], [ann_i], iou_thr=np.float64 thr)`` of this package, which rounds a
    threshold to the NEAREST float32: the two agree unless an IoU equals such a rounded threshold, which is the case
    on the 0.7 image and there alone."""
    z = golden('image_map')
    s = _set(golden, 'main')
    thrs = [t for t in A.default_iou_thrs()]
    assert all(isinstance(t, np.float64) for t in thrs)

    def loop(i):
        means = [m for m, _ in pkg.eval_map([s['dets'][i]], [s['annos'][i]], iou_thr=thrs, logger='silent')]
        return sum(means) / len(means)
    maps = pkg.image_maps(s['dets'], s['annos'])
    busiest = np.argsort([-sum(len(d) for d in per_cls) for per_cls in s['dets']], kind='stable')[:4]
    for i in list(busiest) + [int(z['main/hand/det_of_class_without_gt'])]:
        assert loop(int(i)) == maps[i], i
    i = int(z['main/iou07_image'])
    assert maps[i] == 0.4 and loop(i) == 0.5          # nearest rounding calls float32(0.7) >= 0.7 a hit


def _single_problem(nd, ng, seed):
    """One image, one class: ``ng`` gts and ``nd`` detections -- noisy copies of the gts in three qualities, clutter
    behind them -- with distinct scores."""
    rng = np.random.default_rng(seed)
    gts = MD.boxes(rng, ng)
    reps = np.concatenate([gts + rng.normal(0, s, gts.shape).astype(np.float32) for s in (1.0, 4.0, 9.0)])
    cand = np.concatenate([reps, MD.boxes(rng, max(nd - len(reps), 0))])
    cand = cand[rng.permutation(len(cand))[:nd]]
    sc = (rng.choice(20000, size=nd, replace=False) / 20000).astype(np.float32)
    dets = np.concatenate([cand, sc[:, None]], 1).astype(np.float32)
    return [[dets]], [dict(bboxes=gts, labels=np.zeros(ng, np.int64))]


@pytest.mark.parametrize('ng', [1, 70])
@pytest.mark.parametrize('nd', [1, 63, 64, 65, 255, 256, 257, 600])
def test_thread_map_boundaries_on_a_single_problem(nd, ng, gpu_device):
    dets, annos = _single_problem(nd, ng, 100 * ng + nd)
    want, want_thr = I.image_maps(dets, annos)
    got, got_thr = pkg.image_maps(dets, annos, per_threshold=True)
    np.testing.assert_array_equal(got_thr, want_thr)
    np.testing.assert_array_equal(got, want)
    assert ng == 1 or nd < 64 or 0.0 < got[0] < 1.0              # the large cases are no trivial score


def test_more_gts_than_one_chunk(gpu_device):
    dets, annos = _single_problem(65, 300, 9)
    annos[0]['bboxes_ignore'], annos[0]['labels_ignore'] = annos[0]['bboxes'][250:] + np.float32(3), np.zeros(50, np.int64)
    annos[0]['bboxes'], annos[0]['labels'] = annos[0]['bboxes'][:250], np.zeros(250, np.int64)
    want, want_thr = I.image_maps(dets, annos)
    got, got_thr = pkg.image_maps(dets, annos, per_threshold=True)
    np.testing.assert_array_equal(got_thr, want_thr)
    np.testing.assert_array_equal(got, want)
    assert got[0] > 0.0


def test_no_detections_one_image_and_other_thresholds(gpu_device):
    ann = dict(bboxes=np.array([[0, 0, 10, 10]], np.float32), labels=np.array([1]))
    empty = [np.zeros((0, 5), np.float32)] * 3
    maps, per_thr = pkg.image_maps([empty], [ann], per_threshold=True)                      # N = 1, D = 0
    assert maps.tolist() == [0.0] and per_thr.shape == (10, 1) and not per_thr.any()
    flat = (np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert pkg.image_maps(flat, [ann, ann], num_classes=3).tolist() == [0.0, 0.0]
    hit = [np.zeros((0, 5), np.float32), np.array([[0, 0, 10, 7, 0.5]], np.float32), np.zeros((0, 5), np.float32)]
    maps, per_thr = pkg.image_maps([hit, empty], [ann, dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64))],
                                   iou_thrs=[0.5, np.float64(np.float32(0.7)), 0.7, 0.9], per_threshold=True)
    assert per_thr[:, 0].tolist() == [1.0, 1.0, 0.0, 0.0] and maps.tolist() == [0.5, 0.0]
    assert pkg.bbox_map_eval(hit, ann) == 0.4


def test_a_table_one_element_short_is_refused_with_the_outputs_untouched(gpu_device):
    lib = pkg._lib.lib()
    N, C, T, Dv, G = 2, 1, 2, 3, 2
    P = N * C
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(gpu_device)            # noqa: E731
    tp, fp = t([[1, 0, 1], [0, 0, 1]], np.uint8), t([[0, 1, 0], [1, 1, 0]], np.uint8)
    det_off, gt_off, ign = t([0, 2, 3], np.int64), t([0, 1, 2], np.int64), t([0, 0], np.uint8)
    work = torch.zeros(int(lib.yv4_map_image_ap_work(Dv)), dtype=torch.uint8, device=gpu_device)
    ap = torch.full((T, P), 7.0, dtype=torch.float32, device=gpu_device)
    ngt = torch.full((P,), -5, dtype=torch.int32, device=gpu_device)
    stream = pkg.ops.stream_ptr()

    def call(tpfp=T * Dv, off=P + 1, gts=G, wb=work.numel(), ape=T * P, nge=P):
        return lib.yv4_map_image_ap(tp.data_ptr(), fp.data_ptr(), tpfp, det_off.data_ptr(), gt_off.data_ptr(), off,
                                    ign.data_ptr(), gts, Dv, N, C, T, work.data_ptr(), wb, ap.data_ptr(), ape, ngt.data_ptr(),
                                    nge, stream)
    for short in (dict(tpfp=T * Dv - 1), dict(off=P), dict(wb=4 * Dv - 1), dict(ape=T * P - 1), dict(nge=P - 1), dict(gts=-1)):
        assert call(**short) == -1, short
        assert pkg._lib.lib().yv4_last_error()
    torch.cuda.synchronize()
    assert (ap == 7.0).all() and (ngt == -5).all()
    assert call() == 0
    torch.cuda.synchronize()
    b = lambda row: np.array(row, bool)                                             # noqa: E731
    want = [[I.problem_ap(b([1, 0]), b([0, 1]), 1), I.problem_ap(b([1]), b([0]), 1)],
            [I.problem_ap(b([0, 0]), b([1, 1]), 1), I.problem_ap(b([1]), b([0]), 1)]]
    np.testing.assert_array_equal(ap.cpu().numpy(), np.array(want, np.float32))
    assert ngt.tolist() == [1, 1]
    out_map = torch.full((N,), -1.0, dtype=torch.float64, device=gpu_device)
    out_thr = torch.full((T, N), -1.0, dtype=torch.float32, device=gpu_device)

    def mean(ape=T * P, nge=P, me=N, te=T * N):
        return lib.yv4_map_image_mean(ap.data_ptr(), ape, ngt.data_ptr(), nge, N, C, T, out_map.data_ptr(), me,
                                      out_thr.data_ptr(), te, stream)
    for short in (dict(ape=T * P - 1), dict(nge=P - 1), dict(me=N - 1), dict(te=T * N - 1)):
        assert mean(**short) == -1, short
    torch.cuda.synchronize()
    assert (out_map == -1.0).all() and (out_thr == -1.0).all()
    assert mean() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_thr.cpu().numpy(), np.array(want, np.float32))
    np.testing.assert_array_equal(out_map.cpu().numpy(), [0.5, 1.0])
