"""The proposal recall on the GPU (csrc/recall.hip through recall_eval.py): against the reference-made fixture
(tests/golden/recall.npz) and the numpy restatement (tests/_recall_ref.py, held against the fixture in
tests/test_recall_host.py).  Tolerance: none -- recalls and the recorded IoUs bit for bit.

The kernel has one greedy form (a row is scanned again only when it loses its cached column) and two storage forms:
LDS for a pair with G + c <= the cap, the workspace beyond.  ``lds_cap`` reaches both on the same problems."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd import recall_eval as RE
import _eval_hook_data as DATA
import _recall_ref as RR

pytestmark = pytest.mark.gpu
THRS = np.arange(0.5, 0.96, 0.05)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sorted(ious):
    return -np.sort(-ious, axis=1)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


@pytest.fixture(scope='module')
def sets(golden):
    z = golden('recall')
    return {name: RR.load_set(z, name) for name in RR.SETS}


def _forms(proposals, dev):
    """The input forms a set can take: the reference's arrays; when every image is scored also a per-class split, the
    flat tuple as numpy arrays and as GPU tensors."""
    forms = {'arrays': proposals}
    if all(p.shape[1] == 5 for p in proposals if len(p)):
        five = [p.reshape(-1, 5) if len(p) else np.zeros((0, 5), np.float32) for p in proposals]
        forms['class_lists'] = [[p[0::3], p[1::3], p[2::3]] for p in five]      # three "classes"; scores stay distinct
        flat = RR.flat_form(five)
        forms['flat_numpy'] = flat
        forms['flat_gpu'] = tuple(torch.from_numpy(x).to(dev) for x in flat)
    return forms


@pytest.mark.parametrize('name', RR.SETS)
def test_every_input_form_equals_the_fixture(name, sets, gpu_device):
    gts, proposals, nums, thrs, want, want_ious = sets[name]
    gt = pkg.RecallGt(gts)
    forms = _forms(proposals, gpu_device)
    assert name == 'hand' or len(forms) == 4
    for form, p in forms.items():
        got = pkg.eval_recalls(gts, p, nums, thrs, logger='silent')
        _same(got, want)
        _same(pkg.eval_recalls(gt, p, nums, thrs, logger='silent'), want)          # the cached table
        rec, ious = RE._score(gt, p, nums, thrs, return_ious=True)
        _same(rec, want)
        _same(_bits(_sorted(ious)), _bits(want_ious))
    # a per-class split changes the concatenation order, not the result: the fixture's scores are distinct
    ref, ref_ious = RR.recalls(gts, proposals, nums, thrs, return_ious=True)
    rec, ious = RE._score(gt, proposals, nums, thrs, return_ious=True)
    _same(_bits(ious), _bits(ref_ious))                                             # in recording order too


@pytest.mark.parametrize('name', ['main', 'wide'])
def test_lds_form_and_workspace_form_give_the_same_bytes(name, sets, gpu_device):
    gts, proposals, nums, thrs, want, want_ious = sets[name]
    gt = pkg.RecallGt(gts)
    flat = RR.flat_form(proposals)
    outs = [pkg.recall_device(flat, gt, nums, thrs, return_ious=True, lds_cap=cap) for cap in (0, 1, 100, 5000)]
    for rec, ious in outs:
        _same(rec, want)
        _same(_bits(ious), _bits(outs[0][1]))


def test_a_pair_beyond_the_lds_cap_uses_the_workspace(gpu_device):
    rng = np.random.default_rng(5)
    G, n = 300, 1001                                       # G + min(n, 1000) = 1300 > 1280; beside a small image
    k = np.arange(G)
    gb = np.stack([(k % 20) * 40, (k // 20) * 40, (k % 20) * 40 + 32, (k // 20) * 40 + 32], axis=1).astype(np.float32)
    p = gb[rng.integers(0, G, n)] + rng.integers(-4, 5, (n, 4)).astype(np.float32)
    p = np.concatenate([p, ((rng.permutation(n) + 1) / 2048).astype(np.float32)[:, None]], axis=1)
    assert G + min(n, 1000) > _lib.RECALL_LDS_BOXES
    gts, proposals = [gb[:3], gb], [p[:40], p]
    want, want_ious = RR.recalls(gts, proposals, [64, 1000], THRS, return_ious=True)
    rec, ious = RE._score(pkg.RecallGt(gts), proposals, [64, 1000], THRS, return_ious=True)
    _same(rec, want)
    _same(_bits(ious), _bits(want_ious))
    assert (want_ious[1] >= 0.5).sum() > 100


def _tables(gts, proposals, dev):
    gt = pkg.RecallGt(gts)
    vis = [RR.visiting_order(p) for p in proposals]
    det4 = np.concatenate([np.zeros((0, 4), np.float32)] + vis, axis=0)
    det_off = np.concatenate([[0], np.cumsum([len(v) for v in vis])]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    return gt, t(det4), t(det_off), t(gt.gt), t(gt.gt_off), len(det4)


def test_the_seam_writes_inside_its_outputs_and_twice_the_same(sets, gpu_device):
    gts, proposals, nums, thrs, want, want_ious = sets['wide']
    gt, det4, det_off, gt4, gt_off, D = _tables(gts, proposals, gpu_device)
    N, G, M, T = gt.num_imgs, gt.total_gt, len(nums), len(thrs)
    lib = _lib.lib()
    h_nums = np.array(nums, np.int32)
    t_thr = torch.from_numpy(thrs).to(gpu_device)
    need = int(lib.yv4_recall_work(D, G, N, M))
    pad = 64

    def run(with_ious, cap):
        work = torch.full((need + 2 * pad,), 0x5A, dtype=torch.uint8, device=gpu_device)
        ious = torch.full((M * G * 4 + 2 * pad,), 0x5A, dtype=torch.uint8, device=gpu_device)
        counts = torch.full((M * T * 8 + 2 * pad,), 0x5A, dtype=torch.uint8, device=gpu_device)
        rc = lib.yv4_recall_match(det4.data_ptr(), det_off.data_ptr(), gt4.data_ptr(), gt_off.data_ptr(), N + 1, N, D, G,
                                  h_nums.ctypes.data, M, t_thr.data_ptr(), T, float(np.float32(1e-6)), cap,
                                  work[pad:].data_ptr(), need, ious[pad:].data_ptr() if with_ious else None, M * G,
                                  counts[pad:].data_ptr(), M * T, None)
        assert rc == 0, lib.yv4_last_error()
        torch.cuda.synchronize()
        for buf in (work, ious, counts):
            b = buf.cpu().numpy()
            assert (b[:pad] == 0x5A).all() and (b[-pad:] == 0x5A).all()
        if not with_ious:
            assert (ious.cpu().numpy() == 0x5A).all()
        c = counts.cpu().numpy()[pad:-pad].copy().view(np.int64).reshape(M, T)
        v = ious.cpu().numpy()[pad:-pad].copy().view(np.float32).reshape(M, G)
        return c, v

    c0, v0 = run(True, 0)
    _same(c0 / float(G), want)
    _same(_bits(_sorted(v0)), _bits(want_ious))
    for with_ious, cap in ((True, 0), (False, 0), (True, 1), (False, 1)):
        c, v = run(with_ious, cap)
        _same(c, c0)                                       # counts: identical across runs, forms and without gt_ious
        if with_ious:
            _same(_bits(v), _bits(v0))


def test_equal_scores_keep_the_input_order_at_the_top_n_cut(gpu_device):
    gts = [np.array([[0, 0, 10, 10], [20, 0, 30, 10]], np.float32)]
    # four boxes share the score 0.5; the cut at 2 falls inside them
    p = np.array([[20, 0, 30, 9, 0.9], [0, 0, 10, 5, 0.5], [0, 0, 10, 10, 0.5], [0, 0, 10, 8, 0.5], [20, 0, 30, 10, 0.5],
                  [0, 0, 10, 9, 0.25]], np.float32)
    for order in (np.arange(6), np.array([0, 2, 1, 3, 4, 5]), np.array([5, 4, 3, 2, 1, 0]), np.array([3, 5, 1, 0, 4, 2])):
        q = p[order]
        want, want_ious = RR.recalls(gts, [q], [1, 2, 3, 6], THRS, return_ious=True)
        for form in ([q], RR.flat_form([q]), tuple(torch.from_numpy(x).to(gpu_device) for x in RR.flat_form([q])),
                     [[q[:2], q[2:]]]):
            rec, ious = RE._score(pkg.RecallGt(gts), form, [1, 2, 3, 6], THRS, return_ious=True)
            _same(rec, want)
            _same(_bits(ious), _bits(want_ious))
    a = RR.gt_ious(gts, [p], [2])
    b = RR.gt_ious(gts, [p[[0, 2, 1, 3, 4, 5]]], [2])
    assert a.tolist() != b.tolist()                         # the order of the tied rows decides the top-2
    # -0 and +0 are one score: their input order stays
    z = np.array([[0, 0, 10, 6, 0.0], [0, 0, 10, 10, -0.0]], np.float32)
    rec, ious = RE._score(pkg.RecallGt(gts), [z], [1], [0.5], return_ious=True)
    assert ious[0, 0] == np.float32(0.6)


def test_mixed_and_scoreless_lists(gpu_device):
    gts = [np.array([[0, 0, 10, 10]], np.float32), np.array([[0, 0, 10, 10], [50, 50, 60, 60]], np.float32), None]
    proposals = [np.array([[0, 0, 10, 4], [0, 0, 10, 9]], np.float32),
                 np.array([[50, 50, 60, 58, 0.1], [0, 0, 10, 7, 0.9], [0, 0, 10, 10, 0.1]], np.float32),
                 np.zeros((0, 5), np.float32)]
    want, want_ious = RR.recalls(gts, proposals, [1, 2, 5], THRS, return_ious=True)
    rec, ious = RE._score(pkg.RecallGt(gts), proposals, [1, 2, 5], THRS, return_ious=True)
    _same(rec, want)
    _same(_bits(ious), _bits(want_ious))
    assert want_ious[0].tolist() == [np.float32(0.4), np.float32(0.7), -1.0]


def test_empty_sides_and_one_image(gpu_device, capsys):
    g1 = [np.array([[0, 0, 10, 10], [20, 20, 30, 30]], np.float32)]
    none = [np.zeros((0, 5), np.float32)]
    # total_det == 0: G zeros per number, which reach no positive threshold and every threshold <= 0
    rec, ious = RE._score(pkg.RecallGt(g1), none, [1, 10], [0.0, 0.5], return_ious=True)
    _same(rec, np.array([[1.0, 0.0], [1.0, 0.0]]))
    _same(ious, np.zeros((2, 2), np.float32))
    _same(pkg.eval_recalls(g1, RR.flat_form(none), [1, 10], [0.0, 0.5], logger='silent'), rec)
    # total_gt == 0: nan, with numpy's warning, as the reference
    p1 = [np.array([[0, 0, 10, 9, 0.5]], np.float32)]
    for g in ([None], [np.zeros((0, 4), np.float32)]):
        with pytest.warns(RuntimeWarning):
            rec = pkg.eval_recalls(g, p1, [1], [0.5], logger='silent')
        assert rec.shape == (1, 1) and np.isnan(rec).all()
    # N == 1, and the summary is printed unless silenced
    rec = pkg.eval_recalls(g1, p1, [1], [0.5, 0.95])
    _same(rec, np.array([[0.5, 0.0]]))
    assert '0.500' in capsys.readouterr().out
    # a row whose image index is outside [0, N) takes no part
    flat = (np.array([[0, 0, 10, 10, 0.9], [20, 20, 30, 30, 0.8], [0, 0, 10, 9, 0.5]], np.float32), np.zeros(3, np.int64),
            np.array([1, -1, 0], np.int64))
    _same(pkg.eval_recalls(g1, flat, [3], [0.5], logger='silent'), np.array([[0.5]]))
    with pytest.raises(ValueError, match='proposal numbers'):
        pkg.eval_recalls(g1, p1, list(range(17)), [0.5], logger='silent')
    with pytest.raises(AssertionError):
        pkg.eval_recalls(g1, p1 + p1, [1], [0.5], logger='silent')


def _coco(gts, num_cls):
    """Per image (boxes, labels) -> a COCO dict with one crowd and one ignored box added to image 0."""
    anns = []
    for i, (b, lab) in enumerate(gts):
        for box, c in zip(b, lab):
            anns.append(dict(id=len(anns) + 1, image_id=100 + i, category_id=c + 1, iscrowd=0,
                             bbox=[float(box[0]), float(box[1]), float(box[2] - box[0]), float(box[3] - box[1])],
                             area=float((box[2] - box[0]) * (box[3] - box[1]))))
    anns.append(dict(id=len(anns) + 1, image_id=100, category_id=1, iscrowd=1, bbox=[1.0, 1.0, 50.0, 50.0], area=2500.0))
    anns.append(dict(id=len(anns) + 1, image_id=100, category_id=1, iscrowd=0, ignore=True, bbox=[2.0, 2.0, 40.0, 40.0],
                     area=1600.0))
    return dict(images=[dict(id=100 + i) for i in range(len(gts))],
                categories=[dict(id=c + 1, name=f'c{c}') for c in range(num_cls)], annotations=anns)


def test_coco_dataset_scores_proposal_fast(gpu_device, capsys):
    rng = np.random.default_rng(3)
    num_cls, gts, results = 3, [], []
    for i in range(6):
        g = int(rng.integers(1, 6)) if i != 4 else 0
        b = np.round(np.concatenate([rng.uniform(0, 200, (g, 2)), rng.uniform(20, 90, (g, 2))], 1)).astype(np.float32)
        b[:, 2:] += b[:, :2]
        lab = rng.integers(0, num_cls, g)
        gts.append((b, lab))
        per_cls = []
        for c in range(num_cls):
            mine = b[lab == c]
            d = np.concatenate([mine + rng.integers(-6, 7, mine.shape).astype(np.float32),
                                mine + rng.integers(-20, 21, mine.shape).astype(np.float32)], 0)
            per_cls.append(np.concatenate([d, rng.random((len(d), 1), dtype=np.float32)], 1).astype(np.float32))
        results.append(per_cls)
    ds = pkg.CocoBBoxDataset(_coco(gts, num_cls))
    plain = [b for b, _ in gts]
    nums = (1, 3, 100)
    want = RR.recalls(plain, RR.concat_classes(results), nums, np.linspace(.5, 0.95, 10)).mean(axis=1)
    assert 0 < want[0] < want[2]
    ar = ds.fast_eval_recall(results, nums, np.linspace(.5, 0.95, 10), logger='silent')
    _same(ar, want)
    out = ds.evaluate(results, metric='proposal_fast', logger='silent', proposal_nums=nums)
    assert list(out) == ['AR@1', 'AR@3', 'AR@100'] and [out[k] for k in out] == want.tolist()
    flat = tuple(torch.from_numpy(x).to(gpu_device) for x in pkg.flatten_results(results))
    assert [v for v in ds.evaluate(flat, metric='proposal_fast', logger='silent', proposal_nums=nums).values()] == want.tolist()
    assert ds.recall_gt() is ds.recall_gt()
    capsys.readouterr()
    ds.evaluate(results, metric='proposal_fast', proposal_nums=nums)
    text = capsys.readouterr().out
    assert 'Evaluating proposal_fast...' in text and f'AR@100\t{want[2]:.4f}' in text and '+--' not in text
    # a list: the metrics keep their order and merge; bbox's numbers are the ones bbox alone gives
    bbox = ds.evaluate(results, metric='bbox', logger='silent', proposal_nums=nums)
    both = ds.evaluate(results, metric=['bbox', 'proposal_fast'], logger='silent', proposal_nums=nums)
    assert list(both) == list(bbox) + ['AR@1', 'AR@3', 'AR@100']
    assert all(both[k] == bbox[k] for k in bbox) and [both[f'AR@{n}'] for n in nums] == want.tolist()
    other = ds.evaluate(results, metric=['proposal_fast', 'bbox'], logger='silent', proposal_nums=nums)
    assert list(other) == ['AR@1', 'AR@3', 'AR@100'] + list(bbox)
    # the defaults: (100, 300, 1000) and COCO's ten thresholds
    assert list(ds.evaluate(results, metric='proposal_fast', logger='silent')) == ['AR@100', 'AR@300', 'AR@1000']


def test_custom_dataset_eval_recalls(sets, gpu_device):
    gts, proposals, nums, thrs, want, _ = sets['main']
    annos = [dict(bboxes=np.zeros((0, 4), np.float32) if g is None else g, labels=np.zeros(0 if g is None else len(g), np.int64))
             for g in gts]
    ds = pkg.CustomBBoxDataset(annos, ('a',))
    out = ds.eval_recalls(proposals, proposal_nums=tuple(nums), iou_thr=[0.5, 0.75], logger='silent')
    ref = RR.recalls(gts, proposals, nums, [0.5, 0.75])
    assert list(out) == [f'recall@{n}@{t}' for n in nums for t in (0.5, 0.75)] + [f'AR@{n}' for n in nums]
    assert [out[f'recall@{n}@0.5'] for n in nums] == ref[:, 0].tolist() == want[:, 0].tolist()
    assert [out[f'AR@{n}'] for n in nums] == ref.mean(axis=1).tolist()
    one = ds.eval_recalls(proposals, proposal_nums=(10,), logger='silent')
    assert list(one) == ['recall@10@0.5'] and one['recall@10@0.5'] == want[1, 0]


def test_eval_hook_scores_proposal_fast_from_both_loops(gpu_device, tmp_path):
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
    want = ds.evaluate(lists, metric='proposal_fast', logger='silent')
    assert list(want) == ['AR@100', 'AR@300', 'AR@1000'] and 0 < want['AR@100'] <= 1
    del received[:]
    outs = []
    for n, kw in enumerate((dict(), dict(flat=False))):
        work_dir = tmp_path / str(n)
        work_dir.mkdir()
        runner = H.Runner(det, None, max_epochs=1, work_dir=str(work_dir))
        hook = H.EvalHook(loader, interval=1, metric='proposal_fast', save_best='AR@100', **kw)
        assert hook.rule == 'greater'                      # greater_keys holds 'AR'
        hook.before_run(runner)
        runner.meta['hook_msgs']['last_ckpt'] = str(work_dir / 'epoch_1.pth')       # (what a CheckpointHook leaves)
        hook.after_train_epoch(runner)
        outs.append(dict(runner.log_buffer.output))
        assert runner.meta['hook_msgs']['best_score'] == want['AR@100']
        assert (work_dir / 'best_AR@100.pth').is_symlink()
    assert isinstance(received[0], tuple) and all(t.is_cuda for t in received[0])      # flat by default
    assert isinstance(received[1], list)
    assert outs[0]['AR@100'] == outs[1]['AR@100'] == want['AR@100']
