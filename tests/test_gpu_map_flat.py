"""VOC-style mAP from the flat GPU table (yv4_map_rank -> yv4_bbox_overlaps_batched -> yv4_tpfp_batched ->
yv4_map_accumulate) against the reference-made fixture, against the list path where no two detections of a class share
a score, and against the numpy restatement of the flat definition (tests/_map_flat_ref.py, which
tests/test_map_flat_host.py holds against the same fixture) where ties and the kernels' thread maps are the point.
Tolerance: none -- every comparison is exact, dtypes included."""
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd.coco_eval import flatten_results
import _map_flat_ref as F
from _map_data import CASES, SCALE_RANGES, assert_result_equals_fixture, boxes, load_dataset, without_detections

pytestmark = pytest.mark.gpu

THRS10 = [0.5 + 0.05 * x for x in range(10)]
#: detections per class of the thread-map set: around a wave (64), a workgroup's chunk (256), four chunks, and many
EDGE_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5003]
EDGE_IMGS = 4
ONE_GT_CLASS, MANY_GT_CLASS = 8, 11


@pytest.fixture(scope='module')
def z(golden):
    return golden('map_eval')


@pytest.fixture(scope='module')
def data(z):
    return load_dataset(z)


def _gpu(flat, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in flat)


def _same_results(got, want):
    (ma, ra), (mb, rb) = got, want
    assert type(ma) is type(mb) and np.array_equal(np.asarray(ma), np.asarray(mb)), (ma, mb)
    assert len(ra) == len(rb)
    for c, (a, b) in enumerate(zip(ra, rb)):
        assert a.keys() == b.keys()
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (c, k)


def _last_points(results):
    """What curves=False returns, from full curves."""
    out = []
    for r in results:
        r = dict(r)
        r['recall'], r['precision'] = r['recall'][..., -1:], r['precision'][..., -1:]
        out.append(r)
    return out


# ---- against the reference-made fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_flat_gpu_tensors_reproduce_the_fixture(gpu_device, z, data, name):
    dets, annos = data
    flat = _gpu(flatten_results(without_detections(dets) if name == 'empty' else dets), gpu_device)
    gt = pkg.MapGt(annos, 6)
    mean_ap, results = pkg.eval_map(flat, gt, curves=True, logger='silent', **CASES[name])
    assert_result_equals_fixture(z, name, mean_ap, results)
    # the default: the curves' last points only; lists of annotations with the class count; numpy input
    for res, ann, kw in ((flat, annos, dict(num_classes=6)), (tuple(t.cpu().numpy() for t in flat), gt, {})):
        m2, r2 = pkg.eval_map(res, ann, logger='silent', **kw, **CASES[name])
        _same_results((m2, r2), (mean_ap, _last_points(results)))
    assert set(gt._device) == {(gpu_device.type, gpu_device.index)}      # one device copy, kept


def test_evaluate_map_takes_the_flat_table(gpu_device, data, capsys):
    dets, annos = data
    names = [f'c{i}' for i in range(6)]
    ds = pkg.CustomBBoxDataset(annos, names)
    want = pkg.evaluate_map(dets, annos, classes=names, iou_thr=[0.5, 0.7], logger='silent')
    got = ds.evaluate(_gpu(flatten_results(dets), gpu_device), iou_thr=[0.5, 0.7], logger='silent')
    assert list(got) == ['AP50', 'AP70', 'mAP'] and got.keys() == want.keys()
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert ds.evaluate(dets, logger='silent') == ds.evaluate(flatten_results(dets), logger='silent')
    assert capsys.readouterr().out == ''
    ds.evaluate(_gpu(flatten_results(dets), gpu_device))          # the summary table prints from the last points
    out = capsys.readouterr().out
    assert '| c5 ' in out and '| mAP' in out


# ---- flat == list where no two detections of a class share a score ------------------------------------------------------
def _random_set(rng, num_img, num_cls, max_det):
    dets, annos = [], []
    for i in range(num_img):
        ng = int(rng.integers(0, 12)) if i % 9 else 0
        gb, gl = boxes(rng, ng), rng.integers(0, num_cls, ng)
        ign = rng.random(ng) < 0.2
        anno = dict(bboxes=gb[~ign], labels=gl[~ign].astype(np.int64))
        if i % 3:
            anno.update(bboxes_ignore=gb[ign], labels_ignore=gl[ign].astype(np.int64))
        per_cls = []
        for c in range(num_cls):
            n = int(rng.integers(0, max_det + 1)) if (i + c) % 5 else 0
            d = boxes(rng, n)
            mine = gb[gl == c]
            if len(mine) and n:
                near = rng.random(n) < 0.7
                d[near] = (mine[rng.integers(0, len(mine), n)] + rng.normal(0, 5, (n, 4)).astype(np.float32))[near]
            per_cls.append(d)
        dets.append(per_cls)
        annos.append(anno)
    for c in range(num_cls):                                     # distinct scores within the class
        n = sum(len(d[c]) for d in dets)
        sc = (rng.choice(1 << 16, size=n, replace=False) / float(1 << 16)).astype(np.float32)
        lo = 0
        for d in dets:
            m = len(d[c])
            d[c] = np.concatenate([d[c], sc[lo:lo + m, None]], 1).astype(np.float32)
            lo += m
    return dets, annos


@pytest.fixture(scope='module')
def tie_free():
    dets, annos = _random_set(np.random.default_rng(21), 40, 5, 70)
    for c in range(5):
        sc = np.concatenate([d[c][:, 4] for d in dets])
        assert len(np.unique(sc)) == len(sc) > 768               # distinct, and more than three chunks per class
    assert 60 <= max(len(d[c]) for d in dets for c in range(5)) <= 70
    return dets, annos


@pytest.mark.parametrize('dataset', [None, 'det', 'voc07'])
def test_flat_equals_the_list_path_without_ties(gpu_device, tie_free, dataset):
    dets, annos = tie_free
    kw = dict(scale_ranges=SCALE_RANGES, iou_thr=THRS10, dataset=dataset, logger='silent')
    want = pkg.eval_map(dets, annos, **kw)
    got = pkg.eval_map(_gpu(flatten_results(dets), gpu_device), annos, num_classes=5, curves=True, **kw)
    assert len(got) == len(want) == 10
    for g, w in zip(got, want):
        _same_results(g, w)
    assert any(r['ap'].max() > 0 for _, res in want for r in res)
    one = pkg.eval_map(_gpu(flatten_results(dets), gpu_device), annos, num_classes=5, curves=True, iou_thr=0.5,
                       dataset=dataset, logger='silent')
    _same_results(one, pkg.eval_map(dets, annos, iou_thr=0.5, dataset=dataset, logger='silent'))


@pytest.mark.parametrize('rule', ['default', 'imagenet'])
def test_order_of_the_flat_table_does_not_matter_without_ties(gpu_device, tie_free, rule):
    dets, annos = tie_free
    flat = flatten_results(dets)
    perm = np.random.default_rng(2).permutation(len(flat[0]))
    fn = pkg.tpfp_imagenet if rule == 'imagenet' else pkg.tpfp_default
    kw = dict(num_classes=5, curves=True, scale_ranges=SCALE_RANGES, iou_thr=[0.5, 0.75], tpfp_fn=fn, logger='silent')
    a = pkg.eval_map(_gpu(flat, gpu_device), annos, **kw)
    b = pkg.eval_map(_gpu(tuple(x[perm] for x in flat), gpu_device), annos, **kw)
    for x, y in zip(a, b):
        _same_results(x, y)


# ---- heavy ties: the stable order is the definition --------------------------------------------------------------------------
@pytest.mark.parametrize('rule', ['default', 'imagenet'])
def test_heavy_ties_follow_the_stable_order(gpu_device, rule):
    rng = np.random.default_rng(33)
    dets, annos = _random_set(rng, 12, 4, 40)
    flat = list(flatten_results(dets))
    flat[0] = flat[0].copy()
    flat[0][:, 4] = np.round(flat[0][:, 4] * 11) / 11            # a dozen score values
    flat[0][::17, 4] *= 0                                        # and zeros of both signs
    flat[0][::34, 4] = -0.0
    assert len(np.unique(flat[0][:, 4])) <= 12
    perm = rng.permutation(len(flat[0]))                         # ties then fall by table position, not by image
    flat = tuple(x[perm] for x in flat)
    fn, ref = (pkg.tpfp_imagenet, F.R.tpfp_imagenet) if rule == 'imagenet' else (pkg.tpfp_default, F.R.tpfp_default)
    got = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=4, curves=True, scale_ranges=SCALE_RANGES,
                       iou_thr=[0.5, 0.7], tpfp_fn=fn, logger='silent')
    for g, thr in zip(got, (0.5, 0.7)):
        _same_results(g, F.eval_map_flat(flat, annos, 4, scale_ranges=SCALE_RANGES, iou_thr=thr, rule=ref))
    got = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=4, curves=True, iou_thr=0.5, tpfp_fn=fn, dataset='voc07',
                       logger='silent')
    _same_results(got, F.eval_map_flat(flat, annos, 4, iou_thr=0.5, rule=ref, dataset='voc07'))


# ---- the thread maps: waves, chunks, carries --------------------------------------------------------------------------------
def _edge_set():
    """EDGE_COUNTS detections per class over EDGE_IMGS images.  In every class the best-scored third is clutter (false
    positives first) and the gts' copies follow (true positives late): precision rises again and again, so the suffix
    maximum and the counts must cross every wave and chunk border.  Class ONE_GT_CLASS: image 0 holds one gt and 600
    detections on it; class MANY_GT_CLASS: more gts per image than a wave has lanes.  Rows with labels / image indices
    out of range are mixed in with the best scores of all; the table is shuffled."""
    rng = np.random.default_rng(77)
    C, N = len(EDGE_COUNTS), EDGE_IMGS
    gts = [[None] * C for _ in range(N)]
    rows, labels, imgs = [], [], []
    for c, n in enumerate(EDGE_COUNTS):
        for i in range(N):
            ng = max(2, n // 32)
            if c == ONE_GT_CLASS and i == 0:
                ng = 1
            gts[i][c] = boxes(rng, ng)
        assert c != MANY_GT_CLASS or len(gts[1][c]) > 64
        vals = np.sort(rng.choice(1 << 20, size=n, replace=False))[::-1] / float(1 << 20)      # exact in float32
        early = n // 3
        late = rng.permutation(vals[early:])
        for j in range(n):
            if j < early or rng.random() < 0.1:
                i, b = int(rng.integers(0, N)), boxes(rng, 1)[0]
            else:
                i = 0 if (c == ONE_GT_CLASS and j - early < 600) else int(rng.integers(0, N))
                g = gts[i][c]
                b = g[rng.integers(0, len(g))] + rng.normal(0, 2.5, 4).astype(np.float32)
            rows.append(np.append(b, vals[j] if j < early else late[j - early]))
            labels.append(c)
            imgs.append(i)
    for lab, im in ((-1, 0), (C, 1), (C + 7, 2), (0, -1), (3, N), (5, N + 3), (-4, -4)):
        for _ in range(3):
            rows.append(np.append(boxes(rng, 1)[0], 2.0))
            labels.append(lab)
            imgs.append(im)
    annos = []
    for i in range(N):
        lab = np.concatenate([np.full(len(gts[i][c]), c) for c in range(C)]).astype(np.int64)
        box = np.concatenate(gts[i])
        ign = rng.random(len(lab)) < 0.05
        ign[lab == ONE_GT_CLASS] = False
        annos.append(dict(bboxes=box[~ign], labels=lab[~ign], bboxes_ignore=box[ign], labels_ignore=lab[ign]))
    perm = rng.permutation(len(rows))
    flat = (np.array(rows, np.float32)[perm], np.array(labels, np.int64)[perm], np.array(imgs, np.int64)[perm])
    return flat, annos


@pytest.fixture(scope='module')
def edge():
    flat, annos = _edge_set()
    C = len(EDGE_COUNTS)
    want = {rule: [F.eval_map_flat(flat, annos, C, scale_ranges=SCALE_RANGES, iou_thr=thr,
                                   rule=getattr(F.R, 'tpfp_' + rule)) for thr in (0.5, 0.75)]
            for rule in ('default', 'imagenet')}
    want['voc07'] = F.eval_map_flat(flat, annos, C, iou_thr=0.5, dataset='voc07')
    return flat, annos, want


def test_edge_set_is_what_it_claims(edge):
    flat, annos, want = edge
    part, key = F.problem_keys(flat[1], flat[2], EDGE_IMGS, len(EDGE_COUNTS))
    assert (~part).sum() == 21
    assert np.bincount(flat[1][part], minlength=len(EDGE_COUNTS)).tolist() == EDGE_COUNTS
    assert np.bincount(key[part]).max() >= 600
    res = want['voc07'][1]
    for c, n in enumerate(EDGE_COUNTS):
        assert res[c]['num_dets'] == n
        if n < 63:
            continue
        p, r = res[c]['precision'], res[c]['recall']
        assert (np.diff(p) > 0).any() and (np.diff(p) < 0).any()                 # not monotone
        if n >= 1023:
            steps = np.flatnonzero(np.diff(np.concatenate([[0.], r])) > 0)       # true positives
            first = n // 3
            assert (steps >= first).mean() > 0.85                                # false positives first, true positives late
            chunks = np.unique(steps // 256)
            assert set(range(first // 256 + 1, (n - 1) // 256)) <= set(chunks.tolist())   # a true positive in every later chunk
            assert p[first:].max() > p[:first].max()                             # the maximum comes from behind


@pytest.mark.parametrize('rule', ['default', 'imagenet'])
def test_thread_map_edges_equal_the_restatement(gpu_device, edge, rule):
    flat, annos, want = edge
    C = len(EDGE_COUNTS)
    fn = pkg.tpfp_imagenet if rule == 'imagenet' else pkg.tpfp_default
    got = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=C, curves=True, scale_ranges=SCALE_RANGES,
                       iou_thr=[0.5, 0.75], tpfp_fn=fn, logger='silent')
    for g, w in zip(got, want[rule]):
        _same_results(g, w)
    if rule == 'default':
        got = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=C, curves=True, iou_thr=0.5, dataset='voc07',
                           logger='silent')
        _same_results(got, want['voc07'])
        last = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=C, iou_thr=0.5, dataset='voc07', logger='silent')
        _same_results(last, (want['voc07'][0], _last_points(want['voc07'][1])))


def test_two_runs_give_identical_bytes(gpu_device, edge):
    from mmdet_yolov4_amd import _lib, map_eval as ME
    flat, annos, _ = edge
    gt = pkg.MapGt(annos, len(EDGE_COUNTS))
    area = [(lo ** 2, hi ** 2) for lo, hi in SCALE_RANGES]
    for mode, ap_mode in ((_lib.TPFP_DEFAULT, 'area'), (_lib.TPFP_IMAGENET, '11points')):
        runs = [ME.map_flat_device(_gpu(flat, gpu_device), gt, mode, THRS10, area, ap_mode, curves=True) for _ in range(2)]
        for k in ('ap', 'last_recall', 'last_precision', 'num_dets', 'recall', 'precision', 'cls_off'):
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
        assert runs[0]['ap'].shape == (10, len(EDGE_COUNTS), 3) and runs[0]['total_det'] == sum(EDGE_COUNTS)


def test_one_problem_and_no_detections(gpu_device):
    rng = np.random.default_rng(5)
    gt = boxes(rng, 3)
    det = np.concatenate([gt[[1, 1, 0]] + np.float32(1), boxes(rng, 2)])
    det = np.concatenate([det, np.array([[.9], [.8], [.8], [.7], [.95]], np.float32)], 1).astype(np.float32)
    annos = [dict(bboxes=gt, labels=np.zeros(3, np.int64))]
    flat = (det, np.zeros(5, np.int64), np.zeros(5, np.int64))
    for kw in (dict(), dict(scale_ranges=SCALE_RANGES), dict(dataset='det'), dict(dataset='voc07')):
        got = pkg.eval_map(_gpu(flat, gpu_device), annos, num_classes=1, curves=True, logger='silent', **kw)
        _same_results(got, F.eval_map_flat(flat, annos, 1, **kw))
    assert got[1][0]['num_dets'] == 5 and got[0] > 0
    none = (np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    annos3 = annos + [dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64))]
    for res in (none, _gpu(none, gpu_device), (det, np.full(5, 9, np.int64), np.zeros(5, np.int64))):   # D = 0; no row takes part
        for kw in (dict(), dict(scale_ranges=SCALE_RANGES, iou_thr=[0.5, 0.6]), dict(dataset='voc07')):
            for curves in (False, True):
                got = pkg.eval_map(res, annos3, num_classes=2, curves=curves, logger='silent', **kw)
                want = [F.eval_map_flat(none, annos3, 2, **dict(kw, iou_thr=t)) for t in kw.get('iou_thr', [0.5])]
                for g, w in zip(got if isinstance(got, list) else [got], want):
                    _same_results(g, w)
                    assert all(r['num_dets'] == 0 and r['recall'].shape[-1] == 0 for r in g[1])


# ---- through the hooks ---------------------------------------------------------------------------------------------------------
def test_eval_hook_scores_map_on_the_flat_loop(gpu_device, tmp_path):
    import _eval_hook_data as DATA
    det = DATA.tiny_v4(DATA.make_test_cfg(), gpu_device)
    pipe = pkg.FusedTestPipeline(img_scale=(128, 128), device=gpu_device)
    imgs = DATA.images()
    DATA.lift_head(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    lists = pkg.single_gpu_test(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    rng = np.random.default_rng(4)
    annos = []
    for res in lists:                                            # its first two detections, and a box that matches nothing
        rows = [(c, r) for c, arr in enumerate(res) for r in arr][:2]
        b = np.array([r[:4] for _, r in rows] + [[1, 1, 9, 7]], np.float32).reshape(-1, 4)
        annos.append(dict(bboxes=b, labels=np.array([c for c, _ in rows] + [int(rng.integers(0, DATA.NUM_CLASSES))], np.int64)))

    class Recording(pkg.CustomBBoxDataset):
        received = None

        def evaluate(self, results, **kw):
            self.received = results
            return super().evaluate(results, **kw)
    ds = Recording(annos, [f'c{c}' for c in range(DATA.NUM_CLASSES)])
    loader = DATA.Loader(pipe, imgs, range(DATA.SIZE), dataset=ds)
    outs = {}
    for flat in (None, False):
        work = tmp_path / str(flat)
        os.makedirs(work)
        runner = H.Runner(det, None, max_epochs=1, work_dir=str(work))
        hook = H.EvalHook(loader, interval=1, save_best='mAP', flat=flat, iou_thr=[0.5, 0.75])
        assert hook.use_flat() is (flat is None)
        hook.before_run(runner)
        H.CheckpointHook(interval=1, save_optimizer=False).after_train_epoch(runner)
        hook.after_train_epoch(runner)
        if flat is None:
            assert isinstance(ds.received, tuple) and all(t.is_cuda for t in ds.received)
            for got, ref in zip(ds.received, flatten_results(lists)):
                assert np.array_equal(got.cpu().numpy(), ref)
        else:
            assert isinstance(ds.received, list)
        out = dict(runner.log_buffer.output)
        assert runner.log_buffer.ready and list(out) == ['AP50', 'AP75', 'mAP'] and out['AP50'] > 0
        msgs = runner.meta['hook_msgs']
        assert msgs['best_score'] == out['mAP'] and os.path.isfile(msgs['best_ckpt'])
        link = work / 'best_mAP.pth'
        assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(msgs['best_ckpt'])
        outs[flat] = out
    assert outs[None] == outs[False]
