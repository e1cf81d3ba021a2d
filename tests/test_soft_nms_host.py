"""Soft-NMS without a GPU: the restatement's two forms against each other and against hand-derived cases, the exported
symbols, the C entry points' argument checks and batched_nms' dispatch errors."""
import ctypes

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
import _soft_nms_ref as R

L = pkg._lib


def _problem(n, seed, ties=False, negative=False):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-60 if negative else 0, 200, (n, 2)).astype(np.float32)
    wh = rng.uniform(4, 60, (n, 2)).astype(np.float32)
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    s = rng.uniform(0, 1, n).astype(np.float32)
    if ties:
        s[::4] = 0.5
    return b, s


@pytest.mark.parametrize('method', ['naive', 'linear', 'gaussian'])
@pytest.mark.parametrize('n,seed,ties', [(1, 0, False), (2, 1, False), (17, 2, True), (64, 3, False), (150, 4, True)])
def test_fast_form_equals_the_literal_loop(method, n, seed, ties):
    b, s = _problem(n, seed, ties)
    for min_score in (1e-3, 0.2):
        d0, i0 = R.soft_nms_loop(b, s, 0.3, 0.5, min_score, method)
        d1, i1 = R.soft_nms_fast(b, s, 0.3, 0.5, min_score, method)
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(d0, d1)
        assert (np.diff(d0[:, 4]) <= 0).all()               # selection order: non-increasing scores


def test_compaction_rule_against_the_end_swaps():
    """The literal end swaps of one step (scan left to right, pull from the end, re-examine) against the rule."""
    rng = np.random.default_rng(7)
    for _ in range(500):
        nb = int(rng.integers(2, 40))
        i = int(rng.integers(0, nb - 1))
        disc = np.zeros(nb, bool)
        disc[i + 1:] = rng.random(nb - i - 1) < rng.random()
        arr = list(range(nb))
        flag = list(disc)
        pos, end = i + 1, nb
        while pos < end:
            if flag[pos]:
                arr[pos], flag[pos] = arr[end - 1], flag[end - 1]
                end -= 1
                continue
            pos += 1
        got = R.compact(np.arange(nb), disc, nb)
        assert end == got.shape[0]
        np.testing.assert_array_equal(np.asarray(arr[:end]), got)


def test_definition_cases():
    b = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [100, 100, 110, 110]], np.float32)
    # the first winner is never compared with min_score: everything below it -> exactly one box
    d, i = R.soft_nms_loop(b, np.array([1e-4, 2e-4, 5e-5], np.float32), min_score=1e-3)
    np.testing.assert_array_equal(i, [1])
    # naive with min_score 0 keeps the suppressed box with score 0
    d, i = R.soft_nms_loop(b, np.array([0.9, 0.8, 0.7], np.float32), 0.5, method='naive', min_score=0.0)
    np.testing.assert_array_equal(i, [0, 2, 1])
    np.testing.assert_array_equal(d[:, 4], np.array([0.9, 0.7, 0.0], np.float32))
    # an exact tie goes to the lower current position
    d, i = R.soft_nms_loop(b, np.array([0.5, 0.5, 0.5], np.float32), 0.9, method='linear')
    assert i[0] == 0 and i[1] == 2
    # IoU exactly at the threshold decays (>=): boxes 10x10 and 10x5 overlap 50 -> IoU = 0.5 in fp32
    bb = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], np.float32)
    d, i = R.soft_nms_loop(bb, np.array([0.9, 0.8], np.float32), 0.5, method='linear')
    assert d[1, 4] == np.float32(0.8) * (np.float32(1) - np.float32(0.5))


def test_split_branch_resorts_by_the_decayed_scores():
    b, s = _problem(300, 11)
    idx = np.arange(300) % 3
    d, k = R.batched_soft_nms(b, s, idx, dict(type='soft_nms', iou_threshold=0.3, split_thr=10))
    assert (np.diff(d[:, 4]) <= 0).all()
    d2, k2 = R.batched_soft_nms(b, s, idx, dict(type='soft_nms', iou_threshold=0.3, split_thr=10, max_num=7))
    np.testing.assert_array_equal(k2, k[:7])
    with pytest.raises(TypeError):
        R.batched_soft_nms(b, s, idx, dict(type='soft_nms', iou_threshold=0.3, max_num=7))


def test_symbols_and_constants():
    assert L.FEATURES['soft_nms'].symbols <= set(L.SIGNATURES)
    assert L.has('soft_nms')
    assert (L.SOFT_NMS_NAIVE, L.SOFT_NMS_LINEAR, L.SOFT_NMS_GAUSSIAN) == (0, 1, 2)
    assert L.SOFT_NMS_METHODS == R.METHODS
    assert callable(pkg.soft_nms)


def test_argument_validation_without_gpu():
    lib = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15
    args = dict(keys=p, key_cap=16, counts=p, max_coord=p, boxes=p16, bpi=16, labels=None, ls=0, fused=0, N=1)

    def images(method=1, sigma=0.5, N=1, max_out=4):
        a = args
        return lib.yv4_soft_nms_images(a['keys'], a['key_cap'], a['counts'], a['max_coord'], a['boxes'], a['bpi'],
                                       a['labels'], a['ls'], a['fused'], N, method, 0.3, sigma, 1e-3, max_out, 10000,
                                       p, p, p, p, None)
    assert images(method=3) == -1 and b'method' in lib.yv4_last_error()
    assert images(method=-1) == -1
    assert images(method=2, sigma=0.0) == -1 and b'sigma' in lib.yv4_last_error()
    assert images(method=2, sigma=-1.0) == -1
    assert images(N=0) == -1
    assert images(max_out=0) == -1
    assert lib.yv4_soft_nms_split_work(0) == 0
    assert lib.yv4_soft_nms_split_work(1 << 31) == 0
    assert lib.yv4_soft_nms_split_work(1000) > 1000 * 24

    def split(n=8, method=1, sigma=0.5, per_label=1, work=p & ~255):
        return lib.yv4_soft_nms_split(p, n, 1.0, p16, None, 0, per_label, method, 0.3, sigma, 1e-3, 4, work, p, p, p, p,
                                      None)
    assert split(method=7) == -1
    assert split(method=2, sigma=0.0) == -1
    assert split(n=0) == -1
    assert split(n=1 << 20, per_label=0) == -1
    assert split(per_label=2) == -1


def test_batched_nms_dispatch_errors():
    """Checked before any device work (the tensors may be anywhere that passes the device check)."""
    from mmdet_yolov4_amd import ops
    with pytest.raises(NotImplementedError, match='not built'):
        ops.nms_spec(dict(type='fancy_nms', iou_threshold=0.5))
    with pytest.raises(TypeError):
        ops.nms_spec(dict(type='soft_nms', iou_threshold=0.5, score_threshold=0.1))
    with pytest.raises(ValueError):
        ops.nms_spec(dict(type='soft_nms', method='cubic'))
    with pytest.raises(ValueError):
        ops.nms_spec(dict(type='soft_nms', method='gaussian', sigma=0.0))
    spec = ops.nms_spec(dict(type='soft_nms', iou_threshold=0.4, method='gaussian', sigma=0.3, min_score=0.01))
    assert spec == dict(type='soft_nms', iou_thr=0.4, sigma=0.3, min_score=0.01, method=2, split_thr=10000)
    assert ops.nms_spec(dict(type='soft_nms')) == dict(type='soft_nms', iou_thr=0.3, sigma=0.5, min_score=1e-3,
                                                       method=1, split_thr=10000)
    assert ops.nms_spec(dict(type='nms', iou_threshold=0.6)) == dict(type='nms', iou_thr=0.6, split_thr=10000)
    # CPU tensors are refused before dispatch, as for every op
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.soft_nms(torch.zeros(1, 4), torch.zeros(1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.batched_nms(torch.zeros(1, 4), torch.zeros(1), torch.zeros(1, dtype=torch.long), dict(type='soft_nms'))


@pytest.mark.parametrize('nms_cfg,kernel', [(dict(type='soft_nms', iou_threshold=0.3, method='gaussian'), 'soft_nms_images'),
                                            (dict(type='nms', iou_threshold=0.65), 'nms_images')])
def test_head_plans_launch_the_configured_nms(nms_cfg, kernel):
    """emit_postprocess builds the post-processing from test_cfg.nms (host only, no launch): a soft-NMS config puts
    yv4_soft_nms_images in the plan with its parameters, a hard one the unchanged yv4_nms_images; unknown types raise."""
    head = pkg.build_head(dict(type='YOLOCSPHead', num_classes=4, in_channels=[8, 8, 8], train_cfg=None,
                               test_cfg=dict(nms_pre=-1, score_thr=0.05, nms=nms_cfg, max_per_img=10)))
    plan = pkg.Plan('cpu')
    views = [plan.add_input_nchw(2, 27, h, w, name=f'pred{i}', pad4=False) for i, (h, w) in enumerate([(8, 12), (4, 6), (2, 3)])]
    post = head.emit_postprocess(plan, views)
    assert [o.name for o in plan.ops if o.kind == 'nms'] == [kernel]
    assert post['nms']['type'] == nms_cfg['type'] and post['iou_thr'] == nms_cfg['iou_threshold']
    if nms_cfg['type'] == 'soft_nms':
        assert post['nms']['method'] == L.SOFT_NMS_GAUSSIAN and post['nms']['sigma'] == 0.5
    bad = pkg.build_head(dict(type='YOLOCSPHead', num_classes=4, in_channels=[8, 8, 8], train_cfg=None,
                              test_cfg=dict(nms_pre=-1, score_thr=0.05, nms=dict(type='fancy_nms'), max_per_img=10)))
    with pytest.raises(NotImplementedError):
        bad.emit_postprocess(pkg.Plan('cpu'), views)


def test_restatement_reproduces_the_reference_fixture(golden):
    """tests/golden/soft_nms.npz: the reference's own multiclass_nms (its batched_nms name bound to this restatement's
    soft-NMS) on each case; the restated multiclass_nms gives the same dets, labels and kept candidates, bit for bit."""
    import json
    g = golden('soft_nms')
    meta = json.loads(str(g['meta']))
    names = [k[3:] for k in meta if k.startswith('mc/')]
    assert {'linear', 'naive', 'gaussian', 'split', 'empty', 'below_min', 'ties', 'negative', 'boundary_0.500',
            'score_factors'} <= set(names)
    for name in names:
        m, p = meta[f'mc/{name}'], f'mc/{name}/'
        f = g[p + 'factors'] if p + 'factors' in g.files else None
        d, l, flat = R.multiclass_soft_nms(g[p + 'boxes'], g[p + 'scores'], m['score_thr'], m['nms'], m['max_num'],
                                           score_factors=f)
        valid = np.nonzero(g[p + 'scores'][:, :-1].reshape(-1) > np.float32(m['score_thr']))[0]
        np.testing.assert_array_equal(d, g[p + 'dets'], err_msg=name)
        np.testing.assert_array_equal(l, g[p + 'labels'], err_msg=name)
        np.testing.assert_array_equal(flat, valid[g[p + 'inds']] if valid.size else flat, err_msg=name)
    # the pinned consequences of the definition, as the reference's glue returns them
    assert g['mc/empty/dets'].shape == (0, 4) and g['mc/below_min/dets'].shape[0] == 1
    bd = g['mc/boundary_0.500/dets']
    assert (bd[:, 4] == np.float32(0.4)).any()          # IoU exactly 0.5 decays (>=): 0.8 * (1 - 0.5)
    assert (g['mc/boundary_naive/dets'][:, 4] == 0).sum() >= 3


# bytes per n of the candidate count / detection count: the values the library returned before its workspaces were
# carved by one shared helper (host functions: no GPU)
_WORK_N = (1, 255, 256, 1024, 1025, 10000, 70001)
_NMS_SPLIT_WORK = (527616, 539904, 539904, 582912, 585984, 1095936, 4516096)
_SOFT_NMS_SPLIT_WORK = (528384, 543232, 543232, 595456, 599040, 1216512, 5356544)
_COCO_RANK_WORK = (2816, 7168, 7168, 22528, 24320, 211712, 1472000)
_COCO_ACCUMULATE_WORK = {                                                     # (K, A * T)
    (1, 1): (4096, 10752, 10752, 36096, 38912, 342784, 2382592),
    (1, 40): (4096, 20736, 20736, 76032, 78848, 732672, 5112576),
    (80, 1): (4608, 11264, 11264, 36608, 39424, 343296, 2383104),
    (80, 40): (4608, 21248, 21248, 76544, 79360, 733184, 5113088),
}


def test_workspace_sizes_are_pinned():
    lib = L.lib()
    assert tuple(lib.yv4_nms_split_work(n) for n in _WORK_N) == _NMS_SPLIT_WORK
    assert tuple(lib.yv4_soft_nms_split_work(n) for n in _WORK_N) == _SOFT_NMS_SPLIT_WORK
    assert tuple(lib.yv4_coco_rank_work(n) for n in _WORK_N) == _COCO_RANK_WORK
    for (K, at), want in _COCO_ACCUMULATE_WORK.items():
        assert tuple(lib.yv4_coco_accumulate_work(n, K, at) for n in _WORK_N) == want, (K, at)
    assert lib.yv4_nms_split_work(0) == 0
    assert lib.yv4_nms_split_work(1 << 31) == 0

    def slots_work(levels, nms_pre):
        arr = (ctypes.c_int32 * len(levels))(*levels)
        return lib.yv4_topk_slots_work(len(levels), arr, nms_pre)
    # no level's top-k exceeds what one workgroup sorts in LDS (8192): no workspace
    for levels in ([1], [1000, 250, 63]):
        for nms_pre in (-1, 100):
            assert slots_work(levels, nms_pre) == 0
    # the radix path: the workspace of the largest level that is cut to more than 8192 slots
    assert slots_work([10000], 8193) == 250624
    assert slots_work([70001, 9000], 8193) == 1751040
    assert slots_work([9000, 70001, 63], 9000) == 1751040
    assert slots_work([70001, 9000], 8192) == 0
