"""Soft-NMS on the MI355X against tests/golden/soft_nms.npz, which the reference's own multiclass_nms, YOLOCSPHead /
YOLOV3Head.get_bboxes and YOLOV3Head.aug_test produced (make_golden_soft_nms.py), and the definition's edge cases through
every kernel route: yv4_soft_nms_images, yv4_soft_nms_split with one problem (per_label 0) and per label (per_label 1).
The cases: IoU exactly at the threshold (integer coordinates), every score below min_score, exact ties, negative
coordinates across classes, an image without candidates in a plan, and a step whose compaction takes two LDS batches."""
import json

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import ops
import _soft_nms_ref as R

pytestmark = pytest.mark.gpu
MC = ['linear', 'naive', 'gaussian', 'split', 'empty', 'below_min', 'ties', 'negative', 'boundary_0.250',
      'boundary_0.333', 'boundary_0.500', 'boundary_naive', 'score_factors']


def _meta(g):
    return json.loads(str(g['meta']))


def _mc_inputs(g, name, dev):
    p = f'mc/{name}/'
    f = torch.from_numpy(g[p + 'factors']).to(dev) if p + 'factors' in g.files else None
    return torch.from_numpy(g[p + 'boxes']).to(dev), torch.from_numpy(g[p + 'scores']).to(dev), f


@pytest.mark.parametrize('name', MC)
def test_multiclass_nms_against_the_reference(golden, gpu_device, name):
    g = golden('soft_nms')
    m, p = _meta(g)[f'mc/{name}'], f'mc/{name}/'
    b, s, f = _mc_inputs(g, name, gpu_device)
    d, l, k = pkg.multiclass_nms(b, s, m['score_thr'], m['nms'], m['max_num'], score_factors=f, return_inds=True)
    np.testing.assert_array_equal(l.cpu().numpy(), g[p + 'labels'])
    np.testing.assert_array_equal(k.cpu().numpy(), g[p + 'inds'])
    if m['nms'].get('method') == 'gaussian':
        np.testing.assert_array_equal(d.cpu().numpy()[:, :4], g[p + 'dets'][:, :4])
        np.testing.assert_allclose(d.cpu().numpy()[:, 4], g[p + 'dets'][:, 4], rtol=1e-5, atol=0)
    else:
        np.testing.assert_array_equal(d.cpu().numpy(), g[p + 'dets'])


def _candidates(g, name):
    """multiclass_nms' candidate list of a fixture case (flat order): boxes, scores, labels."""
    m, p = _meta(g)[f'mc/{name}'], f'mc/{name}/'
    sc = g[p + 'scores']
    C = sc.shape[1] - 1
    flat = sc[:, :-1].reshape(-1)
    valid = np.nonzero(flat > np.float32(m['score_thr']))[0]
    scores = flat[valid]
    if p + 'factors' in g.files:
        scores = (scores * np.repeat(g[p + 'factors'], C)[valid]).astype(np.float32)
    return g[p + 'boxes'][valid // C], scores, (valid % C).astype(np.int64), m['nms']


@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('name', [n for n in MC if n not in ('empty', 'gaussian')])
def test_every_kernel_route_on_the_edge_cases(golden, gpu_device, name, agnostic):
    """The same candidates through yv4_soft_nms_images, yv4_soft_nms_split per_label 0 (one problem in global memory)
    and per_label 1 (mmcv's split branch, forced with split_thr 1): bit for bit against the restatement."""
    g = golden('soft_nms')
    b, s, lab, cfg = _candidates(g, name)
    spec = ops.nms_spec(cfg)
    bt, st = torch.from_numpy(np.ascontiguousarray(b)).to(gpu_device), torch.from_numpy(s).to(gpu_device)
    lt = torch.from_numpy(lab).to(gpu_device).int()
    want_d, want_k = R.batched_soft_nms(b, s, lab, dict(cfg, split_thr=1 << 30), class_agnostic=agnostic)
    for single_in_global in (False, True):
        d, k = ops._soft_single(bt, st, lt, spec, -1, 1 << 30, agnostic, single_in_global=single_in_global)
        np.testing.assert_array_equal(k.cpu().numpy(), want_k)
        np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    if name == 'below_min':                       # the first winner is never compared with min_score: one box
        assert want_k.shape[0] == 1 and want_d[0, 4] < cfg.get('min_score', 1e-3)
    if name == 'boundary_0.500':                  # three pairs whose fp32 IoU is exactly 0.5 decay (>=): 0.8 * 0.5
        assert (want_d[:, 4] == np.float32(0.4)).sum() >= 3
    want_d, want_k = R.batched_soft_nms(b, s, lab, dict(cfg, split_thr=1), class_agnostic=agnostic)
    d, k = ops._soft_single(bt, st, lt, spec, -1, 1, agnostic)
    np.testing.assert_array_equal(k.cpu().numpy(), want_k)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    if name == 'below_min':                       # per label (mmcv's split loop, also when class-agnostic): one each
        assert want_k.shape[0] == len(np.unique(lab))


def _close_dets(got, want, labels_got, labels_want, tol=1e-4):
    np.testing.assert_array_equal(labels_got, labels_want)
    assert got.shape == want.shape
    if got.size:
        err = np.abs(got - want) / (1 + np.abs(want))
        assert err.max() <= tol, err.max(0)


@pytest.mark.parametrize('tag', ['linear', 'naive', 'gaussian'])
def test_yolocsp_get_bboxes_against_the_reference(golden, gpu_device, tag):
    g, g4 = golden('soft_nms'), golden('tiny_v4')
    cfg = _meta(g)[f'v4/{tag}']['nms']
    head = pkg.build_head(dict(type='YOLOCSPHead', num_classes=80, in_channels=[8, 8, 8], train_cfg=None,
                               test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=cfg, max_per_img=300))).to(gpu_device)
    preds = [torch.from_numpy(g4[f'pred{i}']).to(gpu_device) for i in range(3)]
    metas = [dict(scale_factor=g4['scale_factors'][i]) for i in range(2)]
    res = head.get_bboxes(preds, metas, rescale=True)
    for n, (d, l) in enumerate(res):
        _close_dets(d.cpu().numpy(), g[f'v4/{tag}/dets{n}'], l.cpu().numpy(), g[f'v4/{tag}/labels{n}'])


def test_image_without_candidates_in_a_soft_plan(golden, gpu_device):
    """Image 1 has no candidate (objectness logits -30): an empty result; image 0 is the reference's."""
    g, g4 = golden('soft_nms'), golden('tiny_v4')
    cfg = _meta(g)['v4/linear']['nms']
    head = pkg.build_head(dict(type='YOLOCSPHead', num_classes=80, in_channels=[8, 8, 8], train_cfg=None,
                               test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=cfg, max_per_img=300))).to(gpu_device)
    preds = []
    for i in range(3):
        p = torch.from_numpy(g4[f'pred{i}']).clone()
        p.view(2, 3, 85, *p.shape[-2:])[1, :, 4] = -30.0
        preds.append(p.to(gpu_device))
    metas = [dict(scale_factor=g4['scale_factors'][i]) for i in range(2)]
    res = head.get_bboxes(preds, metas, rescale=True)
    post = next(iter(head._post_cache.values())).post
    assert int(post['counts'][1]) == 0 and int(post['count'][1]) == 0
    assert res[1][0].shape == (0, 4) and res[1][1].shape == (0,)
    _close_dets(res[0][0].cpu().numpy(), g['v4/linear/dets0'], res[0][1].cpu().numpy(), g['v4/linear/labels0'])


def _v3_head(dev, test_cfg):
    return pkg.YOLOV3Head(num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32],
                          test_cfg=pkg.registry.ConfigDict(test_cfg)).to(dev)


def test_yolov3_get_bboxes_against_the_reference(golden, gpu_device):
    g, g3 = golden('soft_nms'), golden('tiny_v3')
    head = _v3_head(gpu_device, _meta(g)['v3']['test_cfg'])
    preds = [torch.from_numpy(g3[f'pred{i}']).to(gpu_device) for i in range(3)]
    metas = [dict(scale_factor=g3['scale_factors'][i]) for i in range(2)]
    res = head.get_bboxes(preds, metas, rescale=True)
    for n, (d, l) in enumerate(res):
        _close_dets(d.cpu().numpy(), g[f'v3/dets{n}'], l.cpu().numpy(), g[f'v3/labels{n}'])


def test_yolov3_aug_test_against_the_reference(golden, gpu_device):
    """The TTA merge with soft-NMS on the reference's per-augmentation pred maps (v3_tta.npz 'scales_hflip')."""
    g, gt = golden('soft_nms'), golden('v3_tta')
    meta = _meta(g)['tta']
    case = json.loads(str(gt['cases']))[meta['case']]
    head = _v3_head(gpu_device, meta['test_cfg'])
    name = meta['case']
    metas = [[dict(img_shape=tuple(int(v) for v in gt[f'{name}/img_shape{a}']),
                   pad_shape=tuple(int(v) for v in gt[f'{name}/pad_shape{a}']),
                   scale_factor=gt[f'{name}/scale_factor{a}'], flip=d is not None, flip_direction=d)]
             for a, d in enumerate(case['flips'])]
    preds = [[torch.from_numpy(gt[f'{name}/pred{a}_{i}']).to(gpu_device) for i in range(3)]
             for a in range(case['num_augs'])]
    with torch.no_grad():
        res = head.aug_test_preds(preds, metas, rescale=True)[0]
    assert sum(r.shape[0] for r in res) == meta['detections'] > 0
    for c in range(6):
        want = g[f'tta/result_{c}']
        assert res[c].shape == want.shape, (c, res[c].shape, want.shape)
        if want.size:
            assert (np.abs(res[c] - want) / (1 + np.abs(want))).max() <= 1e-4, c


@pytest.mark.parametrize('per_label', [0, 1])
def test_compaction_over_two_lds_batches(gpu_device, per_label):
    """40 000 candidates, 60 % of them below min_score: the first step discards ~24 000 entries spread over the array,
    more than 8 192 of them below the new end -- the hole moves of that step take two LDS batches."""
    rng = np.random.default_rng(40)
    n = 40000
    xy = rng.uniform(0, 20000, (n, 2)).astype(np.float32)
    b = np.concatenate([xy, xy + rng.uniform(8, 40, (n, 2)).astype(np.float32)], 1)
    s = rng.uniform(0, 1, n).astype(np.float32)
    ms = 0.6
    below = s < np.float32(ms)
    below[int(np.argmax(s))] = False
    nb2 = n - int(below.sum())
    assert int(below[:nb2].sum()) > 8192          # holes below the new end in step 1 (decay only lowers scores)
    bt, st = torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device)
    spec = dict(method=pkg._lib.SOFT_NMS_LINEAR, iou_thr=0.3, sigma=0.5, min_score=ms)
    lab = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    d, k = ops._soft_single(bt, st, lab, spec, -1, 1 << 30 if per_label == 0 else 1, per_label == 0)
    rd, rk = R.soft_nms(b, s, 0.3, 0.5, ms, 'linear')
    if per_label:
        rk, sc = R._resort(rk, rd[:, 4])
        rd = np.concatenate([b[rk], sc[:, None]], 1)
    np.testing.assert_array_equal(k.cpu().numpy(), rk)
    np.testing.assert_array_equal(d.cpu().numpy()[:, 4], rd[:, 4])
