"""Soft-NMS on the MI355X against the host restatement (tests/_soft_nms_ref.py, the definition in include/yv4.h):
the standalone op and batched_nms over sizes from 1 to 70 001 candidates, the plans' post-processing (YOLOCSPHead,
YOLOV3Head, its test-time augmentation) on identical candidates, graph replay and the split path.  `linear` / `naive`
bit for bit; `gaussian` (the GPU's expf against numpy's) to the same selections with scores within rtol 1e-5."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
import _soft_nms_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000, 9999, 10000, 10241, 30000, 70001]


def _problem(n, seed, ties=False, negative=False, spread=None):
    rng = np.random.default_rng(seed)
    spread = spread or max(200.0, 6.0 * np.sqrt(n) * 10)
    xy = rng.uniform(-spread / 3 if negative else 0, spread, (n, 2)).astype(np.float32)
    wh = rng.uniform(4, 60, (n, 2)).astype(np.float32)
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    s = rng.uniform(0, 1, n).astype(np.float32)
    if ties:
        s[::4] = 0.5
    return b, s


def _min_score(n):
    return 1e-3 if n <= 10241 else 0.9        # fewer steps for the host restatement at the largest sizes


@pytest.mark.parametrize('method', ['linear', 'naive'])
@pytest.mark.parametrize('n', SIZES)
def test_standalone_op_bit_exact(gpu_device, method, n):
    b, s = _problem(n, n, ties=n % 2 == 1, negative=n % 3 == 0)
    ms = _min_score(n)
    dets, inds = pkg.soft_nms(torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device), 0.3, 0.5, ms,
                              method)
    rd, ri = R.soft_nms(b, s, 0.3, 0.5, ms, method)
    np.testing.assert_array_equal(inds.cpu().numpy(), ri)
    np.testing.assert_array_equal(dets.cpu().numpy(), np.concatenate([b[ri], rd[:, 4:5]], 1))


@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('method', ['linear', 'naive'])
@pytest.mark.parametrize('n', [1, 65, 257, 1000, 9999, 10000, 10241, 30000])
def test_batched_nms_bit_exact(gpu_device, method, n, agnostic):
    b, s = _problem(n, 100 + n, ties=True, negative=True, spread=400.0)
    idx = np.random.default_rng(n).integers(0, 7, n)
    cfg = dict(type='soft_nms', iou_threshold=0.45, min_score=_min_score(n) if n > 10241 else 0.05, method=method)
    d, k = pkg.batched_nms(torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device),
                           torch.from_numpy(idx), cfg, class_agnostic=agnostic)
    rd, rk = R.batched_soft_nms(b, s, idx, cfg, class_agnostic=agnostic)
    np.testing.assert_array_equal(k.cpu().numpy(), rk)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)


def test_batched_nms_split_max_num_and_multiclass(gpu_device):
    b, s = _problem(12000, 5, spread=300.0)
    idx = np.random.default_rng(1).integers(0, 5, 12000)
    cfg = dict(type='soft_nms', iou_threshold=0.3, min_score=0.2, max_num=50)
    d, k = pkg.batched_nms(torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device), torch.from_numpy(idx),
                           cfg)
    rd, rk = R.batched_soft_nms(b, s, idx, cfg)
    assert rk.shape[0] == 50
    np.testing.assert_array_equal(k.cpu().numpy(), rk)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)
    with pytest.raises(TypeError):                     # below split_thr max_num goes to soft_nms, which has no such key
        pkg.batched_nms(torch.from_numpy(b[:10]).to(gpu_device), torch.from_numpy(s[:10]).to(gpu_device),
                        torch.from_numpy(idx[:10]), cfg)
    # multiclass_nms: (n, C+1) scores with the background column, cut to max_num
    ms = np.random.default_rng(3).uniform(0, 1, (400, 5)).astype(np.float32)
    for mcfg in (dict(type='soft_nms', iou_threshold=0.5), dict(type='soft_nms', method='naive', min_score=0.0)):
        dd, ll = pkg.multiclass_nms(torch.from_numpy(b[:400]).to(gpu_device), torch.from_numpy(ms).to(gpu_device), 0.3,
                                    mcfg, max_num=60)
        rdd, rll, _ = R.multiclass_soft_nms(b[:400], ms, 0.3, mcfg, max_num=60)
        np.testing.assert_array_equal(dd.cpu().numpy(), rdd)
        np.testing.assert_array_equal(ll.cpu().numpy(), rll)


@pytest.mark.parametrize('n', [64, 1000, 9999, 30000])
def test_gaussian_within_tolerance(gpu_device, n):
    """Clusters of three overlapping boxes, clusters 80 px apart: every decay chain stays inside its cluster, so a last-bit
    difference of expf can only swap the order of two selections whose scores tie to rounding -- it cannot change which
    boxes survive or their scores.  Same keep set, scores within rtol 1e-5, and where the order differs the swapped
    selections' scores are within that tolerance."""
    rng = np.random.default_rng(n)
    cells = (n + 2) // 3
    side = int(np.ceil(np.sqrt(cells)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:cells].astype(np.float32) * 80
    xy = (np.repeat(g, 3, 0)[:n] + rng.integers(0, 10, (n, 2)).astype(np.float32)).astype(np.float32)
    b = np.concatenate([xy, xy + 24 + rng.integers(0, 8, (n, 2)).astype(np.float32)], 1)
    s = rng.uniform(0.05, 1, n).astype(np.float32)
    ms = 1e-3 if n <= 10000 else 0.3
    dets, inds = pkg.soft_nms(torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device), 0.3, 0.5, ms,
                              'gaussian')
    rd, ri = R.soft_nms(b, s, 0.3, 0.5, ms, 'gaussian')
    got, gi = dets.cpu().numpy(), inds.cpu().numpy()
    assert sorted(gi.tolist()) == sorted(ri.tolist())
    ref_score = dict(zip(ri.tolist(), rd[:, 4].tolist()))
    want = np.array([ref_score[i] for i in gi.tolist()], np.float32)
    np.testing.assert_array_equal(got[:, :4], b[gi])
    dev = np.abs(got[:, 4] - want) / np.maximum(np.abs(want), 1e-30)
    moved = int((gi != ri).sum())
    print(f'gaussian n={n}: largest relative score deviation {dev.max():.3e}, {moved} selections in another order')
    np.testing.assert_allclose(got[:, 4], want, rtol=1e-5, atol=0)
    for j in np.nonzero(gi != ri)[0]:
        assert abs(float(got[j, 4]) - float(rd[j, 4])) <= 1e-5 * abs(float(rd[j, 4])), j


def test_early_stop_equals_a_full_run_cut(gpu_device):
    from mmdet_yolov4_amd import ops
    b, s = _problem(3000, 9, ties=True)
    bt, st = torch.from_numpy(b).to(gpu_device), torch.from_numpy(s).to(gpu_device)
    spec = dict(method=1, iou_thr=0.3, sigma=0.5, min_score=1e-3)
    full_d, full_k = ops._soft_single(bt, st, None, spec, -1, 1 << 30, True)
    for cap in (1, 100, 300):
        d, k = ops._soft_single(bt, st, None, spec, cap, 1 << 30, True)
        np.testing.assert_array_equal(k.cpu().numpy(), full_k[:cap].cpu().numpy())
        np.testing.assert_array_equal(d.cpu().numpy(), full_d[:cap].cpu().numpy())
    # the split path's per-label early stop keeps the re-sorted head exact, ties at the cut included
    idx = torch.from_numpy(np.arange(3000) % 4).to(gpu_device).int()
    full_d, full_k = ops._soft_single(bt, st, idx, spec, -1, 10, False)
    for cap in (5, 37, 300):
        d, k = ops._soft_single(bt, st, idx, spec, cap, 10, False)
        np.testing.assert_array_equal(k.cpu().numpy(), full_k[:cap].cpu().numpy())
        np.testing.assert_array_equal(d.cpu().numpy(), full_d[:cap].cpu().numpy())


# ---- plans: the candidates the kernel consumed, restated ------------------------------------------------------------
def _key_scores(keys):
    hi = (keys.astype(np.uint64) >> np.uint64(32)).astype(np.uint32)
    u = ~hi
    bits = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32)
    return bits.view(np.float32)


def _check_post(post, nms_cfg, agnostic=False, exact=True):
    """Every image of a finished plan against the restatement on the candidates of its key buffer."""
    from mmdet_yolov4_amd.yolocsp_head import collect_results
    res = collect_results(post, with_nms=True)
    C = post['num_classes']
    for n in range(post['N']):
        cnt = int(post['counts'][n])
        keys = post['keys'][n, :cnt].cpu().numpy()
        flat = (keys & 0xffffffff).astype(np.int64)
        order = np.argsort(flat, kind='stable')
        flat, sc = flat[order], _key_scores(keys[order])
        boxes = post['boxes'][n].cpu().numpy()[flat // C]
        labels = flat % C
        d, l = res[n]
        if cnt == 0:
            assert d.shape[0] == 0
            continue
        rd, rk = R.batched_soft_nms(boxes, sc, labels, dict(nms_cfg, split_thr=post['split_thr']),
                                    class_agnostic=agnostic)
        rd, rk = rd[:post['max_per_img']], rk[:post['max_per_img']]
        np.testing.assert_array_equal(l.cpu().numpy(), labels[rk])
        np.testing.assert_array_equal(post['index'][n, :d.shape[0]].cpu().numpy(), flat[rk])
        if exact:
            np.testing.assert_array_equal(d.cpu().numpy(), rd)
        else:
            np.testing.assert_array_equal(d.cpu().numpy()[:, :4], rd[:, :4])
            np.testing.assert_allclose(d.cpu().numpy()[:, 4], rd[:, 4], rtol=1e-5, atol=0)
    return res


def _v4_head(dev, nms_cfg, agnostic=False, ncls=80, max_per_img=300):
    return pkg.build_head(dict(type='YOLOCSPHead', num_classes=ncls, in_channels=[8, 8, 8], class_agnostic=agnostic,
                               train_cfg=None,
                               test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=nms_cfg, max_per_img=max_per_img))).to(dev)


NMS_CFGS = [dict(type='soft_nms', iou_threshold=0.3, method='linear'),
            dict(type='soft_nms', iou_threshold=0.5, method='naive', min_score=0.0),
            dict(type='soft_nms', iou_threshold=0.3, method='gaussian', sigma=0.5)]


@pytest.mark.parametrize('ci', range(3))
def test_yolocsp_get_bboxes(golden, gpu_device, ci):
    g = golden('tiny_v4')
    cfg = NMS_CFGS[ci]
    head = _v4_head(gpu_device, cfg)
    preds = [torch.from_numpy(g[f'pred{i}']).to(gpu_device) for i in range(3)]
    metas = [dict(scale_factor=g['scale_factors'][i]) for i in range(2)]
    head.get_bboxes(preds, metas, rescale=True)
    plan = next(iter(head._post_cache.values()))
    assert [o.name for o in plan.ops if o.kind == 'nms'] == ['soft_nms_images']
    _check_post(plan.post, cfg, exact=cfg['method'] != 'gaussian')


def test_yolocsp_get_bboxes_class_agnostic(golden, gpu_device):
    g = golden('post_variants')
    cfg = dict(type='soft_nms', iou_threshold=0.3)
    head = _v4_head(gpu_device, cfg, agnostic=True, ncls=int(g['num_classes']), max_per_img=50)
    preds = [torch.from_numpy(g[f'agnostic/pred{i}']).to(gpu_device) for i in range(3)]
    metas = [dict(scale_factor=g['scale_factors'][i]) for i in range(2)]
    head.get_bboxes(preds, metas, rescale=True)
    _check_post(next(iter(head._post_cache.values())).post, cfg, agnostic=False)


@pytest.mark.parametrize('ci', range(2))
def test_collect_results_split_path(golden, gpu_device, ci):
    """>= 10 000 candidates per image: yv4_soft_nms_images flags them, collect_results runs yv4_soft_nms_split."""
    g = golden('tiny_v4')
    cfg = NMS_CFGS[ci]
    preds = []
    for i in range(3):
        p = torch.from_numpy(g[f'pred{i}']).clone()
        p.view(2, 3, 85, *p.shape[-2:])[:, :, 4:] += 3.5
        preds.append(p.to(gpu_device))
    head = _v4_head(gpu_device, cfg)
    metas = [dict(scale_factor=g['scale_factors'][i]) for i in range(2)]
    head.get_bboxes(preds, metas, rescale=True)
    post = next(iter(head._post_cache.values())).post
    assert (post['counts'].cpu().numpy() >= 10000).all()
    _check_post(post, cfg)


def test_yolov3_get_bboxes(golden, gpu_device):
    g = golden('tiny_v3')
    cfg = dict(type='soft_nms', iou_threshold=0.45, method='linear')
    tc = pkg.registry.ConfigDict(nms_pre=-1, min_bbox_size=0, score_thr=0.05, conf_thr=-1, nms=cfg, max_per_img=100)
    head = pkg.YOLOV3Head(num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32], test_cfg=tc).to(gpu_device)
    preds = [torch.from_numpy(g[f'pred{i}']).to(gpu_device) for i in range(3)]
    metas = [dict(scale_factor=g['scale_factors'][i]) for i in range(2)]
    head.get_bboxes(preds, metas, rescale=True)
    plan = next(iter(head._post_cache.values()))
    assert [o.name for o in plan.ops if o.kind == 'nms'] == ['soft_nms_images']
    _check_post(plan.post, cfg)


def _smoke_detector(dev, nms_cfg):
    torch.manual_seed(0)
    scale = [['conv', 'bottleneck', 'csp', 'csp', 'csp', 'sppv4'], [None, 1, 1, 2, 2, 1], [8, 16, 32, 64, 128, 128]]
    det = pkg.build_detector(dict(
        type='SingleStageDetector', backbone=dict(type='DarknetCSP', scale=scale, out_indices=[3, 4, 5]),
        neck=dict(type='YOLOV4Neck', in_channels=[64, 128, 128], out_channels=[64, 128, 256], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=4, in_channels=[64, 128, 256]), train_cfg=None,
        test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=nms_cfg, max_per_img=300)))
    with torch.no_grad():
        for conv in det.bbox_head.convs_pred:
            conv.weight.normal_(0, 0.02)
            conv.bias.view(3, 9)[:, 4:] = -2.5            # every (box, class) passes: 1 512 candidates per image
    return det.eval().to(dev)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_simple_test_graph_replay_equals_eager(gpu_device, dtype):
    cfg = dict(type='soft_nms', iou_threshold=0.3, method='linear')
    det = _smoke_detector(gpu_device, cfg)
    img = ((torch.randint(0, 256, (2, 3, 64, 96)).float() - 114.0) / 255.0).to(gpu_device)
    outs = []
    for graph in (False, True):
        plan = det.compile(2, 64, 96, device=gpu_device, rescale=False, graph=graph, dtype=dtype)
        assert [o.name for o in plan.ops if o.kind == 'nms'] == ['soft_nms_images']
        plan.run(img)
        plan.run(img)
        torch.cuda.synchronize()
        outs.append([plan.post[k].clone() for k in ('dets', 'labels', 'index', 'count')])
        if graph:
            _check_post(plan.post, cfg)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert int(outs[0][3].min()) > 0
    res = det.simple_test(img, [dict(scale_factor=np.ones(4, np.float32))] * 2, rescale=True)
    assert len(res) == 2 and len(res[0]) == 4


def test_yolov3_aug_test(golden, gpu_device):
    """The TTA plan's merged candidates through yv4_soft_nms_images against the restatement."""
    from test_gpu_v3 import build
    g = golden('tiny_v3')
    det = build(g, gpu_device)
    cfg = dict(type='soft_nms', iou_threshold=0.45, method='linear')
    det.bbox_head.test_cfg = pkg.registry.ConfigDict(nms_pre=40, min_bbox_size=0, score_thr=0.05, conf_thr=0.005,
                                                     nms=cfg, max_per_img=100)
    img = torch.from_numpy(g['img'][:1]).to(gpu_device)
    H, W = img.shape[2:]
    tta = det.compile_tta(1, [(H, W), (H, W)], [0, 1], device=gpu_device, graph=False)
    assert [o.name for o in tta.ops if o.kind == 'nms'] == ['soft_nms_images']
    metas = [[dict(img_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=False)],
             [dict(img_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=True, flip_direction='horizontal')]]
    pkg.tta.set_tta_metas(tta.post, metas)
    tta.run(torch.cat([img, img]))
    torch.cuda.synchronize()
    _check_post(tta.post, cfg)
