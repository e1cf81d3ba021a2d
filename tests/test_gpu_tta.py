"""YOLOv3 test-time augmentation on the GPU against the reference's own aug_test (tests/golden/v3_tta.npz, made by
tests/golden/make_golden_v3_tta.py on tiny_v3.npz's network): flipped letterbox, get_bboxes(with_nms=False), the
merged NMS of aug_test / forward_test, batches, graph replay and 16-bit plans."""
import json

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from conftest import state_dict_from

pytestmark = pytest.mark.gpu

CASES = ['scales_hflip', 'vflip_dflip', 'split', 'empty']
IMG_NORM = dict(mean=[0, 0, 0], std=[255.0, 255.0, 255.0], to_rgb=True)


class TinyDarknet(pkg.Darknet):
    """The fixture's run-time narrowed arch (tests/golden/make_golden_v3.py)."""
    arch_settings = {53: ((1, 1, 2, 2, 1), ((32, 16), (16, 32), (32, 32), (32, 64), (64, 64)))}


def case_of(g, name):
    return json.loads(str(g['cases']))[name]


def build(dev, test_cfg):
    sd = state_dict_from(np.load(_golden_path('tiny_v3')))
    det = pkg.YOLOV3(backbone=dict(type='Darknet', depth=53, out_indices=(3, 4, 5)),
                     neck=dict(type='YOLOV3Neck', num_scales=3, in_channels=[1024, 512, 256],
                               out_channels=[512, 256, 128]),
                     bbox_head=dict(type='YOLOV3Head', num_classes=6, in_channels=[512, 256, 128],
                                    out_channels=[1024, 512, 256]), test_cfg=test_cfg)
    det.backbone = TinyDarknet(depth=53, out_indices=(3, 4, 5))
    det.neck = pkg.YOLOV3Neck(num_scales=3, in_channels=[64, 64, 32], out_channels=[64, 32, 16])
    det.bbox_head = pkg.YOLOV3Head(num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32], test_cfg=test_cfg)
    det.load_state_dict(sd, strict=True)
    return det.to(dev).eval()


def _golden_path(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.npz')


def metas_of(g, name, case):
    out = []
    for a, d in enumerate(case['flips']):
        out.append([dict(img_shape=tuple(int(v) for v in g[f'{name}/img_shape{a}']),
                         pad_shape=tuple(int(v) for v in g[f'{name}/pad_shape{a}']),
                         scale_factor=g[f'{name}/scale_factor{a}'], flip=d is not None, flip_direction=d)])
    return out


def imgs_of(g, name, case, dev):
    return [torch.from_numpy(g[f'{name}/img{a}']).to(dev) for a in range(case['num_augs'])]


def check_result(got, g, key, tol=1e-4, box_tol=None):
    """Per-class lists: the same number of detections per class (labels exact); scores within `tol` and boxes within
    `box_tol` (default `tol`) as |got - want| / (1 + |want|), the measure of test_gpu_v3.py."""
    box_tol = tol if box_tol is None else box_tol
    for c in range(6):
        want = g[f'{key}_{c}']
        assert got[c].shape == want.shape, (key, c, got[c].shape, want.shape)
        err = np.abs(got[c] - want) / (1 + np.abs(want))
        if err.size:
            assert err[:, :4].max() <= box_tol and err[:, 4].max() <= tol, (key, c, err.max(0))


def test_flipped_letterbox_is_a_permutation(gpu_device):
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (61, 93, 3), dtype=np.uint8), rng.integers(0, 256, (80, 50, 3), dtype=np.uint8)]
    pipe = pkg.FusedTestPipeline(img_scale=(96, 64), size_divisor=32, mean=IMG_NORM['mean'], std=IMG_NORM['std'],
                                 to_rgb=True, pad_before_normalize=False, device=gpu_device, flip=True,
                                 flip_direction=['horizontal', 'vertical', 'diagonal'])
    batches, metas = pipe(imgs)                          # a ragged batch: the second image is narrower
    assert len(batches) == 4 and [m[0]['flip_direction'] for m in metas] == [None, 'horizontal', 'vertical', 'diagonal']
    base = batches[0].cpu().numpy()
    axes = {'horizontal': (2,), 'vertical': (1,), 'diagonal': (1, 2)}
    for a in range(1, 4):
        got = batches[a].cpu().numpy()
        for i, m in enumerate(metas[a]):
            nh, nw = m['img_shape'][:2]
            assert m['flip'] and m['img_shape'] == metas[0][i]['img_shape'] and m['pad_shape'] == metas[0][i]['pad_shape']
            np.testing.assert_array_equal(m['scale_factor'], metas[0][i]['scale_factor'])
            want = np.flip(base[i, :, :nh, :nw], axis=axes[m['flip_direction']])
            assert np.array_equal(got[i, :, :nh, :nw], want), (a, i)
            pad = np.ones(got.shape[1:], bool)
            pad[:, :nh, :nw] = False
            assert np.array_equal(got[i][pad], base[i][pad])          # the pad region stays where it is


def test_pipeline_reproduces_fixture_inputs(golden, gpu_device):
    g = golden('v3_tta')
    for name in CASES:
        case = case_of(g, name)
        pipe = pkg.FusedTestPipeline(img_scale=[tuple(s) for s in case['scales']], size_divisor=32,
                                     mean=IMG_NORM['mean'], std=IMG_NORM['std'], to_rgb=True, pad_before_normalize=False,
                                     device=gpu_device, flip=bool(case['flip_direction']),
                                     flip_direction=case['flip_direction'] or 'horizontal')
        batches, metas = pipe([g[f'{name}/src']])
        assert len(batches) == case['num_augs']
        for a, (b, m) in enumerate(zip(batches, metas)):
            assert np.array_equal(b.cpu().numpy(), g[f'{name}/img{a}']), (name, a)
            assert m[0]['img_shape'] == tuple(int(v) for v in g[f'{name}/img_shape{a}'])
            np.testing.assert_array_equal(m[0]['scale_factor'], g[f'{name}/scale_factor{a}'])


@pytest.mark.parametrize('name', CASES)
def test_get_bboxes_without_nms(golden, gpu_device, name):
    g = golden('v3_tta')
    case = case_of(g, name)
    det = build(gpu_device, case['test_cfg'])
    metas = metas_of(g, name, case)
    for a in range(case['num_augs']):
        preds = [torch.from_numpy(g[f'{name}/pred{a}_{i}']).to(gpu_device) for i in range(3)]
        (b, s, c), = det.bbox_head.get_bboxes(preds, metas[a], rescale=False, with_nms=False)
        # the slot table: a cut level in descending objectness, ties to the lower anchor, of the kernel's own conf;
        # an uncut level in anchor order
        post = next(iter(det.bbox_head._post_cache.values())).post['res']['g0']
        conf_all = post['conf'][0].cpu().numpy()
        slots = post['slots'][0].cpu().numpy()
        nms_pre, base, sb, want = case['test_cfg']['nms_pre'], 0, 0, []
        for n_l in post['sizes']:
            idx = np.arange(base, base + n_l)
            if 0 < nms_pre < n_l:
                idx = idx[np.lexsort((idx, -conf_all[idx].astype(np.float64)))][:nms_pre]
            want.append(idx)
            base += n_l
        np.testing.assert_array_equal(slots, np.concatenate(want))
        # the reference's order and values: the GPU sigmoid (the simple_test path's) and torch's CPU sigmoid differ by
        # up to two ulp
        np.testing.assert_array_max_ulp(c.cpu().numpy(), g[f'{name}/conf{a}'], maxulp=2)
        np.testing.assert_array_max_ulp(s.cpu().numpy(), g[f'{name}/scores{a}'], maxulp=2)
        assert not s[:, -1].any()
        np.testing.assert_allclose(b.cpu().numpy(), g[f'{name}/bboxes{a}'], rtol=1e-4, atol=1e-4)
        (br, _, _), = det.bbox_head.get_bboxes(preds, metas[a], rescale=True, with_nms=False)
        np.testing.assert_array_equal(br.cpu().numpy(), (b.cpu() / torch.from_numpy(metas[a][0]['scale_factor'])).numpy())


@pytest.mark.parametrize('name', CASES)
def test_aug_test_against_reference(golden, gpu_device, name):
    g = golden('v3_tta')
    case = case_of(g, name)
    det = build(gpu_device, case['test_cfg'])
    imgs, metas = imgs_of(g, name, case, gpu_device), metas_of(g, name, case)
    preds = [[torch.from_numpy(g[f'{name}/pred{a}_{i}']).to(gpu_device) for i in range(3)]
             for a in range(case['num_augs'])]
    with torch.no_grad():
        for rescale, tag in ((True, ''), (False, '_norescale')):
            # the merge on the reference's pred maps: within 1e-4
            res = det.bbox_head.aug_test_preds(preds, metas, rescale=rescale)
            check_result(res[0], g, f'{name}/result{tag}')
            # the whole path: the network's pred maps are within 1e-4 of the reference's (test_gpu_v3.py), which the
            # exp() of the box decode and the division by scale_factor amplify in the boxes
            res = det.aug_test(imgs, metas, rescale=rescale)
            assert len(res) == 1
            check_result(res[0], g, f'{name}/result{tag}', box_tol=1e-3)
            res = det.forward_test(imgs, metas, rescale=rescale)
            check_result(res[0], g, f'{name}/result{tag}', box_tol=1e-3)
        # YOLOV3Head.aug_test: features in, the reference's batch-1 per-class list out
        feats = [det.neck(det.backbone(x)) for x in imgs]
        check_result(det.bbox_head.aug_test(feats, metas, rescale=True), g, f'{name}/result', box_tol=1e-3)
    if name == 'split':
        flips = [pkg._lib.FLIP_CODES[d] if d else 0 for d in case['flips']]
        plan = det.compile_tta(1, [tuple(x.shape[2:]) for x in imgs], flips, device=gpu_device, graph=True)
        assert int(plan.post['counts'][0]) >= plan.post['split_thr']       # the run above took mmcv's split path


def test_batch_equals_batch_one(golden, gpu_device):
    g = golden('v3_tta')
    name = 'scales_hflip'
    case = case_of(g, name)
    det = build(gpu_device, case['test_cfg'])
    imgs, metas = imgs_of(g, name, case, gpu_device), metas_of(g, name, case)
    gen = torch.Generator(device='cpu').manual_seed(5)
    N = 4
    # four images: the fixture's and three variants with the same geometry
    big = [torch.cat([x] + [(x + 0.05 * k * torch.rand(x.shape, generator=gen).to(x.device)).clamp(0, 1)
                            * (x != 0) for k in range(1, N)]) for x in imgs]
    bmetas = [[dict(m[0]) for _ in range(N)] for m in metas]
    with torch.no_grad():
        res = det.aug_test(big, bmetas, rescale=True)
        assert len(res) == N
        for i in range(N):
            one = det.aug_test([x[i:i + 1] for x in big], [m[i:i + 1] for m in bmetas], rescale=True)[0]
            for c in range(6):
                assert np.array_equal(res[i][c], one[c]), (i, c)
        with pytest.raises(AssertionError, match='aug test does not support inference with batch size 4'):
            det.forward_test(big, bmetas, rescale=True)


def test_graph_replay_equals_eager(golden, gpu_device):
    g = golden('v3_tta')
    name = 'vflip_dflip'
    case = case_of(g, name)
    det = build(gpu_device, case['test_cfg'])
    imgs, metas = imgs_of(g, name, case, gpu_device), metas_of(g, name, case)
    geos = [tuple(x.shape[2:]) for x in imgs]
    flips = [pkg._lib.FLIP_CODES[d] if d else 0 for d in case['flips']]
    outs = []
    for graph in (False, True):
        plan = det.compile_tta(1, geos, flips, device=gpu_device, graph=graph)
        assert len(plan.tta_groups) == 1                  # an image and its flips: one network pass
        pkg.tta.set_tta_metas(plan.post, metas)
        plan.run(torch.cat(imgs))
        torch.cuda.synchronize()
        outs.append([plan.post[k].clone() for k in ('count', 'dets', 'labels', 'index', 'boxes')])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_16_bit_tta_plans(golden, gpu_device, dtype):
    g = golden('v3_tta')
    name = 'scales_hflip'
    case = case_of(g, name)
    det = build(gpu_device, case['test_cfg'])
    imgs, metas = imgs_of(g, name, case, gpu_device), metas_of(g, name, case)
    geos = [tuple(x.shape[2:]) for x in imgs]
    flips = [pkg._lib.FLIP_CODES[d] if d else 0 for d in case['flips']]
    plan = det.compile_tta(1, geos, flips, device=gpu_device, graph=True, dtype=dtype)
    assert len(plan.tta_groups) == 2
    pkg.tta.set_tta_metas(plan.post, metas)
    plan.run(*[torch.cat([imgs[a] for a in augs]) for augs in plan.tta_groups])
    torch.cuda.synchronize()
    got = pkg.tta.collect_tta(plan.post, metas, True, 6)
    # the plan's pred maps, per augmentation (NHWC fp32 buffers -> NCHW)
    preds = [None] * len(imgs)
    tol = 2e-2 if dtype == torch.float16 else 1.5e-1
    for views, augs in zip(plan.pred_views, plan.tta_groups):
        maps = [v.buf.tensor.view(v.N, v.H, v.W, v.C).permute(0, 3, 1, 2).contiguous() for v in views]
        for r, a in enumerate(augs):
            preds[a] = [m[r:r + 1] for m in maps]
            for i, p in enumerate(preds[a]):
                ref = g[f'{name}/pred{a}_{i}']
                err = np.abs(p.cpu().numpy() - ref) / (1 + np.abs(ref))
                assert err.max() <= tol, (dtype, a, i, err.max())
    # the post-network path does not depend on the dtype: the fp32 merge on the same pred maps, bit for bit
    want = det.bbox_head.aug_test_preds(preds, metas, rescale=True)[0]
    for c in range(6):
        assert np.array_equal(got[0][c], want[c]), c


def test_csp_head_aug_test_still_raises(gpu_device):
    scale = [['conv', 'bottleneck', 'csp', 'csp', 'csp', 'sppv4'], [None, 1, 1, 2, 2, 1], [8, 16, 32, 64, 128, 128]]
    det = pkg.build_detector(dict(
        type='SingleStageDetector', backbone=dict(type='DarknetCSP', scale=scale, out_indices=[3, 4, 5]),
        neck=dict(type='YOLOV4Neck', in_channels=[64, 128, 128], out_channels=[64, 128, 256], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=[64, 128, 256]), train_cfg=None,
        test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65),
                      max_per_img=300))).to(gpu_device).eval()
    img = torch.zeros((1, 3, 64, 64), device=gpu_device)
    metas = [[dict(img_shape=(64, 64, 3), scale_factor=np.ones(4, np.float32), flip=False)],
             [dict(img_shape=(64, 64, 3), scale_factor=np.ones(4, np.float32), flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match=r'aug_test \(TTA\) is not built'):
        det.forward_test([img, img], metas)
    with pytest.raises(NotImplementedError, match='YOLOCSPHead.aug_test'):
        det.bbox_head.aug_test(None, metas)


def test_inference_detector_and_single_gpu_test_with_flip(golden, gpu_device):
    g = golden('v3_tta')
    case = case_of(g, 'scales_hflip')
    det = build(gpu_device, case['test_cfg'])
    pipeline = [dict(type='LoadImageFromFile'),
                dict(type='MultiScaleFlipAug', img_scale=[(64, 48), (96, 64)], flip=True,
                     transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                 dict(type='Normalize', **IMG_NORM), dict(type='Pad', size_divisor=32),
                                 dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    src = g['scales_hflip/src']
    res = pkg.inference_detector(det, [src, src[:, ::-1].copy()], test_pipeline=pipeline)
    assert len(res) == 2 and all(len(r) == 6 for r in res)
    check_result(res[0], g, 'scales_hflip/result', box_tol=1e-3)   # the fixture's image through the whole path
    one = pkg.inference_detector(det, src, test_pipeline=pipeline)
    assert len(one) == 6
    # single_gpu_test: a loader item holds one batch per augmentation
    pipe = pkg.FusedTestPipeline.from_config(pipeline, device=gpu_device)
    batches, metas = pipe([src])
    results = pkg.single_gpu_test(det, [dict(img=batches, img_metas=metas)] * 2)
    assert len(results) == 2
    for r in results:
        check_result(r, g, 'scales_hflip/result', box_tol=1e-3)
