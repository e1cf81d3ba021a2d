"""YOLOv3 mstrain train pipeline kernel (csrc/augment_v3.hip) against the reference-made fixture
(tests/golden/v3_augment.npz) and the numpy float32 restatement (tests/_v3_aug_ref.py): the resized region, the flip, the
normalisation and the zero pad bit for bit -- every step of the kernel is an IEEE float32 / float64 add, multiply or
divide compiled without contraction, the same operations numpy performs, so no stage needs a bound -- boxes and labels
exact; the ragged batch; the seeded path; refused inputs; and a tiny YOLOV3 trained one step on the pipeline's output."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd.augment_v3 import FusedV3TrainPipeline

import _v3_aug_ref as R

pytestmark = pytest.mark.gpu


def _sources(rng, sizes, num_classes=80):
    out = []
    for (h, w) in sizes:
        k = rng.randint(1, 6)
        xy = rng.rand(k, 2) * [w * 0.6, h * 0.6]
        wh = rng.rand(k, 2) * [w * 0.4, h * 0.4] + 6
        b = np.concatenate([xy, np.minimum(xy + wh, [w, h])], 1).astype(np.float32)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 / w, yy * 255 / h, (xx + yy) * 255 / (w + h)], -1) + rng.randn(h, w, 3) * 40
        img = np.clip(base, 0, 255).astype(np.uint8)
        img[:5, :9] = 0                                              # v == 0 / v < 0 pixels, s == 0
        out.append((img, b, rng.randint(0, num_classes, k).astype(np.int64)))
    return out


def _dev(samples, dev):
    return [(torch.from_numpy(s[0]).to(dev), s[1], s[2]) for s in samples]


def _check_against_restatement(pipe, samples, out):
    N = len(samples)
    img = out['img'].cpu().numpy()
    assert not np.isnan(img).any()
    for n in range(N):
        p, meta = out['params'][n], out['img_metas'][n]
        want = R.pipeline(samples[n][0], p, pipe.mean, pipe.std, pipe.to_rgb, pipe.size_divisor, pipe.expand_fill)
        ph, pw = meta['pad_shape'][:2]
        assert want.shape == (3, ph, pw)
        np.testing.assert_array_equal(img[n, :, :ph, :pw], want)
        assert not img[n, :, ph:].any() and not img[n, :, :, pw:].any()
        h, w = samples[n][0].shape[:2]
        b, l, sf = pipe.transform_boxes(p, h, w, samples[n][1], samples[n][2])
        np.testing.assert_array_equal(out['gt_bboxes'][n].cpu().numpy(), b)
        np.testing.assert_array_equal(out['gt_labels'][n].cpu().numpy(), l)
        assert out['gt_labels'][n].dtype == torch.int64 and out['gt_bboxes'][n].dtype == torch.float32


def test_fixture_cases_bit_for_bit(golden, gpu_device):
    """Every fixture case, run with the recorded draws: the image (resized region, flip, normalisation, zero pad) equals
    the fixture bit for bit, boxes and labels exactly (labels int64), metas as the reference's."""
    g = golden('v3_augment')
    pipe = FusedV3TrainPipeline(**R.fixture_kwargs(g))
    cases = R.fixture_cases(g)
    for c in cases:
        out = pipe([(torch.from_numpy(c['src']).to(gpu_device), c['boxes'], c['labels'])], params=[c['p']])
        got = out['img'].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (1,) + c['img'].shape
        np.testing.assert_array_equal(got[0], c['img'])
        assert not np.isnan(got).any()
        np.testing.assert_array_equal(got[0].view(np.uint32), c['img'].view(np.uint32))      # the bits, zero signs included
        np.testing.assert_array_equal(out['gt_bboxes'][0].cpu().numpy(), c['out_boxes'])
        np.testing.assert_array_equal(out['gt_labels'][0].cpu().numpy(), c['out_labels'])
        assert out['gt_labels'][0].dtype == torch.int64 and out['gt_bboxes'][0].is_cuda
        m = out['img_metas'][0]
        assert (m['ori_shape'], m['img_shape'], m['pad_shape']) == (c['ori_shape'], c['img_shape'], c['pad_shape'])
        np.testing.assert_array_equal(m['scale_factor'], c['scale_factor'])
        assert m['flip'] == c['flip'] and m['flip_direction'] == c['p']['flip']
        assert m['img_norm_cfg']['to_rgb'] == pipe.to_rgb
        np.testing.assert_array_equal(m['img_norm_cfg']['mean'], pipe.mean)
    # all cases as one ragged batch
    out = pipe([(torch.from_numpy(c['src']).to(gpu_device), c['boxes'], c['labels']) for c in cases],
               params=[c['p'] for c in cases])
    img = out['img'].cpu().numpy()
    for n, c in enumerate(cases):
        ph, pw = c['pad_shape'][:2]
        np.testing.assert_array_equal(img[n, :, :ph, :pw], c['img'])


@pytest.mark.parametrize('direction', ['horizontal', 'vertical', 'diagonal'])
def test_ragged_batch_equals_batches_of_one(gpu_device, direction):
    """Images with different drawn scales come out as one (N, 3, Hmax, Wmax) tensor: each equals its batch-of-one result
    in its own region and is 0 elsewhere; every image also equals the restatement bit for bit (up- and down-scaling
    sources, all three flip directions, a non-zero mean)."""
    rng = np.random.RandomState(11)
    samples = _sources(rng, [(96, 128), (128, 96), (50, 75), (120, 160), (33, 47), (64, 64)])
    pipe = FusedV3TrainPipeline(img_scale=[(64, 64), (192, 192)], expand_ratio_range=(1, 2), expand_mean=(10, 20, 30),
                                min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9), flip_direction=direction,
                                mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375))
    draw = np.random.RandomState(2)
    params = [pipe.draw_params(draw, s[0].shape[0], s[0].shape[1], s[1]) for s in samples]
    dsamples = _dev(samples, gpu_device)
    out = pipe(dsamples, params=params)
    shapes = [m['pad_shape'][:2] for m in out['img_metas']]
    assert len(set(shapes)) > 1, 'the draws must give a ragged batch'
    Hmax, Wmax = max(s[0] for s in shapes), max(s[1] for s in shapes)
    assert out['img'].shape == (len(samples), 3, Hmax, Wmax) and Hmax % 32 == 0 and Wmax % 32 == 0
    assert any(p['flip'] for p in params) and not all(p['flip'] for p in params)
    _check_against_restatement(pipe, samples, out)
    for n in range(len(samples)):
        one = pipe([dsamples[n]], params=[params[n]])
        ph, pw = shapes[n]
        assert one['img'].shape == (1, 3, ph, pw)
        assert torch.equal(out['img'][n, :, :ph, :pw], one['img'][0])
        assert not out['img'][n, :, ph:].any() and not out['img'][n, :, :, pw:].any()
        assert torch.equal(out['gt_bboxes'][n], one['gt_bboxes'][0]) and torch.equal(out['gt_labels'][n], one['gt_labels'][0])


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_seeded_run_equals_the_params_path(gpu_device, seed):
    """The same RandomState seed through __call__(..., rng=) equals the params= path, and the restatement."""
    rng = np.random.RandomState(100 + seed)
    samples = _sources(rng, [(90, 120), (120, 90), (64, 100), (100, 64)])
    pipe = FusedV3TrainPipeline(img_scale=[(64, 64), (160, 160)], expand_ratio_range=(1, 2),
                                min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9))
    dsamples = _dev(samples, gpu_device)
    a = pipe(dsamples, rng=np.random.RandomState(seed))
    draw = np.random.RandomState(seed)
    params = [pipe.draw_params(draw, s[0].shape[0], s[0].shape[1], s[1]) for s in samples]
    b = pipe(dsamples, params=params)
    assert a['params'] == params
    assert torch.equal(a['img'], b['img'])
    for x, y in zip(a['gt_bboxes'] + a['gt_labels'], b['gt_bboxes'] + b['gt_labels']):
        assert torch.equal(x, y)
    _check_against_restatement(pipe, samples, a)


def test_bad_inputs_are_refused(gpu_device):
    rng = np.random.RandomState(0)
    (img, boxes, labels), = _sources(rng, [(64, 96)])
    pipe = FusedV3TrainPipeline(img_scale=[(32, 32), (64, 64)])
    d = torch.from_numpy(img).to(gpu_device)
    good = pipe([(d, boxes, labels)], rng=np.random.RandomState(0))
    assert good['img'].shape[0] == 1
    with pytest.raises(TypeError):
        pipe([(d.float(), boxes, labels)], rng=np.random.RandomState(0))              # not u8
    with pytest.raises(ValueError):
        pipe([(d[:, ::2], boxes, labels)], rng=np.random.RandomState(0))              # not dense along w
    with pytest.raises(TypeError, match='no CPU fallback'):
        pipe([(torch.from_numpy(img), boxes, labels)], rng=np.random.RandomState(0))  # CPU tensor
    with pytest.raises(TypeError):
        pipe([(d.permute(2, 0, 1).contiguous(), boxes, labels)], rng=np.random.RandomState(0))   # CHW
    with pytest.raises(ValueError):
        pipe([(d, np.zeros((len(boxes), 5), np.float32), labels)], rng=np.random.RandomState(0))  # wrong box shape
    with pytest.raises(ValueError):
        pipe([(d, boxes, labels[:-1])], rng=np.random.RandomState(0))                 # labels do not match boxes
    bad = dict(good['params'][0], expand=None, crop=(200, 0, 300, 40), rh=32, rw=32)
    with pytest.raises(ValueError):
        pipe([(d, boxes, labels)], params=[bad])                                      # a patch outside the canvas
    # a dense row pitch larger than 3 * w is accepted (a column slice of a wider image)
    wide = torch.from_numpy(np.concatenate([img, img], 1)).to(gpu_device)
    view = wide[:, :img.shape[1]]
    out = pipe([(view, boxes, labels)], params=good['params'])
    assert torch.equal(out['img'], good['img'])


def test_tiny_yolov3_trains_on_the_pipeline_output(golden, gpu_device):
    """End to end: a ragged multiple-of-32 batch from the pipeline through YOLOV3.forward_train and backward (the tiny
    model of the v3 loss tests): finite loss, non-zero gradients."""
    from test_gpu_v3 import TEST_CFG, build
    g = golden('tiny_v3')
    det = build(g, gpu_device)
    sd = det.state_dict()
    det.bbox_head = pkg.YOLOV3Head(
        num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32],
        loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
        loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'),
        train_cfg=dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0)),
        test_cfg=TEST_CFG)
    det.load_state_dict(sd)
    det.to(gpu_device)
    det.training = True
    for m in (det.backbone, det.neck, det.bbox_head):
        torch.nn.Module.train(m, True)
    rng = np.random.RandomState(3)
    samples = _sources(rng, [(96, 128), (128, 96), (80, 80), (100, 150)], num_classes=6)
    pipe = FusedV3TrainPipeline(img_scale=[(64, 64), (160, 160)], expand_ratio_range=(1, 2),
                                min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9))
    batch = pipe(_dev(samples, gpu_device), rng=np.random.RandomState(4))
    N, _, H, W = batch['img'].shape
    assert H % 32 == 0 and W % 32 == 0 and len({m['pad_shape'] for m in batch['img_metas']}) > 1
    assert sum(len(b) for b in batch['gt_bboxes']) > 0
    losses = det.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'])
    loss, log_vars = det._parse_losses(losses)
    assert torch.isfinite(loss).item() and float(loss) > 0
    loss.backward()
    grads = [p.grad for p in det.parameters() if p.requires_grad]
    assert all(gr is not None and torch.isfinite(gr).all().item() for gr in grads)
    assert float(det.backbone.conv1.conv.weight.grad.abs().sum()) > 0
    assert float(det.bbox_head.convs_pred[0].weight.grad.abs().sum()) > 0
