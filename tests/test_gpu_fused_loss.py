"""The fused YOLOCSPHead loss (yv4_yolo_loss_fwd / _bwd: assignment, gather, decode, GIoU, BCE and the whole
conv-output gradient) against the oracle's head_loss (yolocsp_head.py:384-575 restated with torch CPU ops,
differentiated by autograd; index_put runs in order there, so duplicate positives resolve to the last one) and
against the package's own tensor-op path.  Tolerances: losses 2e-5 relative, gradients 2e-5 of the largest
entry for fp32 maps; 16-bit maps: the gradient is stored in 16 bits (bf16 4e-3 / fp16 1e-3 relative to max).

These are toy sizes (3 to 6 classes, square maps of 2 to 16 cells, at most 7 boxes per image).  The real sizes (80 classes,
608 x 608, the grid-stride loops), non-square maps, the hand-built edge cases, the assignment's integer outputs and the
per-element comparison with float64 are in test_gpu_loss_exact.py."""
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd.yolocsp_head import RawPredMap
from oracle import yolov4_oracle as O

pytestmark = pytest.mark.gpu

STRIDES = [8, 16, 32]
BASE = [[(10, 12), (16, 30), (30, 20)], [(30, 60), (60, 45), (58, 100)], [(100, 90), (150, 190), (300, 320)]]


def make_head(num_classes, dev, class_agnostic=False, smoother=0.0):
    return pkg.YOLOCSPHead(num_classes=num_classes, in_channels=[8, 8, 8], featmap_strides=STRIDES,
                           anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=BASE, strides=STRIDES),
                           class_agnostic=class_agnostic, one_hot_smoother=smoother).to(dev).train()


def make_maps(head, N, img, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    attr = head.num_attrib
    maps, leaves = [], []
    for l, s in enumerate(STRIDES):
        h = img // s
        co = 3 * attr
        cp = co + (-co) % (4 if dtype == torch.float32 else 8)
        raw = (torch.randn(N, cp, h, h, generator=g) * 1.5).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
        raw.requires_grad_(True)
        bias = (torch.randn(co, generator=g) * 0.5).to(dev).requires_grad_(True)
        maps.append(RawPredMap(raw, bias, 3, attr))
        leaves.append((raw, bias))
    return maps, leaves


def random_gts(N, img, num_classes, seed, per_img=(0, 7)):
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for n in range(N):
        k = int(torch.randint(per_img[0], per_img[1], (1,), generator=g))
        c = torch.rand(k, 2, generator=g) * img
        wh = torch.rand(k, 2, generator=g) * img * 0.5 + 4
        b = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, img)
        boxes.append(b)
        labels.append(torch.randint(0, max(num_classes, 1), (k,), generator=g))
    return boxes, labels


def oracle_run(leaves, A_attr, gts, labels, num_classes, smoother, class_agnostic, weights):
    """Dense fp32 pred maps (raw + bias) on the CPU through the oracle; returns losses and d/d(pred map)."""
    dense = []
    for raw, bias in leaves:
        d = (raw.detach()[:, :A_attr].float().cpu() + bias.detach().cpu().view(1, -1, 1, 1)).requires_grad_(True)
        dense.append(d)
    if class_agnostic:
        raise AssertionError('use tensor-op path as the checker for class_agnostic')
    out = O.head_loss(dense, [g.cpu() for g in gts], [l.cpu() for l in labels], num_classes=num_classes,
                      base_sizes=BASE, strides=STRIDES, one_hot_smoother=smoother)
    tot = sum(w * v for key in ('loss_cls', 'loss_conf', 'loss_bbox') for w, v in zip(weights[key], [x.sum() for x in out[key]]))
    tot.backward()
    return out, [d.grad for d in dense]


def flat(losses, key):
    return torch.stack([x.reshape(()) for x in losses[key]]).detach().double().cpu()


def run_pkg(head, maps, leaves, gts, labels, weights, fused):
    os.environ['YV4_FUSED_LOSS'] = '1' if fused else '0'
    try:
        for raw, bias in leaves:
            raw.grad = None
            bias.grad = None
        out = head.loss(maps, gts, labels, None)
        keys = [k for k in ('loss_cls', 'loss_conf', 'loss_bbox') if k in out]
        tot = sum(w * v for key in keys for w, v in zip(weights[key], [x.sum() for x in out[key]]))
        tot.backward()
        return out, [(r.grad.detach().clone(), b.grad.detach().clone()) for r, b in leaves]
    finally:
        os.environ.pop('YV4_FUSED_LOSS', None)


WEIGHTS = dict(loss_cls=[1.0, 0.7, 1.3], loss_conf=[0.9, 1.1, 1.0], loss_bbox=[1.2, 1.0, 0.8])   # upstream gradients


@pytest.mark.parametrize('smoother', [0.0, 0.1])
def test_fused_loss_matches_oracle_fp32(smoother):
    dev = torch.device('cuda', 0)
    C_, N, img = 5, 3, 96
    head = make_head(C_, dev, smoother=smoother)
    maps, leaves = make_maps(head, N, img, torch.float32, dev, 1)
    gts, labels = random_gts(N, img, C_, 2)
    # image 0: two different boxes centred in the same cell (duplicate anchor boxes, different GIoU), one box at
    # the image corner, one with its centre exactly on a cell boundary
    gts[0] = torch.tensor([[20., 20., 44., 44.], [21., 21., 45., 43.], [0., 0., 14., 12.], [24., 40., 40., 56.]])
    labels[0] = torch.tensor([1, 3, 0, 2])
    gts_d = [g.to(dev) for g in gts]
    labels_d = [l.to(dev) for l in labels]
    ref, ref_grads = oracle_run(leaves, 3 * head.num_attrib, gts, labels, C_, smoother, False, WEIGHTS)
    out, grads = run_pkg(head, maps, leaves, gts_d, labels_d, WEIGHTS, fused=True)
    for key in ('loss_cls', 'loss_conf', 'loss_bbox'):
        assert out[key][0].shape == ref[key][0].shape
        np.testing.assert_allclose(flat(out, key), flat(ref, key), rtol=2e-5, atol=1e-7)
    assert float(out['num_gts']) == float(ref['num_gts'])
    co = 3 * head.num_attrib
    for (draw, dbias), dref in zip(grads, ref_grads):
        d = draw[:, :co].float().cpu()
        assert float((d - dref).abs().max()) <= 2e-5 * float(dref.abs().max())
        assert float(draw[:, co:].abs().max()) == 0 if draw.shape[1] > co else True
        bref = dref.sum((0, 2, 3))
        assert float((dbias.cpu() - bref).abs().max()) <= 2e-5 * float(bref.abs().max()) + 1e-7


@pytest.mark.parametrize('dtype,tol', [(torch.bfloat16, 4e-3), (torch.float16, 1e-3)])
def test_fused_loss_16bit_maps(dtype, tol):
    dev = torch.device('cuda', 0)
    C_, N, img = 4, 2, 64
    head = make_head(C_, dev)
    maps, leaves = make_maps(head, N, img, dtype, dev, 5)
    gts, labels = random_gts(N, img, C_, 6, per_img=(2, 6))
    ref, ref_grads = oracle_run(leaves, 3 * head.num_attrib, gts, labels, C_, 0.0, False, WEIGHTS)
    out, grads = run_pkg(head, maps, leaves, [g.to(dev) for g in gts], [l.to(dev) for l in labels], WEIGHTS, True)
    for key in ('loss_cls', 'loss_conf', 'loss_bbox'):
        np.testing.assert_allclose(flat(out, key), flat(ref, key), rtol=2e-5, atol=1e-7)   # the loss itself is fp32
    co = 3 * head.num_attrib
    for (draw, dbias), dref in zip(grads, ref_grads):
        assert draw.dtype == dtype
        assert float((draw[:, :co].float().cpu() - dref).abs().max()) <= tol * float(dref.abs().max())
        bref = dref.sum((0, 2, 3))
        assert float((dbias.cpu() - bref).abs().max()) <= 2e-5 * float(bref.abs().max()) + 1e-7


@pytest.mark.parametrize('agnostic', [False, True])
def test_fused_equals_tensor_op_path(agnostic):
    """Same inputs through the package's two GPU paths (no duplicate positives here: the tensor-op path's
    index_put is order-dependent on the GPU)."""
    dev = torch.device('cuda', 0)
    C_, N, img = 6, 4, 128
    head = make_head(C_, dev, class_agnostic=agnostic, smoother=0.05)
    maps, leaves = make_maps(head, N, img, torch.float32, dev, 11)
    gts, labels = random_gts(N, img, C_, 12, per_img=(1, 3))
    gts_d, labels_d = [g.to(dev) for g in gts], [l.to(dev) for l in labels]
    a, ga = run_pkg(head, maps, leaves, gts_d, labels_d, WEIGHTS, fused=False)
    b, gb = run_pkg(head, maps, leaves, gts_d, labels_d, WEIGHTS, fused=True)
    assert set(a) == set(b) and ('loss_cls' in b) == (not agnostic)
    for key in a:
        if key != 'num_gts':
            np.testing.assert_allclose(flat(b, key), flat(a, key), rtol=2e-5, atol=1e-7)
    for (d1, b1), (d2, b2) in zip(ga, gb):
        assert float((d1 - d2).abs().max()) <= 2e-5 * float(d1.abs().max())
        assert float((b1 - b2).abs().max()) <= 2e-5 * float(b1.abs().max()) + 1e-7


def test_no_ground_truth_and_determinism():
    dev = torch.device('cuda', 0)
    C_, N, img = 3, 2, 64
    head = make_head(C_, dev)
    maps, leaves = make_maps(head, N, img, torch.float32, dev, 21)
    empty = [torch.zeros(0, 4, device=dev) for _ in range(N)]
    el = [torch.zeros(0, dtype=torch.long, device=dev) for _ in range(N)]
    out, grads = run_pkg(head, maps, leaves, empty, el, WEIGHTS, fused=True)
    assert all(float(x.detach()) == 0 for x in out['loss_cls'] + out['loss_bbox'])
    for (raw, bias), lc, bal in zip(leaves, out['loss_conf'], head.conf_level_balance_weight):
        x = raw.detach()[:, 4:3 * head.num_attrib:head.num_attrib].float() + bias.detach()[4::head.num_attrib].view(1, -1, 1, 1)
        want = torch.nn.functional.binary_cross_entropy_with_logits(x, torch.zeros_like(x)) * 64. * bal
        np.testing.assert_allclose(float(lc), float(want), rtol=2e-5)
    # duplicates everywhere (the same box eight times): results are bit-identical from run to run
    gts = [torch.tensor([[10., 12., 40., 44.]] * 4 + [[11., 12., 41., 43.]] * 4, device=dev) for _ in range(N)]
    labels = [torch.tensor([0, 1, 2, 0, 1, 2, 0, 1], device=dev) for _ in range(N)]
    first = None
    for _ in range(5):
        out, grads = run_pkg(head, maps, leaves, gts, labels, WEIGHTS, fused=True)
        sig = [flat(out, k) for k in ('loss_cls', 'loss_conf', 'loss_bbox')]
        if first is None:
            first = sig
        assert all(torch.equal(a, b) for a, b in zip(sig, first))         # the scatter is deterministic
