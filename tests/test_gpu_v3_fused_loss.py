"""YOLOv3 head loss on yv4_yolov3_loss_fwd / _bwd (csrc/loss_v3.hip) against the reference's YOLOV3Head.loss +
GridAssigner + PseudoSampler (tests/golden/v3_loss.npz, tests/golden/make_golden_v3_loss.py), against this
package's own tensor-op path at full size, and through a detector training step."""
import json

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import yolov3 as V3

pytestmark = pytest.mark.gpu

TERMS = ('loss_cls', 'loss_conf', 'loss_xy', 'loss_wh')


def _head(meta):
    return pkg.YOLOV3Head(num_classes=meta['C'], in_channels=[8, 8, 8], out_channels=[8, 8, 8],
                          train_cfg=dict(assigner=meta['assigner']), **meta['losses'], **meta['head'])


def _cases(g):
    return json.loads(str(g['meta']))


def _case_inputs(g, meta, dev, channels_last=False):
    p = meta['name'] + '/'
    maps = [torch.from_numpy(g[p + f'pred{l}']).to(dev) for l in range(3)]
    if channels_last:
        maps = [m.contiguous(memory_format=torch.channels_last) for m in maps]
    gts = [torch.from_numpy(g[p + f'gt{n}']).to(dev) for n in range(meta['N'])]
    labels = [torch.from_numpy(g[p + f'label{n}']).to(dev) for n in range(meta['N'])]
    return maps, gts, labels


def _run_fused(head, maps, gts, labels, gout):
    maps = [m.detach().clone().requires_grad_(True) for m in maps]
    out, assigned = V3.v3_fused_loss(head, maps, gts, labels)
    grads = torch.autograd.grad((out * gout).sum(), maps)
    return out.detach(), assigned, grads, maps


@pytest.mark.parametrize('channels_last', [False, True])
def test_v3_fused_loss_matches_reference_fixture(golden, gpu_device, channels_last):
    g = golden('v3_loss')
    for meta in _cases(g):
        p = meta['name'] + '/'
        head = _head(meta)
        maps, gts, labels = _case_inputs(g, meta, gpu_device, channels_last)
        assert head._fused_loss_ok(maps), meta['name']
        gout = torch.from_numpy(g[p + 'gout']).to(gpu_device)
        out, assigned, grads, _ = _run_fused(head, maps, gts, labels, gout)
        assigned = assigned.cpu().numpy()
        for n in range(meta['N']):
            np.testing.assert_array_equal(assigned[n], g[p + f'assigned{n}'], err_msg=f'{p}assigned{n}')
        np.testing.assert_allclose(out.cpu().numpy(), g[p + 'losses'], rtol=2e-5, atol=1e-6, err_msg=p + 'losses')
        for l in range(3):
            ref = g[p + f'grad{l}']
            got = grads[l]
            assert got.stride() == maps[l].stride()
            err = np.abs(got.cpu().numpy() - ref).max()
            assert err <= 2e-5 * max(np.abs(ref).max(), 1e-30), f'{p}grad{l}: {err}'


def test_v3_fused_loss_dict_matches_the_reference_losses(golden, gpu_device):
    """head.loss returns the reference's dict of per-level 0-d tensors."""
    g = golden('v3_loss')
    meta = _cases(g)[0]
    head = _head(meta)
    maps, gts, labels = _case_inputs(g, meta, gpu_device)
    losses = head.loss(maps, gts, labels, [dict() for _ in range(meta['N'])])
    assert list(losses) == list(TERMS)
    for k, key in enumerate(TERMS):
        assert len(losses[key]) == 3 and all(t.dim() == 0 for t in losses[key])
        np.testing.assert_allclose(torch.stack(losses[key]).cpu().numpy(), g[meta['name'] + '/losses'][:, k], rtol=2e-5)


def _recipe_head(num_classes=80):
    return pkg.YOLOV3Head(
        num_classes=num_classes, in_channels=[8, 8, 8], out_channels=[8, 8, 8],
        loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
        loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'),
        train_cfg=dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0)))


def _random_batch(dev, N=16, size=608, C=80, seed=5):
    gen = torch.Generator().manual_seed(seed)
    maps = [torch.randn(N, 3 * (5 + C), size // s, size // s, generator=gen).to(dev) for s in (32, 16, 8)]
    gts, labels = [], []
    for _ in range(N):
        k = int(torch.randint(0, 41, (1,), generator=gen))
        c = torch.rand(k, 2, generator=gen) * (size - 1)
        wh = 4 + torch.rand(k, 2, generator=gen) * 300
        b = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, size - 1)
        gts.append(b.to(dev))
        labels.append(torch.randint(0, C, (k,), generator=gen).to(dev))
    return maps, gts, labels


def test_v3_fused_loss_full_size_matches_the_tensor_op_path(gpu_device, monkeypatch):
    head = _recipe_head()
    maps, gts, labels = _random_batch(gpu_device)
    assert head._fused_loss_ok(maps)
    gout = torch.rand(3, 4, generator=torch.Generator().manual_seed(1)).to(gpu_device) + 0.5
    out, assigned, grads, _ = _run_fused(head, maps, gts, labels, gout)
    # the composed path's assignment, image by image
    sizes = [m.shape[-2:] for m in maps]
    anchors = torch.cat(head.anchor_generator.grid_anchors(sizes, gpu_device))
    for n in range(len(gts)):
        flags = torch.cat(head.anchor_generator.responsible_flags(sizes, gts[n], gpu_device))
        want = head.assigner.assign(anchors, flags, gts[n]).gt_inds
        assert torch.equal(assigned[n].long(), want), n
    monkeypatch.setenv('YV4_FUSED_LOSS', '0')
    assert not head._fused_loss_ok(maps)
    ref_maps = [m.detach().clone().requires_grad_(True) for m in maps]
    ref = head.loss(ref_maps, gts, labels, [dict() for _ in gts])
    mat = torch.stack([torch.stack(ref[k]) for k in TERMS], 1)
    ref_grads = torch.autograd.grad((mat * gout).sum(), ref_maps)
    np.testing.assert_allclose(out.cpu().numpy(), mat.detach().cpu().numpy(), rtol=2e-5)
    for l in range(3):
        err = (grads[l] - ref_grads[l]).abs().max().item()
        assert err <= 2e-5 * ref_grads[l].abs().max().item(), (l, err)


def test_v3_fused_loss_deterministic_mode_is_bitwise_repeatable(golden, gpu_device):
    """Under set_deterministic(True) the sums go through the fixed-point words (their lo halves are written; the default
    mode leaves them zero) and two runs give the same raw sum words, losses and gradients bit for bit."""
    head = _recipe_head()
    maps, gts, labels = _random_batch(gpu_device, N=8, seed=9)
    gout = torch.ones(3, 4, device=gpu_device)

    def run():
        scratch = {}
        maps_ = [m.detach().clone().requires_grad_(True) for m in maps]
        out, assigned = V3.v3_fused_loss(head, maps_, gts, labels, scratch=scratch)
        grads = torch.autograd.grad((out * gout).sum(), maps_)
        return out.detach(), assigned, grads, scratch['sums'].view(torch.int64).clone()

    was = pkg.deterministic()
    try:
        pkg.set_deterministic(False)
        plain = run()
        pkg.set_deterministic(True)
        a = run()
        b = run()
    finally:
        pkg.set_deterministic(was)
    assert not plain[3][1].any()                        # default mode: double sums only, lo words untouched
    assert a[3][1].any()                                # deterministic mode: fixed-point [hi | lo] words
    assert torch.equal(a[3], b[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    np.testing.assert_allclose(a[0].cpu().numpy(), plain[0].cpu().numpy(), rtol=1e-6)


def test_v3_fused_loss_gate_falls_back_unchanged(golden, gpu_device, monkeypatch):
    """An unsupported configuration (loss_wh=CrossEntropyLoss) takes the tensor-op path, with its own result."""
    g = golden('v3_loss')
    meta = _cases(g)[1]
    losses = dict(meta['losses'], loss_wh=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0,
                                                 reduction='sum'))
    head = _head(dict(meta, losses=losses))
    maps, gts, labels = _case_inputs(g, meta, gpu_device)
    assert not head._fused_loss_ok(maps)
    calls = []
    monkeypatch.setattr(V3.YoloV3LossFunction, 'apply', lambda *a: calls.append(1))
    got = head.loss(maps, gts, labels, [dict() for _ in gts])
    assert not calls
    monkeypatch.setenv('YV4_FUSED_LOSS', '0')
    want = head.loss(maps, gts, labels, [dict() for _ in gts])
    for k in TERMS:
        for x, y in zip(got[k], want[k]):
            assert torch.equal(x, y), k


def test_v3_train_step_takes_the_fused_loss(golden, gpu_device, monkeypatch):
    """YOLOV3.train_step on the tiny fixture model: the fused loss runs, and the parameter gradients match the
    tensor-op path's within the tolerances of test_gpu_v3.py::test_v3_train_step_matches_reference."""
    from test_gpu_v3 import TEST_CFG, build
    g = golden('tiny_v3')
    train_cfg = dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0))
    img = torch.from_numpy(g['img']).to(gpu_device)
    gtb = [torch.from_numpy(g[f'train/gt_bboxes{i}']).to(gpu_device) for i in range(2)]
    gtl = [torch.from_numpy(g[f'train/gt_labels{i}']).to(gpu_device) for i in range(2)]
    calls = []
    real = V3.YoloV3LossFunction.apply

    def spy(*a):
        calls.append(1)
        return real(*a)

    def step(fused):
        det = build(g, gpu_device)
        sd = det.state_dict()
        det.bbox_head = pkg.YOLOV3Head(
            num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32],
            loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
            loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
            loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
            loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'), train_cfg=train_cfg, test_cfg=TEST_CFG)
        det.load_state_dict(sd)
        det.to(gpu_device)
        det.training = True
        for m in (det.backbone, det.neck, det.bbox_head):
            torch.nn.Module.train(m, True)
        with monkeypatch.context() as mp:
            mp.setattr(V3.YoloV3LossFunction, 'apply', spy)
            if not fused:
                mp.setenv('YV4_FUSED_LOSS', '0')
            out = det.train_step(dict(img=img, img_metas=[dict(), dict()], gt_bboxes=gtb, gt_labels=gtl), None)
            out['loss'].backward()
        return out, {n: p.grad.detach().clone() for n, p in det.named_parameters()}

    out_f, grads_f = step(True)
    assert len(calls) == 1
    out_c, grads_c = step(False)
    assert len(calls) == 1
    for k in ('loss',) + TERMS:
        np.testing.assert_allclose(out_f['log_vars'][k], out_c['log_vars'][k], rtol=1e-4, err_msg=k)
        if k != 'loss':
            np.testing.assert_allclose(out_f['log_vars'][k], float(g['train/' + k].sum()), rtol=1e-4, err_msg=k)
    for n, gc in grads_c.items():
        gf = grads_f[n].double()
        gc = gc.double()
        np.testing.assert_allclose([float(gf.abs().sum()), float(gf.pow(2).sum().sqrt())],
                                   [float(gc.abs().sum()), float(gc.pow(2).sum().sqrt())], rtol=1e-2, atol=1e-5, err_msg=n)
    for k in ('bbox_head.convs_pred.0.bias', 'bbox_head.convs_pred.2.weight', 'backbone.conv1.conv.weight'):
        ref = grads_c[k].cpu().numpy()
        np.testing.assert_allclose(grads_f[k].cpu().numpy(), ref, rtol=1e-2, atol=2e-3 * float(np.abs(ref).max()) + 2e-5)
