"""Host side of the fused-loss tests (tests/_loss_ref.py, used by test_gpu_loss_exact.py): no GPU.

  * ``oracle.head_loss`` at its default float32 is what it was before it took ``dtype``: values and autograd gradients
    bit for bit against the restatement kept below, on the toy inputs of test_gpu_fused_loss.py.
  * every case builder's coverage assertions (computed from the oracle's assignment alone);
  * float64 against float32 of the reference itself on every case (same assignment by construction): ``e32``, the number
    the GPU bound ``4 * e32 + 8 * 2**-24`` is set from, is computed and printed here.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _loss_ref as R
from oracle import yolov4_oracle as O

ALL = list(R.CASES)


def _head_loss_before(pred_maps, gt_bboxes, gt_labels, num_classes, base_sizes, strides, one_hot_smoother):
    """``head_loss`` as it stood before the ``dtype`` argument (float32 throughout, classes required), default weights."""
    pred_maps = [p.float() for p in pred_maps]
    sizes = [p.shape[-2:] for p in pred_maps]
    resp = O.responsible_indices(sizes, gt_bboxes, 2, 4., base_sizes, strides)
    gtb, gtl = torch.cat(gt_bboxes, dim=0), torch.cat(gt_labels, dim=0)
    anchors = O.grid_anchors(sizes, base_sizes, strides)
    attr = 5 + num_classes
    out = []
    for lvl, pm in enumerate(pred_maps):
        img_ind, anc_ind, g_ind = resp[lvl]
        N = pm.shape[0]
        pmap = pm.permute(0, 2, 3, 1).reshape(N, -1, attr)
        pred_conf = pmap[..., 4]
        target_conf = torch.zeros_like(pred_conf)
        loss_bbox, loss_cls = pmap.new_zeros((1,)), pmap.new_zeros((1,))
        if anc_ind.numel():
            pos = pmap[img_ind, anc_ind]
            pb = pos[..., :4].sigmoid()
            box = O.bbox_decode(anchors[lvl][anc_ind], torch.cat((pb[..., :2] * 2. - 1., (pb[..., 2:] * 2.) ** 2.), dim=-1),
                                strides[lvl])
            giou_l = 1 - O.bbox_overlaps_giou_aligned(box, gtb[g_ind], eps=1e-6)
            loss_bbox = loss_bbox + giou_l.mean()
            tcls = F.one_hot(gtl[g_ind], num_classes=num_classes).float()
            if one_hot_smoother != 0:
                tcls = tcls * (1 - one_hot_smoother) + one_hot_smoother / num_classes
            loss_cls = loss_cls + 32. * F.binary_cross_entropy_with_logits(pos[..., 5:], tcls, reduction='none').mean()
            conf_t = (1 - giou_l).detach().clamp(0.0, 1.0)
            flat = img_ind * pred_conf.shape[1] + anc_ind
            last = torch.full((pred_conf.numel(),), -1, dtype=torch.long)
            last.scatter_reduce_(0, flat, torch.arange(flat.numel()), reduce='amax', include_self=True)
            target_conf = target_conf.reshape(-1)
            target_conf[flat] = conf_t[last[flat]]
            target_conf = target_conf.view(pred_conf.shape)
        loss_conf = 64. * F.binary_cross_entropy_with_logits(pred_conf, target_conf, reduction='none').mean()
        out.append((loss_cls, loss_conf * (4.0, 1.0, 0.4)[lvl], loss_bbox * 3.2))
    return out


@pytest.mark.parametrize('smoother', [0.0, 0.1])
def test_head_loss_float32_is_unchanged(smoother):
    """The toy inputs of test_gpu_fused_loss.py::test_fused_loss_matches_oracle_fp32, on the CPU."""
    C_, N, img = 5, 3, 96
    strides, base = [8, 16, 32], R.SMALL_BASE
    g = torch.Generator().manual_seed(1)
    maps = [torch.randn(N, 3 * (5 + C_), img // s, img // s, generator=g) * 1.5 for s in strides]
    gts = [torch.tensor([[20., 20., 44., 44.], [21., 21., 45., 43.], [0., 0., 14., 12.], [24., 40., 40., 56.]]),
           torch.tensor([[10., 30., 60., 70.], [50., 8., 90., 40.]]), torch.tensor([[33., 35., 80., 90.]])]
    labels = [torch.tensor([1, 3, 0, 2]), torch.tensor([4, 0]), torch.tensor([2])]
    res = []
    for fn in ('new', 'old'):
        leaves = [m.clone().requires_grad_(True) for m in maps]
        if fn == 'new':
            out = O.head_loss(leaves, gts, labels, num_classes=C_, base_sizes=base, strides=strides,
                              one_hot_smoother=smoother)
            rows = [(out['loss_cls'][l], out['loss_conf'][l], out['loss_bbox'][l]) for l in range(3)]
        else:
            rows = _head_loss_before(leaves, gts, labels, C_, base, strides, smoother)
        vals = torch.stack([torch.stack([v.reshape(()) for v in r]) for r in rows])
        (vals * R.gout_matrix(3)).sum().backward()
        res.append((vals.detach(), [x.grad for x in leaves]))
    assert res[0][0].dtype == torch.float32 and float(res[0][0].abs().min()) > 0
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert a.dtype == torch.float32 and torch.equal(a, b)


def test_head_loss_class_agnostic_has_no_class_term():
    g = torch.Generator().manual_seed(3)
    maps = [torch.randn(2, 15, 64 // s, 64 // s, generator=g).requires_grad_(True) for s in (8, 16, 32)]
    gts = [torch.tensor([[10., 12., 40., 44.]]), torch.tensor([[5., 5., 30., 50.], [20., 20., 60., 60.]])]
    out = O.head_loss(maps, gts, [torch.zeros(1, dtype=torch.long), torch.zeros(2, dtype=torch.long)], num_classes=0,
                      base_sizes=R.SMALL_BASE)
    assert all(float(v) == 0 for v in out['loss_cls'])
    assert all(float(v.detach()) > 0 for v in out['loss_conf']) and any(float(v.detach()) > 0 for v in out['loss_bbox'])


@pytest.mark.parametrize('name', ALL)
def test_case_coverage(name):
    """Building the case runs its coverage assertions (``check_coverage``) and the slot-order assertion."""
    case = R.get_case(name)
    assert case.name == name and len(case.assign) == case.L
    print(name, 'G', case.G, 'positives per level', [a.slot.numel() for a in case.assign])


@pytest.mark.parametrize('name', ALL)
def test_reference_float32_against_float64(name):
    """The reference's own fp32 evaluation against its float64 one: e32 exists, is finite and is of fp32 size (a
    float64 evaluation that had silently stayed in fp32 would give exactly 0 everywhere; a wrong one, something large)."""
    case, inputs, r64, e32 = R.references(name)
    assert r64.losses.dtype == torch.float64 and all(d.dtype == torch.float64 for d in r64.draw)
    print(f'{name}: e32 losses (L x [cls, conf, bbox])', [[f'{v:.2e}' for v in row] for row in e32.losses.tolist()])
    print(f'{name}: e32 conf_t {[f"{v:.2e}" for v in e32.conf_t]} draw {[f"{v:.2e}" for v in e32.draw]} '
          f'dbias {[f"{v:.2e}" for v in e32.dbias]}')
    every = e32.losses.reshape(-1).tolist() + e32.conf_t + e32.draw + e32.dbias
    assert all(math.isfinite(v) and v < 1e-4 for v in every), every
    assert max(e32.draw) > 0
    for l in range(case.L):                  # the float64 gradient is a gradient of these inputs: padding-free, full size
        assert tuple(r64.draw[l].shape) == (case.N,) + tuple(case.sizes[l]) + (case.co,)
