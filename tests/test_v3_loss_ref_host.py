"""Host side of the fused YOLOv3 loss tests (tests/_v3_loss_ref.py, used by test_gpu_v3_loss_exact.py): no GPU.

  * the reference is tied to the real implementation: on the nine cases of tests/golden/v3_loss.npz (made by the reference's
    own ``YOLOV3Head.loss`` + ``GridAssigner``) its discrete half reproduces every ``assigned{n}`` exactly and its float32
    continuous half the losses and gradients at the tolerance test_gpu_v3_fused_loss.py uses against that fixture;
  * every case's coverage assertions (computed from the reference's assignment alone);
  * ``e32``, the number the GPU bound ``4 * e32 + 8 * 2**-24`` is set from, is finite for every tensor of every case;
  * the inputs of the exact row count are exact in fp32: ``bce(64, 0) == 64``.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _v3_loss_ref as R

ALL = list(R.CASES)


def _fixture_case(g, meta):
    p = meta['name'] + '/'
    asg = meta['assigner']
    neg = asg['neg_iou_thr']
    losses = meta['losses']
    case = R._case(meta['name'], [32, 16, 8], R.V3_BASE_SIZES, [(2, 3), (4, 6), (8, 12)], meta['C'],
                   [torch.from_numpy(g[p + f'gt{n}']) for n in range(meta['N'])], seed=0,
                   assigner=dict(pos_iou_thr=float(asg['pos_iou_thr']), neg_iou_thr=float(neg) if not isinstance(neg, list) else tuple(neg),
                                 min_pos_iou=float(asg['min_pos_iou']), gt_max_assign_all=asg.get('gt_max_assign_all', True)),
                   smoother=meta['head'].get('one_hot_smoother', 0.0),
                   weights=[losses[k]['loss_weight'] for k in R.TERMS], reduction=[losses[k]['reduction'] for k in R.TERMS])
    case.labels = [torch.from_numpy(g[p + f'label{n}']).long() for n in range(meta['N'])]
    return case


def test_reference_reproduces_the_fixture(golden):
    g = golden('v3_loss')
    metas = json.loads(str(g['meta']))
    assert len(metas) == 9
    for meta in metas:
        p = meta['name'] + '/'
        case = _fixture_case(g, meta)
        asg = R.assign(case)
        for n in range(case.N):
            np.testing.assert_array_equal(asg.assigned[n].numpy(), g[p + f'assigned{n}'], err_msg=f'{p}assigned{n}')
        maps = [torch.from_numpy(g[p + f'pred{l}']) for l in range(3)]
        ref = R.reference(case, asg, maps, torch.float32, gout=torch.from_numpy(g[p + 'gout']))
        np.testing.assert_allclose(ref.losses.numpy(), g[p + 'losses'], rtol=2e-5, atol=1e-6, err_msg=p + 'losses')
        for l in range(3):
            want = g[p + f'grad{l}']
            err = np.abs(ref.grads[l].numpy() - want).max()
            assert err <= 2e-5 * max(np.abs(want).max(), 1e-30), f'{p}grad{l}: {err}'
        # the work-buffer tables agree with the assignment they explain
        assert asg.img_off.tolist() == np.cumsum([0] + [len(g[p + f'gt{n}']) for n in range(case.N)]).tolist()
        assert bool((asg.gt_cell >= 0).all())


@pytest.mark.parametrize('name', ALL + ['recipe'])
def test_case_coverage(name):
    """Building the case runs its coverage assertions."""
    case, asg = R.get_case(name)
    assert case.name == name and asg.assigned.shape == (case.N, asg.TA)
    a = asg.assigned
    print(name, 'G', case.G, 'rows', R.rows_of(case), 'positive / negative / ignored',
          int((a > 0).sum()), int((a == 0).sum()), int((a < 0).sum()))
    assert int(a.max()) <= max([int(b.shape[0]) for b in case.boxes]) and int(a.min()) >= -1
    assert asg.gt_max.shape == (case.G,) and asg.gt_cell.shape == (case.L, case.G) and asg.img_off.shape == (case.N + 1,)
    none = asg.gt_arg == R.NO_ARG
    assert bool(((asg.gt_max == R.MINUS_ONE_BITS) == none).all())
    assert bool((asg.gt_arg[~none] < asg.TA).all())


@pytest.mark.parametrize('name', ALL)
def test_reference_float32_against_float64(name):
    """e32 exists, is finite and of fp32 size for each of the 4L loss values and every (level, attribute group)."""
    case, asg, maps, r64, e32 = R.references(name)
    assert r64.losses.dtype == torch.float64 and all(x.dtype == torch.float64 for x in r64.grads)
    print(f'{name}: e32 losses (L x [cls, conf, xy, wh])', [[f'{v:.2e}' for v in row] for row in e32.losses.tolist()])
    print(f'{name}: e32 grads', {k: f'{v:.2e}' for k, v in e32.grads.items()})
    every = e32.losses.reshape(-1).tolist() + list(e32.grads.values())
    assert all(math.isfinite(v) and v < 1e-4 for v in every), every
    assert max(e32.grads.values()) > 0
    for l, (H, W) in enumerate(case.sizes):
        assert tuple(r64.grads[l].shape) == (case.N, case.A * (5 + case.C), H, W)
    if name == 'no_gt':
        assert float(r64.losses[:, [0, 2, 3]].abs().max()) == 0 and float(r64.losses[:, 1].min()) > 0
        for l in range(case.L):
            for gname, lo, hi in R.GROUPS:
                m = float(R.group_view(case, r64.grads[l], lo, hi).abs().max())
                assert (m > 0) == (gname == 'conf'), (l, gname, m)


def test_exact_count_inputs_are_exact_in_fp32():
    x = torch.tensor([64.0])
    assert float(F.binary_cross_entropy_with_logits(x, torch.zeros(1), reduction='none')) == 64.0
    assert 0 < float(F.binary_cross_entropy_with_logits(x.double(), torch.ones(1).double(), reduction='none')) < 2e-28
    for name in R.COUNT_CASES:
        case, asg = R.get_case(name)
        exp = R.count_expectation(case, asg)
        maps = R.exact_count_maps(case)
        attr = 5 + case.C
        for l, m in enumerate(maps):
            v = m.view(case.N, case.A, attr, *case.sizes[l])
            assert bool((v[:, :, 4:] == 64.0).all())
            # the fp32 sum of the negatives' objectness rows is the count itself, in a double
            assert 64.0 * exp[l][0] == float(64 * exp[l][0]) and 64.0 * (case.C - 1) * exp[l][1] < 2.0 ** 40
