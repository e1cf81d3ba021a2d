"""The exact references of tests/_exact_ref.py on the CPU: they agree with torch's float64 convolution and gradients,
and the comparator catches a single one-unit change at a border tap of dW and at a corner pixel of dX."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ref as X  # noqa: E402


def test_references_match_torch_float64():
    X.check_refs_cpu()


def test_epilogue_reference_matches_torch_float64():
    X.check_epilogue_ref_cpu()


def test_epilogue_guard_counts_scales_shifts_residual_and_fractional_bits():
    """(conv * 2 + 3 + residual) * 2 + 3 with two slope-0.5 activations: the bound is the magnitude times 4."""
    ep = X.Epilogue(64, 0, 'cpu', True, X.ACT_LEAKY, True, X.ACT_LEAKY)
    s1, t1, s2, t2 = X.amax(ep.s1), X.amax(ep.t1), X.amax(ep.s2), X.amax(ep.t2)
    assert (s1, s2) == (2, 2) and t1 <= 3 and t2 <= 3
    assert ep.bound(1000, res_max=2) == ((1000 * s1 + t1 + 2) * s2 + t2) * 4
    assert X.Epilogue(64, 0, 'cpu', False).bound(1000) == 1000
    ep.guard(9 * 512, 2, 2, res_max=2)
    with pytest.raises(AssertionError, match='not exact'):
        ep.guard(2 ** 18, 2, 2, res_max=2)          # the convolution alone would pass: 2**20


def test_int_operand_values_and_seed():
    a = X.int_operand((3, 5, 7, 11), 4, 'cpu', torch.bfloat16)
    assert set(a.float().unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
    assert torch.equal(a, X.int_operand((3, 5, 7, 11), 4, 'cpu', torch.bfloat16))
    b = X.int_operand((1000,), 4, 'cpu', big=True)
    assert set(b.unique().tolist()) == {-1.0, 1.0}


def test_guard_refuses_inexact_cases():
    assert X.guard(64 * 304 * 304, 1, 1) < 2 ** 24
    with pytest.raises(AssertionError, match='not exact'):
        X.guard(64 * 608 * 608, 1, 1)
    with pytest.raises(AssertionError, match='not exact'):
        X.guard(2 ** 22, 2, 2, extra=0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_comparator_catches_one_unit(dtype):
    """One product more or less is one unit at an integer-valued result: the comparator must see it at the least
    covered places -- a border tap (kh, kw) = (0, 0) of dW and the corner pixel of dX -- and name the element."""
    N, H, W, Cin, Cout = 2, 9, 7, 8, 4
    x = X.int_operand((N, H, W, Cin), 1, 'cpu', dtype)
    w = X.int_operand((Cout, Cin, 3, 3), 2, 'cpu')
    dy = X.int_operand((N, H, W, Cout), 3, 'cpu', dtype)
    dw = X.wgrad_ref(x, dy, 3, 3, 1, 1)
    dx = X.dgrad_ref(dy, w, H, W, 1, 1)
    got_w, got_x = dw.float(), dx.to(dtype)
    X.assert_exact(got_w, dw, torch.float32, 'dW', X.WGRAD_NAMES)
    X.assert_exact(got_x, dx, dtype, 'dX')
    assert float(dx[0, 0, 0, 0].abs()) < 256      # (a corner sums 4 taps x 4 channels: one unit is visible in bf16)
    got_w[1, 0, 0, 2] += 1
    with pytest.raises(AssertionError, match=r'1 of .* differ; first at \(co=1, kh=0, kw=0, ci=2\)'):
        X.assert_exact(got_w, dw, torch.float32, 'dW', X.WGRAD_NAMES)
    got_x[0, 0, 0, 0] += 1
    with pytest.raises(AssertionError, match=r'1 of .* differ; first at \(n=0, h=0, w=0, c=0\)'):
        X.assert_exact(got_x, dx, dtype, 'dX')
