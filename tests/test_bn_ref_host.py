"""The BatchNorm + activation reference of tests/_bn_ref.py, checked on the CPU: it is the operation (against
torch.nn.functional.batch_norm and torch autograd in float64), its generators deliver what they claim, and the
integer-operand cases of tests/test_gpu_bn_exact.py are exact (every sum below 2**24)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_ref as B  # noqa: E402
import _exact_ref as X  # noqa: E402

ACTS = list(B.ACT_NAMES)
SLOPE = B.f32(0.1)
EPS = 1e-3


def _close(a, b, what):
    assert float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max())), what


def _inputs(M=53, C=12, seed=0):
    x = B._randn((M, C), seed, 'cpu') * 1.5 + 0.3
    dy, res = B._randn((M, C), seed + 1, 'cpu'), B._randn((M, C), seed + 2, 'cpu')
    gamma, beta = torch.linspace(-1.5, 1.5, C), torch.linspace(-0.4, 0.4, C)
    return x, dy, res, gamma, beta


def test_self_check():
    B.check_refs_cpu()


@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('act', ACTS, ids=[B.ACT_NAMES[a] for a in ACTS])
def test_train_mode_is_batch_norm_plus_autograd(act, with_res):
    x, dy, res, gamma, beta = _inputs()
    res = res if with_res else None
    M = x.shape[0]
    st = B.stats(x, EPS)
    y, S_y = B.forward(x, st['mean'], st['invstd'], gamma, beta, act, SLOPE, res)
    sums = B.backward_sums(x, dy, st['mean'], st['invstd'], gamma, beta, act, SLOPE)
    dx, S_dx = B.backward_dx(x, dy, st['mean'], st['invstd'], gamma, beta, act, SLOPE, sums, M)
    wy, wdx, wdg, wdb = B.torch_reference(x, dy, gamma, beta, EPS, act, SLOPE, res)
    _close(y, wy, 'y')
    _close(dx, wdx, 'dx')
    _close(sums['dgamma'], wdg, 'dgamma')
    _close(sums['dbeta'], wdb, 'dbeta')
    assert bool((S_y >= y.abs()).all()) and bool((S_dx > 0).all())
    # statistics against torch's own
    _close(st['mean'], x.double().mean(0), 'mean')
    _close(st['var'], x.double().var(0, unbiased=False), 'var')
    rm, rv = B.running(torch.zeros(12), torch.ones(12), st['mean'], st['var'], M, 0.03)
    bn = torch.nn.BatchNorm1d(12, eps=B.f32(EPS), momentum=B.f32(0.03)).double().train()
    bn(x.double())
    _close(rm, bn.running_mean, 'running_mean')
    _close(rv, bn.running_var, 'running_var')


@pytest.mark.parametrize('act', ACTS, ids=[B.ACT_NAMES[a] for a in ACTS])
def test_eval_mode_is_batch_norm_plus_autograd(act):
    x, dy, res, gamma, beta = _inputs(seed=5)
    rm, rv = torch.linspace(-0.5, 0.5, 12), torch.linspace(0.5, 2.0, 12)
    invstd = 1 / torch.sqrt(rv.double() + B.f32(EPS))
    y, _ = B.forward(x, rm, invstd, gamma, beta, act, SLOPE, res)
    sums = B.backward_sums(x, dy, rm, invstd, gamma, beta, act, SLOPE)
    dx, S_dx = B.backward_dx(x, dy, rm, invstd, gamma, beta, act, SLOPE, None, 0, eval_mode=True)
    wy, wdx, wdg, wdb = B.torch_reference(x, dy, gamma, beta, EPS, act, SLOPE, res, eval_stats=(rm, rv))
    for name, a, b in (('y', y, wy), ('dx', dx, wdx), ('dgamma', sums['dgamma'], wdg), ('dbeta', sums['dbeta'], wdb)):
        _close(a, b, name)


@pytest.mark.parametrize('act', ACTS, ids=[B.ACT_NAMES[a] for a in ACTS])
def test_two_way_row_split_reproduces_the_whole(act):
    """The SyncBN identity: sums of the halves add up to the whole's, and each half's dx from the totals over M_total
    rows is the whole's dx on those rows."""
    x, dy, _, gamma, beta = _inputs(M=64, seed=9)
    st = B.stats(x, EPS)
    args = (st['mean'], st['invstd'], gamma, beta, act, SLOPE)
    whole = B.backward_sums(x, dy, *args)
    dx, S = B.backward_dx(x, dy, *args, whole, 64)
    halves = [B.backward_sums(x[h], dy[h], *args) for h in (slice(0, 29), slice(29, 64))]
    tot = {k: halves[0][k] + halves[1][k] for k in whole}
    for k in whole:
        _close(tot[k], whole[k], k)
    for h in (slice(0, 29), slice(29, 64)):
        dxh, Sh = B.backward_dx(x[h], dy[h], *args, tot, 64)
        _close(dxh, dx[h], 'dx of a half')
        _close(Sh, S[h], 'S_dx of a half')


def test_leaky_at_zero_gives_slope():
    """z == 0 exactly (and -0.0): torch's leaky_relu_backward takes ``x > 0``, so the derivative there is ``slope``."""
    z = torch.tensor([0.0, -0.0, 1e-300, -1e-300], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, SLOPE).sum().backward()
    assert z.grad.tolist() == [SLOPE, SLOPE, 1.0, SLOPE]
    assert B.act_grad(z.detach(), B.ACT_LEAKY, SLOPE).tolist() == [SLOPE, SLOPE, 1.0, SLOPE]
    # through the whole backward: an input whose z is exactly zero on a third of a channel's rows
    c = B.settle_leaky(B.gen_leaky_zero(B.F32, 1206, 8, 3, 'cpu'))
    c.check_claims()
    sums = B.backward_sums(c.x, c.dy, c.mean, c.invstd, c.gamma, c.beta, B.ACT_LEAKY, SLOPE)
    z64, _ = c.z64()
    at0 = z64[:, 0] == 0
    want = (c.dy.double()[:, 0] * torch.where(z64[:, 0] > 0, 1.0, SLOPE)).sum()
    assert int(at0.sum()) == 402 and abs(float(sums['dbeta'][0] - want)) < 1e-12
    ge = (c.dy.double()[:, 0] * torch.where(z64[:, 0] >= 0, 1.0, SLOPE)).sum()
    assert abs(float(ge - want)) > 1e-3, 'the >= convention must be visible in dbeta on this input'


def test_fp32_counterpart_stays_near_float64():
    """K32 of the usual input is a small number: the scales are of the right order (an fp32 evaluation lands within a
    few u S of float64), and not so loose that K32 vanishes."""
    c = B.gen_usual(B.F32, 4099, 12, 1, 'cpu')
    args = (c.mean, c.invstd, c.gamma, c.beta, B.ACT_MISH, SLOPE)
    y64, S = B.forward(c.x, *args, c.res)
    y32, _ = B.forward(c.x, *args, c.res, dt=B.F32, want_scale=False)
    k, _ = B.k_of(y32, y64, S)
    assert 0.05 < k < 8, k
    s64 = B.backward_sums(c.x, c.dy, *args)
    s32 = B.backward_sums(c.x, c.dy, *args, dt=B.F32)
    dx64, Sdx = B.backward_dx(c.x, c.dy, *args, s64, c.M)
    dx32, _ = B.backward_dx(c.x, c.dy, *args, s32, c.M, dt=B.F32, want_scale=False)
    k, _ = B.k_of(dx32, dx64, Sdx)
    assert 0.05 < k < 8, k


def test_half_ulp_and_measure():
    v = torch.tensor([1.0, 1.5, 2.0, 3.0, 2.0 ** -20, 0.0], dtype=torch.float64)
    assert B.half_ulp(v, B.BF16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -28, 2.0 ** -134]
    assert B.half_ulp(v, B.F16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25]
    assert not B.half_ulp(v, B.F32).any()
    # rounding the exact value to the type costs at most 1 in the measure, whatever S is
    w = torch.linspace(-3, 3, 10001, dtype=torch.float64)
    for dt in (B.BF16, B.F16):
        assert B.k_of(w.to(dt), w, torch.zeros_like(w), dt)[0] <= 1.0
    assert B.k_of(torch.tensor([float('nan')]), torch.tensor([1.0], dtype=torch.float64), torch.ones(1))[0] == float('inf')
    assert B.k_of(torch.tensor([1.0]), torch.tensor([1.0], dtype=torch.float64), torch.zeros(1))[0] == 0.0
    assert B.k_of(torch.tensor([1.5]), torch.tensor([1.0], dtype=torch.float64), torch.zeros(1))[0] == float('inf')


# ---------------------------------------------------------------------------------------------------------------------
# the generators deliver what they claim
# ---------------------------------------------------------------------------------------------------------------------
DTYPES = [B.F32, B.BF16, B.F16]
_ids = {B.F32: 'f32', B.BF16: 'bf16', B.F16: 'f16'}


@pytest.mark.parametrize('dtype', DTYPES, ids=[_ids[d] for d in DTYPES])
def test_generators_deliver(dtype):
    M, C = 8208, 12
    for gen in (B.gen_usual, B.gen_const_channel, B.gen_tiny_std, B.gen_big_gamma, B.gen_gamma_signs, B.gen_leaky_zero):
        c = gen(dtype, M, C, 3, 'cpu')
        c.check_claims()
        B.settle_leaky(c)
        assert not bool(B.ambiguous(c).any())
        c.check_claims()                      # moving the ambiguous elements did not take away what the case is for
    for ratio in B.ratios_for(dtype):
        c = B.settle_leaky(B.gen_ratio(ratio, dtype, M, C, 3, 'cpu'))
        c.check_claims()
        assert float(c.ratio().min()) >= ratio
    if dtype != B.F16:
        c = B.gen_huge_gamma(dtype, M, C, 3, 'cpu')
        c.check_claims()
    else:
        B.gen_fp16_range(M, C, 3, 'cpu').check_claims()


def test_big_gamma_reaches_the_overflow_the_select_hides():
    """The forward's n = e (e + 2) overflows fp32 for some z of the big_gamma input, and the fp32 product z * a * e of the
    derivative overflows for some z of the huge_gamma input: the branches that must hide them are exercised."""
    z, _ = B.gen_big_gamma(B.F32, 8208, 12, 3, 'cpu').z64()
    e = torch.exp(z.clamp_max(88.0)).float()
    assert bool(torch.isinf(e * (e + 2)).any())
    z, _ = B.gen_huge_gamma(B.F32, 8208, 12, 3, 'cpu').z64()
    e20 = torch.exp(torch.tensor(20.0))
    assert bool(torch.isinf(z.float() * ((e20 + 1) * e20)).any())


def test_bn16_derivative_is_exactly_one_at_the_exact_cases():
    """The exact cases run Mish at beta = 64 (z >= 62).  The general kernels select 1 for z >= 20.  The pipelined ones
    evaluate 1 - u + zc (a e) u^2 with zc = 20, e = exp(20) and u = 2 / (a^2 + 1): in fp32 that is exactly 1 for any
    e within a relative 1e-3 of exp(20) (far more than the hardware exp2 and rcp can be off), and the forward
    z (n r) with n r = 1 - O(2**-24) rounds to z in either 16-bit type for integer z <= 68."""
    f = torch.float32
    for rel in (-1e-3, 0.0, 1e-3):
        e = (torch.exp(torch.tensor(20.0, dtype=torch.float64)) * (1 + rel)).to(f)
        a = e + 1
        for rel_u in (-1e-3, 0.0, 1e-3):
            u = (2.0 / (a.double() * a.double() + 1) * (1 + rel_u)).to(f)
            g = torch.tensor(20.0, dtype=f) * (a * e) * (u * u) + (1 - u)
            assert float(g) == 1.0
            n = e * (e + 2)
            nr = (n.double() / (n.double() + 2) * (1 + rel_u * 1e-4)).to(f)
            for zi in range(60, 69):
                for dt in (B.BF16, B.F16):
                    assert float((torch.tensor(float(zi), dtype=f) * nr).to(dt)) == float(zi)


# ---------------------------------------------------------------------------------------------------------------------
# the exact cases stay exact
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_cases_pass_the_guard():
    """Every integer-operand case of test_gpu_bn_exact.py: sums of M terms of |x| <= 2, |dy| <= 2 (dy * x <= 4) plus what
    publish == 2 starts from stay below 2**24; the largest layer-table maps use {-1, 1} and a lowered batch."""
    import test_gpu_bn_exact as G
    for (M, C) in G.COVER_SHAPES:
        X.guard(M, 2, 2, extra=G.ACCUM_BASE_MAX)
    for dtype, batch in G.TABLE_RUNS:
        for hw, C, _ in G.BN_SHAPES:
            M, big = G.table_rows(batch, hw)
            X.guard(M, 1 if big else 2, 1 if big else 2, extra=G.ACCUM_BASE_MAX)
            assert M <= batch * hw * hw
    # and the operand set itself
    t = X.int_operand((1000, 8), 1, 'cpu')
    assert set(t.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
