"""Exact references for convolutions on integer-valued operands (a helper module for the tests, not a conftest).

Small integers are exact in bf16, fp16 and fp32, and so are their products.  While every partial sum is an integer
below 2**24, every fp32 summation order gives the same exact value, so a correct kernel equals a float64 reference bit
for bit on any route and at any size; a 16-bit output is rounded once, which ``ref64.to(dtype)`` reproduces.  One
dropped, duplicated or misplaced product changes the result.  The fused forward epilogue stays exact as well on the
operands of ``Epilogue`` (scales from {1, 2}, integer shifts, an integer residual, a leaky slope of 0.5).

Tensors here are NHWC: x (N, H, W, Cin), dY / y (N, Ho, Wo, Cout); weights are (Cout, Cin, KH, KW) as torch has
them, weight gradients (Cout, KH, KW, Cin) as the kernels write them.  The references are sums over taps of shifted
matmuls in float64 (no im2col), taken a few images at a time so that the 608 x 608 layers fit.
"""
import torch
import torch.nn.functional as F

EXACT_LIMIT = 2 ** 24          # fp32 holds every integer below this exactly
_CHUNK_ELEMS = 1 << 26         # float64 elements per batch chunk of a reference (512 MB)


def int_operand(shape, seed, device, dtype=torch.float32, big=False):
    """Seeded integer-valued tensor from {-2, -1, 1, 2} (``big``: {-1, 1}, for long reductions).  Zero is excluded, so
    every term of every sum counts, border pixels included."""
    g = torch.Generator(device=device).manual_seed(seed)
    if big:
        r = torch.randint(0, 2, shape, generator=g, device=device, dtype=torch.int8)
        return (2 * r - 1).to(dtype)
    r = torch.randint(0, 4, shape, generator=g, device=device, dtype=torch.int8)
    return (r - 2 + (r >= 2).to(torch.int8)).to(dtype)


def amax(t):
    return int(t.abs().max().item()) if t.numel() else 0


def guard(terms, *maxima, extra=0, limit=EXACT_LIMIT):
    """Assert that a sum of ``terms`` products of operands bounded by ``maxima`` (plus ``extra``) stays exact in fp32."""
    bound = terms
    for m in maxima:
        bound *= m
    bound += extra
    assert bound < limit, f'worst-case partial sum {bound} is not below {limit}: the case is not exact'
    return bound


def out_size(H, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1


def _batch_step(per_image):
    return max(1, _CHUNK_ELEMS // max(1, per_image))


def _taps(xp, KH, KW, stride, Ho, Wo):
    for kh in range(KH):
        for kw in range(KW):
            yield kh, kw, xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]


def wgrad_ref(x, dy, KH, KW, stride, pad):
    """dW[co, kh, kw, ci] = sum over (n, ho, wo) of dy[n, ho, wo, co] * x[n, ho*s - p + kh, wo*s - p + kw, ci]."""
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    assert Ho == out_size(H, KH, stride, pad) and Wo == out_size(W, KW, stride, pad)
    dw = torch.zeros(Cout, KH, KW, Cin, dtype=torch.float64, device=x.device)
    step = _batch_step((H + 2 * pad) * (W + 2 * pad) * Cin + Ho * Wo * (Cout + Cin))
    for n0 in range(0, N, step):
        xp = F.pad(x[n0:n0 + step].double(), (0, 0, pad, pad, pad, pad))
        d = dy[n0:n0 + step].double().reshape(-1, Cout).t()
        for kh, kw, xs in _taps(xp, KH, KW, stride, Ho, Wo):
            dw[:, kh, kw, :] += d @ xs.reshape(-1, Cin)
    return dw


def dgrad_ref(dy, w, H, W, stride, pad, out_dtype=torch.float64):
    """dX[n, h, w, ci] = sum over taps of dy[n, ho, wo, co] * w[co, ci, kh, kw] with h = ho*s - p + kh; rows beyond the
    last window (odd sizes at stride 2) get nothing.  ``out_dtype``: rounded once per batch chunk."""
    N, Ho, Wo, Cout = dy.shape
    _, Cin, KH, KW = w.shape
    assert Ho == out_size(H, KH, stride, pad) and Wo == out_size(W, KW, stride, pad)
    w64 = w.double()
    Hp, Wp = max(H + 2 * pad, stride * (Ho - 1) + KH), max(W + 2 * pad, stride * (Wo - 1) + KW)
    out = torch.empty(N, H, W, Cin, dtype=out_dtype, device=dy.device)
    step = _batch_step(Hp * Wp * Cin + Ho * Wo * (Cout + Cin))
    for n0 in range(0, N, step):
        d = dy[n0:n0 + step].double()
        nb = d.shape[0]
        dxp = torch.zeros(nb, Hp, Wp, Cin, dtype=torch.float64, device=dy.device)
        for kh, kw, xs in _taps(dxp, KH, KW, stride, Ho, Wo):
            xs += (d.reshape(-1, Cout) @ w64[:, :, kh, kw]).view(nb, Ho, Wo, Cin)
        out[n0:n0 + nb] = dxp[:, pad:pad + H, pad:pad + W, :].to(out_dtype)
    return out


def fwd_ref(x, w, stride, pad, out_dtype=torch.float64):
    """y[n, ho, wo, co] = sum over taps of x[n, ho*s - p + kh, wo*s - p + kw, ci] * w[co, ci, kh, kw]."""
    N, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    Ho, Wo = out_size(H, KH, stride, pad), out_size(W, KW, stride, pad)
    w64 = w.double()
    out = torch.empty(N, Ho, Wo, Cout, dtype=out_dtype, device=x.device)
    step = _batch_step((H + 2 * pad) * (W + 2 * pad) * Cin + Ho * Wo * (Cout + Cin))
    for n0 in range(0, N, step):
        xp = F.pad(x[n0:n0 + step].double(), (0, 0, pad, pad, pad, pad))
        nb = xp.shape[0]
        acc = torch.zeros(nb * Ho * Wo, Cout, dtype=torch.float64, device=x.device)
        for kh, kw, xs in _taps(xp, KH, KW, stride, Ho, Wo):
            acc += xs.reshape(-1, Cin) @ w64[:, :, kh, kw].t()
        out[n0:n0 + nb] = acc.view(nb, Ho, Wo, Cout).to(out_dtype)
    return out


ACT_NONE, ACT_LEAKY = 0, 2     # YV4_ACT_NONE, YV4_ACT_LEAKY
EXACT_SLOPE = 0.5              # a leaky slope that keeps integers exact: one more fractional bit per activation


class Epilogue:
    """Operands of the fused epilogue ``y = act2((act1(conv * s1 + t1) + residual) * s2 + t2)`` that keep it exact in
    fp32: per-channel s from {1, 2} and t integers in [-3, 3] (seeded, fp32, on ``device``), the activations NONE or
    LEAKY with slope 0.5.  ``affine1`` False: s1 = 1, t1 = 0 (the entry points always take a first stage);
    ``two_stage`` False: no second stage at all.  The residual is the caller's (``int_operand``)."""

    def __init__(self, Cout, seed, device, affine1=True, act1=ACT_NONE, two_stage=False, act2=ACT_NONE):
        g = torch.Generator(device=device).manual_seed(seed)

        def st():
            s = torch.randint(1, 3, (Cout,), generator=g, device=device).float()
            t = torch.randint(-3, 4, (Cout,), generator=g, device=device).float()
            return s, t
        self.s1, self.t1 = st()
        self.s2, self.t2 = st()
        if not affine1:
            self.s1, self.t1 = torch.ones_like(self.s1), torch.zeros_like(self.t1)
        assert act1 in (ACT_NONE, ACT_LEAKY) and act2 in (ACT_NONE, ACT_LEAKY)
        self.act1, self.act2, self.two_stage = act1, act2 if two_stage else ACT_NONE, two_stage
        self.slope = EXACT_SLOPE

    def bound(self, conv_bound, res_max=0):
        """Worst-case magnitude after the whole epilogue times 2**(fractional bits): below EXACT_LIMIT, every
        intermediate and the result are exact in fp32 (a slope of 0.5 adds one fractional bit per activation, an
        integer affine none)."""
        b = conv_bound * amax(self.s1) + amax(self.t1)
        frac = 1 if self.act1 == ACT_LEAKY else 0
        b += res_max
        if self.two_stage:
            b = b * amax(self.s2) + amax(self.t2)
            frac += 1 if self.act2 == ACT_LEAKY else 0
        return b * 2 ** frac

    def guard(self, terms, *maxima, res_max=0):
        """``guard`` for the convolution's partial sums AND for the epilogue's result."""
        conv_bound = guard(terms, *maxima)
        return guard(1, self.bound(conv_bound, res_max))


def _act64(v, act, slope):
    return torch.where(v >= 0, v, v * slope) if act == ACT_LEAKY else v


def epilogue_ref(conv64, ep, residual=None):
    """The fused epilogue on a float64 convolution (N, Ho, Wo, Cout), every step in float64."""
    v = _act64(conv64 * ep.s1.double() + ep.t1.double(), ep.act1, ep.slope)
    if residual is not None:
        v = v + residual.double()
    if ep.two_stage:
        v = _act64(v * ep.s2.double() + ep.t2.double(), ep.act2, ep.slope)
    return v


def fwd_epilogue_ref(x, w, stride, pad, ep, residual=None):
    return epilogue_ref(fwd_ref(x, w, stride, pad), ep, residual)


REF_SHAPES_CPU = [(2, 7, 5, 3, 4, 3, 1, 1), (2, 9, 8, 5, 6, 3, 2, 1), (1, 6, 7, 4, 3, 1, 2, 0),
                  (3, 5, 5, 2, 3, 1, 1, 0), (1, 12, 11, 3, 2, 6, 2, 2), (2, 8, 8, 4, 5, 3, 2, 0)]


def check_epilogue_ref_cpu():
    """``fwd_epilogue_ref`` against F.conv2d plus the same expression written out in float64 (NCHW, F.leaky_relu), on
    the shapes of ``check_refs_cpu``, every combination of stages; the result is exact in fp32 (it survives the round
    trip) and below the guard's bound."""
    for i, (N, H, W, Cin, Cout, K, s, p) in enumerate(REF_SHAPES_CPU):
        x = int_operand((N, H, W, Cin), 1, 'cpu')
        w = int_operand((Cout, Cin, K, K), 2, 'cpu')
        Ho, Wo = out_size(H, K, s, p), out_size(W, K, s, p)
        res = int_operand((N, Ho, Wo, Cout), 3, 'cpu')
        conv = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, s, p)
        for affine1 in (False, True):
            for act1 in (ACT_NONE, ACT_LEAKY):
                for use_res in (False, True):
                    for two_stage, act2 in ((False, ACT_NONE), (True, ACT_NONE), (True, ACT_LEAKY)):
                        ep = Epilogue(Cout, 10 + i, 'cpu', affine1, act1, two_stage, act2)
                        assert set(ep.s2.tolist()) <= {1.0, 2.0} and ep.t2.abs().max() <= 3
                        c = lambda t: t.double()[None, :, None, None]
                        v = conv * c(ep.s1) + c(ep.t1) if affine1 else conv
                        if act1 == ACT_LEAKY:
                            v = F.leaky_relu(v, 0.5)
                        if use_res:
                            v = v + res.double().permute(0, 3, 1, 2)
                        if two_stage:
                            v = v * c(ep.s2) + c(ep.t2)
                            if act2 == ACT_LEAKY:
                                v = F.leaky_relu(v, 0.5)
                        got = fwd_epilogue_ref(x, w, s, p, ep, res if use_res else None)
                        assert torch.equal(got, v.permute(0, 2, 3, 1))
                        assert torch.equal(got.float().double(), got)
                        b = ep.guard(K * K * Cin, amax(x), amax(w), res_max=amax(res) if use_res else 0)
                        frac = (act1 == ACT_LEAKY) + (two_stage and act2 == ACT_LEAKY)
                        assert float(got.abs().max()) * 2 ** frac <= b
                        assert torch.equal(got * 2 ** frac, (got * 2 ** frac).round())


def check_refs_cpu():
    """The three references against F.conv2d and torch.nn.grad in float64 on the CPU, at small shapes covering 1x1,
    3x3 and 6x6 windows, stride 1 and 2, even and odd sizes."""
    for (N, H, W, Cin, Cout, K, s, p) in REF_SHAPES_CPU:
        x = int_operand((N, H, W, Cin), 1, 'cpu')
        w = int_operand((Cout, Cin, K, K), 2, 'cpu').double()
        Ho, Wo = out_size(H, K, s, p), out_size(W, K, s, p)
        dy = int_operand((N, Ho, Wo, Cout), 3, 'cpu')
        xn, dyn = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
        y = F.conv2d(xn, w, None, s, p).permute(0, 2, 3, 1)
        assert torch.equal(fwd_ref(x, w, s, p), y)
        dw = torch.nn.grad.conv2d_weight(xn, w.shape, dyn, s, p).permute(0, 2, 3, 1)
        assert torch.equal(wgrad_ref(x, dy, K, K, s, p), dw)
        dx = torch.nn.grad.conv2d_input(xn.shape, w, dyn, s, p).permute(0, 2, 3, 1)
        assert torch.equal(dgrad_ref(dy, w, H, W, s, p), dx)


def assert_exact(got, ref64, dtype=None, what='', names=('n', 'h', 'w', 'c')):
    """``got`` must equal ``ref64`` rounded once to ``dtype`` (default: got's own type) bit for bit.  On failure the
    message gives the number of wrong elements and the first one by its index names: ('co', 'kh', 'kw', 'ci') for a
    weight gradient, ('n', 'h', 'w', 'c') for a map."""
    dtype = dtype or got.dtype
    want = ref64.to(got.device).to(dtype)
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} != {tuple(want.shape)}'
    got = got.to(dtype)
    if torch.equal(got, want):
        return
    bad = got != want
    nbad = int(bad.sum().item())
    first = [int(i) for i in bad.nonzero()[0].tolist()]
    where = ', '.join(f'{k}={i}' for k, i in zip(names, first))
    raise AssertionError(f'{what}: {nbad} of {got.numel()} elements differ; first at ({where}): got '
                         f'{float(got[tuple(first)])}, want {float(want[tuple(first)])} (exact {float(ref64[tuple(first)])})')


WGRAD_NAMES = ('co', 'kh', 'kw', 'ci')
