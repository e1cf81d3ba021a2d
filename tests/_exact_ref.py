"""Exact references for convolutions on integer-valued operands (a helper module for the tests, not a conftest).

Small integers are exact in bf16, fp16 and fp32, and so are their products.  While every partial sum is an integer
below 2**24, every fp32 summation order gives the same exact value, so a correct kernel equals a float64 reference bit
for bit on any route and at any size; a 16-bit output is rounded once, which ``ref64.to(dtype)`` reproduces.  One
dropped, duplicated or misplaced product changes the result.

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


def check_refs_cpu():
    """The three references against F.conv2d and torch.nn.grad in float64 on the CPU, at small shapes covering 1x1,
    3x3 and 6x6 windows, stride 1 and 2, even and odd sizes."""
    for (N, H, W, Cin, Cout, K, s, p) in [(2, 7, 5, 3, 4, 3, 1, 1), (2, 9, 8, 5, 6, 3, 2, 1), (1, 6, 7, 4, 3, 1, 2, 0),
                                          (3, 5, 5, 2, 3, 1, 1, 0), (1, 12, 11, 3, 2, 6, 2, 2), (2, 8, 8, 4, 5, 3, 2, 0)]:
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
