"""The references of tests/_pool_ref.py, checked on the CPU: the SPP backward against an explicit restatement of the
first-maximum rule, the resample references against F.interpolate and its autograd, the dilation against a loop, and
the operand makers against what they claim."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pool_ref as P  # noqa: E402
import _exact_ref as X  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SMALL = [(2, 3, 7, 9), (1, 2, 1, 1), (1, 2, 3, 11), (2, 1, 12, 2), (1, 1, 1, 17)]     # the last three: narrower / shorter than a window


def slow_spp_bwd(x, dcat):
    """The rule, restated: scan the border-clipped window in row-major order, move to an element only when it is
    strictly greater (so the first maximum stays, and -0 does not beat +0), give the pool's gradient to where the scan
    ended."""
    N, C, H, W = x.shape
    x, dcat = x.double(), dcat.double()
    dx = dcat[:, :C].clone()
    for n in range(N):
        for c in range(C):
            for k, K in enumerate(P.POOLS):
                r = K // 2
                for y in range(H):
                    for xx in range(W):
                        best, by, bx = None, -1, -1
                        for yy in range(max(0, y - r), min(H, y + r + 1)):
                            for xw in range(max(0, xx - r), min(W, xx + r + 1)):
                                v = float(x[n, c, yy, xw])
                                if best is None or v > best:
                                    best, by, bx = v, yy, xw
                        dx[n, c, by, bx] += dcat[n, (k + 1) * C + c, y, xx]
    return dx


@pytest.mark.parametrize('maker', [P.tie_map, P.distinct_map], ids=['tie', 'distinct'])
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_spp_backward_reference_is_the_first_maximum_rule(shape, maker):
    N, C, H, W = shape
    x = maker(shape, torch.float32, 3)
    if maker is P.tie_map and H * W > 1:
        x.view(-1)[:2] = torch.tensor([-0.0, 0.0])              # a -0 ahead of a +0 inside one window
    dcat = X.int_operand((N, 4 * C, H, W), 4, 'cpu')
    ref, terms = P.spp_cat_bwd_ref(x, dcat, return_terms=True)
    assert torch.equal(ref, slow_spp_bwd(x, dcat))
    assert float(ref.abs().max()) <= 2 * P.SPP_MAX_TERMS and float(terms.max()) <= 1 + 25 + 81 + 169
    assert float(terms.sum()) == 4 * x.numel()                   # every gradient lands exactly once
    # channels_last input: the same rule
    assert torch.equal(P.spp_cat_bwd_ref(x.contiguous(memory_format=torch.channels_last), dcat), ref)
    # and autograd of the forward agrees
    xr = x.double().requires_grad_(True)
    torch.cat([xr] + [F.max_pool2d(xr, k, 1, k // 2) for k in P.POOLS], 1).backward(dcat.double())
    assert torch.equal(xr.grad, ref)


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_spp_forward_reference(shape):
    x = P.distinct_map(shape, torch.float32, 5)
    N, C, H, W = shape
    got = P.spp_cat_ref(x)
    assert got.shape == (N, 4 * C, H, W) and torch.equal(got[:, :C], x.double())
    for k, K in enumerate(P.POOLS):
        r = K // 2
        xp = F.pad(x.double(), (r, r, r, r), value=float('-inf'))
        want = xp.unfold(2, K, 1).unfold(3, K, 1).amax((4, 5))
        assert torch.equal(got[:, (k + 1) * C:(k + 2) * C], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_operand_makers_deliver_what_they_claim(dtype):
    for shape in [(2, 3, 7, 9), (1, 2, 40, 36), (1, 1, 513, 1)]:
        m = P.distinct_map(shape, dtype, 7)
        assert m.dtype == dtype and m.shape == shape and bool(torch.isfinite(m).all())
        planes = m.double().view(shape[0] * shape[1], -1)
        for p in planes:
            assert p.unique().numel() == p.numel() and p.abs().unique().numel() == p.numel()
        assert float(planes.abs().min()) >= 1.0                  # normal range in every type
        if planes.shape[0] > 1:
            assert not torch.equal(planes[0], planes[1])
        if shape[2] * shape[3] > 1:
            assert bool((planes < 0).any()) and bool((planes > 0).any())
        if dtype == torch.float32:                               # bf16 patterns, widened
            assert torch.equal(m, P.distinct_map(shape, torch.bfloat16, 7).float())
        assert torch.equal(P.distinct_map(shape, dtype, 7), m)
    t = P.tie_map((2, 3, 7, 9), dtype, 1)
    assert t.dtype == dtype and set(t.double().unique().tolist()) == {-1.0, 0.0, 1.0}
    assert bool((torch.signbit(t) & (t == 0)).any()) and bool((~torch.signbit(t) & (t == 0)).any())
    idx5 = P.spp_argmax(t)[0]
    centre = torch.arange(7 * 9).view(1, 1, 7, 9)
    assert float((idx5 != centre).double().mean()) > 0.5         # ties everywhere: most windows' argmax is not trivially found


@pytest.mark.parametrize('geom', [(7, 9, 14, 18), (5, 5, 5, 5), (6, 4, 24, 16), (3, 5, 24, 10), (4, 3, 4, 24),
                                  (19, 19, 38, 38), (10, 10, 19, 19), (13, 13, 20, 20), (7, 9, 10, 31)])
def test_resample_references(geom):
    Hs, Ws, Hd, Wd = geom
    x = X.int_operand((2, 3, Hs, Ws), 11, 'cpu')
    want = F.interpolate(x.double(), size=(Hd, Wd), mode='nearest')
    assert torch.equal(P.resample_nearest_ref(x, Hd, Wd), want)
    assert torch.equal(P.resample_nearest_ref(x, Hd, Wd), F.interpolate(x, size=(Hd, Wd), mode='nearest').double())
    if Hd % Hs == 0 and Wd % Ws == 0:
        fy, fx = Hd // Hs, Wd // Ws
        dy = X.int_operand((2, 3, Hd, Wd), 12, 'cpu')
        xr = x.double().requires_grad_(True)
        F.interpolate(xr, size=(Hd, Wd), mode='nearest').backward(dy.double())
        got = P.resample_nearest_bwd_ref(dy, fy, fx)
        assert torch.equal(got, xr.grad)
        loop = torch.zeros(2, 3, Hs, Ws, dtype=torch.float64)
        for y in range(Hd):
            for xx in range(Wd):
                loop[:, :, y // fy, xx // fx] += dy[:, :, y, xx].double()
        assert torch.equal(got, loop)


def test_dilate_reference():
    src = X.int_operand((2, 3, 5, 7), 13, 'cpu')
    got = P.dilate2_ref(src)
    want = torch.zeros(2, 3, 10, 14, dtype=torch.float64)
    for y in range(5):
        for x in range(7):
            want[:, :, 2 * y, 2 * x] = src[:, :, y, x].double()
    assert torch.equal(got, want) and float((got != 0).sum()) == src.numel()
    # it is the data gradient's dilation: conv_transpose2d of a 1x1 unit kernel at stride 2, padded to 2H x 2W
    ct = F.conv_transpose2d(src.double(), torch.eye(3, dtype=torch.float64).view(3, 3, 1, 1), stride=2, output_padding=1)
    assert torch.equal(got, ct)
