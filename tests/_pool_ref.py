"""Float64 references and exact operands for the data-movement kernels of a training step (a helper module for the
tests, not a conftest): the SPP concat and its backward, the nearest resample and its backward, the zero-dilation.

Tensors here are NCHW, as torch has them; the GPU tests permute into the kernels' NHWC views.

Tie rule of the SPP backward (what ATen's ``max_pool2d`` does and what ``spp_pool_bwd_kernel`` /
``spp_pool_bwd_lds_kernel`` document): a pool's gradient goes to the FIRST maximum of its border-clipped window in
row-major order, where ``-0 == +0``.  ``spp_cat_bwd_ref`` takes the argmax from ATen's float64 CPU kernel;
tests/test_pool_ref_host.py pins that against an explicit restatement of the rule.

Domain: every input is FINITE.  For NaN and for windows that hold nothing but ``-inf`` the two backward forms and the
forward differ from ATen and from each other; that is a known, separate matter which these references do not define.

Exactness.  ``distinct_map`` and ``tie_map`` give values that are exact in bf16, fp16 and fp32, so the maxima and their
positions are the same in every type.  With gradients from ``_exact_ref.int_operand`` ({-2, -1, 1, 2}) an SPP ``dx``
element sums at most 1 + 25 + 81 + 169 = 276 terms (<= 1 + 3 * 169), |dx| <= 552: an integer, exact in fp32 in any
order of the atomics, and a 16-bit result is ``ref64.to(dtype)``, one rounding.  A resample backward element sums
fy * fx <= 64 such terms.
"""
import numpy as np
import torch
import torch.nn.functional as F

POOLS = (5, 9, 13)
SPP_MAX_TERMS = 1 + 3 * 169
_BASE16 = {torch.bfloat16: 0x3F80, torch.float16: 0x3C00, torch.float32: 0x3F80}      # 1.0 (fp32: bf16 patterns, widened)


# ---- operands --------------------------------------------------------------------------------------------------------
def distinct_map(shape, dtype, seed):
    """(N, C, H, W): every (image, channel) plane is a seeded permutation of H*W distinct finite values that are exact in
    ``dtype``: consecutive bit patterns of the 16-bit type upwards from 1.0 (bf16 patterns widened for fp32) with random
    signs -- the magnitudes are distinct, so no two values of a plane are equal and no window has a tie."""
    N, C, H, W = shape
    HW = H * W
    t16 = torch.bfloat16 if dtype == torch.float32 else dtype
    base = _BASE16[dtype]
    top = 0x7F80 if t16 == torch.bfloat16 else 0x7C00               # the first non-finite pattern
    assert base + HW < top, f'{HW} consecutive patterns from {base:#x} leave the finite range'
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(N * C, HW, generator=g).argsort(1)
    mag = (base + perm).to(torch.int16).view(t16).float()
    sign = torch.randint(0, 2, (N * C, HW), generator=g).float() * 2 - 1
    return (mag * sign).view(N, C, H, W).to(dtype)


def tie_map(shape, dtype, seed):
    """(N, C, H, W) drawn from {-1, -0.0, +0.0, 1}: nearly every window has several maxima, and +0 / -0 meet."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-1.0, -0.0, 0.0, 1.0])
    return vals[torch.randint(0, 4, tuple(shape), generator=g)].to(dtype)


# ---- SPP -------------------------------------------------------------------------------------------------------------
def spp_cat_ref(x):
    """cat([x, mp5(x), mp9(x), mp13(x)], 1) in float64 (stride 1, padding k // 2, implicit -inf padding)."""
    x64 = x.detach().double().cpu().contiguous()
    return torch.cat([x64] + [F.max_pool2d(x64, k, 1, k // 2) for k in POOLS], 1)


def spp_argmax(x):
    """Per pool the flat (y * W + x) index of every window's first maximum, (N, C, H, W) int64, from ATen's float64 CPU
    kernel."""
    x64 = x.detach().double().cpu().contiguous()
    return [F.max_pool2d(x64, k, 1, k // 2, return_indices=True)[1] for k in POOLS]


def spp_cat_bwd_ref(x, dcat, return_terms=False):
    """dx (N, C, H, W) float64 = dcat[:, :C] + for each pool the scatter of its gradient to the window's first maximum.
    ``return_terms``: also the number of contributions each element received (identity included)."""
    N, C, H, W = x.shape
    HW = H * W
    d64 = dcat.detach().double().cpu().contiguous()
    assert d64.shape == (N, 4 * C, H, W)
    dx = d64[:, :C].clone().view(-1)
    terms = torch.ones(N * C * HW, dtype=torch.float64)
    plane = (torch.arange(N * C, dtype=torch.int64) * HW).view(N, C, 1, 1)
    for k, idx in enumerate(spp_argmax(x)):
        flat = (idx + plane).view(-1)
        dx.index_add_(0, flat, d64[:, (k + 1) * C:(k + 2) * C].reshape(-1))
        if return_terms:
            terms.index_add_(0, flat, torch.ones_like(terms))
    dx = dx.view(N, C, H, W)
    return (dx, terms.view(N, C, H, W)) if return_terms else dx


# ---- nearest resample ------------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out):
    """torch's 'nearest': src = min(floor(dst * scale), in - 1) with scale = in / out formed in float32."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(src, n_in - 1))


def resample_nearest_ref(x, Hd, Wd):
    """F.interpolate(x, size=(Hd, Wd), mode='nearest') in float64 as an index gather."""
    x64 = x.detach().double().cpu()
    return x64[:, :, nearest_index(x.shape[2], Hd)][:, :, :, nearest_index(x.shape[3], Wd)].contiguous()


def resample_nearest_bwd_ref(dy, fy, fx):
    """Backward of the resample by integer factors: dx[n, c, sy, sx] = the sum of the fy x fx pixels of dy that read it."""
    d64 = dy.detach().double().cpu()
    N, C, Hd, Wd = d64.shape
    assert Hd % fy == 0 and Wd % fx == 0
    return d64.view(N, C, Hd // fy, fy, Wd // fx, fx).sum((3, 5))


# ---- zero-dilation ---------------------------------------------------------------------------------------------------
def dilate2_ref(src):
    """dst[n, c, 2y, 2x] = src[n, c, y, x], everything else 0; dst is (N, C, 2H, 2W)."""
    s64 = src.detach().double().cpu()
    N, C, H, W = s64.shape
    dst = torch.zeros(N, C, 2 * H, 2 * W, dtype=torch.float64)
    dst[:, :, ::2, ::2] = s64
    return dst
