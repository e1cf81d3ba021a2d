"""FP8 (OCP e4m3fn) inference kernels and plans on the GPU (csrc/conv_f8.hip, plan.Plan(dtype=torch.float8_e4m3fn)).

Contract: codes are e4m3(clamp(v * inv_s, +-448)) rounded to nearest even, bit-equal to torch's
conversion; the conv is bit-identical to a float64 conv on integer-valued operands; with real data each output code
equals the float64 emulation of the same quantized operands or differs by one code, for at most 0.2 % of the codes (0.13 % measured); a
larger distance only where the accumulation bound of _acc_bound covers it (near zero, where the code step is finest).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import plan as P
from mmdet_yolov4_amd.calibrate import calibrate_bn, calibrate_fp8

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
MAX_DIFF_FRAC = 2e-3       # codes off the float64 emulation: up to 1.25e-3 measured on a network layer
REL_L2_BOUND = 0.35        # pred maps of the fp8 plan vs the fp32 plan: 0.275 measured (YOLOv4-S 416)


def _lib():
    return pkg._lib.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ord(codes):
    """e4m3 codes (uint8 tensor) -> integers in code order (sign-magnitude; -0 and +0 both 0)."""
    c = codes.to(torch.int32)
    mag = c & 0x7F
    return torch.where(c & 0x80 != 0, -mag, mag)


def _q(v, inv):
    return (v * inv).clamp(-448, 448).float().to(F8)


# ---- 1. quantize op ---------------------------------------------------------------------------------------------------
def _special_values():
    sub = [k * 2.0 ** -9 for k in range(8)]                      # every subnormal code and the smallest normal
    ties = []
    for e in range(-9, 9):                                       # midpoints between neighbouring codes
        for m in range(8):
            lo = (1 + m / 8) * 2.0 ** e if e >= -6 else None
            if lo is not None and lo * (1 + 1 / 16) <= 448:
                ties.append(lo + 2.0 ** e / 16)
    ties += [(k + 0.5) * 2.0 ** -9 for k in range(8)]
    big = [447.9, 448.0, 449.0, 464.0, 465.0, 480.0, 1e4, 3e38]
    vals = torch.tensor(sub + ties + big + [0.0], dtype=torch.float64)
    vals = torch.cat([vals, -vals, torch.tensor([-0.0], dtype=torch.float64)])
    return vals


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_quantize_op_matches_torch(gpu_device, dtype):
    torch.manual_seed(0)
    sp = _special_values()
    N, H, W, Cs, coff, Cq = 2, 7, 9, 48, 8, 32
    x = (torch.randn(N, H, W, Cs, dtype=torch.float64) * 3).to(dtype)
    flat = x[..., coff:coff + Cq].reshape(-1)
    flat[:sp.numel()] = sp.to(dtype)                                      # inv_s = 1: the special values as they are
    x[..., coff:coff + Cq] = flat.view(N, H, W, Cq)
    for inv in (1.0, 3.7):
        xd = x.to(gpu_device).contiguous()
        y = torch.full((N, H, W, 40), 0x55, dtype=torch.uint8, device=gpu_device)
        code = {torch.bfloat16: pkg._lib.BF16, torch.float32: pkg._lib.F32}[dtype]
        pkg._lib.check(_lib().yv4_quantize_f8(xd.data_ptr(), code, N, H, W, Cq, Cs, coff, y.data_ptr(), 40, 4,
                                              float(inv), _stream()), 'quantize')
        torch.cuda.synchronize()
        got = y.cpu()
        src = x[..., coff:coff + Cq].float()
        exp = _q(src * torch.tensor(inv, dtype=torch.float32), 1.0).view(torch.uint8)
        bad = (got[..., 4:4 + Cq] != exp)
        assert not bool(bad.any()), (inv, src[bad][:8].tolist(), got[..., 4:4 + Cq][bad][:8].tolist(), exp[bad][:8].tolist())
        assert bool((got[..., :4] == 0x55).all()) and bool((got[..., 4 + Cq:] == 0x55).all())    # nothing outside the view
        assert not bool(((got & 0x7F) == 0x7F).any())                                             # no NaN code


# ---- conv helpers -----------------------------------------------------------------------------------------------------
def _conv_f8(x8, w8, s1, t1, k, stride, Cout, out_f32, act1=(0, 0.0), s2=None, t2=None, act2=(0, 0.0), res8=None,
             r_scale=1.0, y_inv=1.0, xv=(None, 0), yv=(None, 0), rv=(None, 0), tile=0):
    """x8: (N, H, W, Cs) uint8 codes, the conv reads channels [xv[1], xv[1] + Cin); w8: (Cout, k*k*Cin) codes.  Output
    buffer (N, Ho, Wo, yv[0] or Cout) filled with a sentinel; returns it (fp32 or uint8)."""
    dev = x8.device
    N, H, W, Cs = x8.shape
    Cin = w8.shape[1] // (k * k)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ycs = yv[0] or Cout
    y = (torch.full((N, Ho, Wo, ycs), -7.0, device=dev) if out_f32
         else torch.full((N, Ho, Wo, ycs), 0x55, dtype=torch.uint8, device=dev))
    d = pkg._lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, Ho, Wo, Cout
    d.KH = d.KW = k
    d.stride, d.pad = stride, pad
    d.x_cstride, d.x_coff = Cs, xv[1]
    d.y_cstride, d.y_coff = ycs, yv[1]
    if res8 is not None:
        d.r_cstride, d.r_coff = res8.shape[-1], rv[1]
    d.act1, d.slope1 = act1
    d.act2, d.slope2 = act2
    d.tile = tile
    keep = [s1.to(dev).float().contiguous(), t1.to(dev).float().contiguous()]
    if s2 is not None:
        keep += [s2.to(dev).float().contiguous(), t2.to(dev).float().contiguous()]
    pkg._lib.check(_lib().yv4_conv_bn_act_fwd_f8(
        C.byref(d), pkg._lib.F32 if out_f32 else pkg._lib.F8E4M3, x8.data_ptr(), w8.data_ptr(), keep[0].data_ptr(),
        keep[1].data_ptr(), keep[2].data_ptr() if s2 is not None else None, keep[3].data_ptr() if s2 is not None else None,
        res8.data_ptr() if res8 is not None else None, float(r_scale), float(y_inv), y.data_ptr(), _stream()), 'conv f8')
    torch.cuda.synchronize()
    return y


def _acc64(xv, w8, k, stride):
    """float64 conv of the code VALUES: xv (N, H, W, Cin) float64 on the device, w8 (Cout, k*k*Cin) codes -> (N, Ho, Wo,
    Cout) float64 (unfold + dgemm, exact for the integer data of the operand-map test)."""
    N, H, W, Cin = xv.shape
    Cout = w8.shape[0]
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(xv.permute(0, 3, 1, 2), k, padding=pad, stride=stride)          # (N, Cin*k*k, L), (ci, kh, kw)
    w = w8.view(F8).double().view(Cout, k, k, Cin).permute(0, 3, 1, 2).reshape(Cout, Cin * k * k)
    out = torch.matmul(w, cols)                                                      # (N, Cout, L)
    return out.view(N, Cout, Ho, Wo).permute(0, 2, 3, 1)


def _codes_of_ints(t):
    return t.float().to(F8).view(torch.uint8)


# ---- 2. operand map, exact ----------------------------------------------------------------------------------------------
MAP_CASES = [
    # k, stride, Cin, Cout, N, H, W
    (1, 1, 16, 32, 2, 9, 7),
    (3, 1, 32, 64, 2, 11, 13),
    (3, 2, 64, 255, 1, 17, 15),
    (3, 1, 96, 256, 1, 10, 12),
    (1, 1, 128, 255, 3, 13, 11),
    (3, 2, 128, 64, 2, 20, 18),
    (3, 1, 512, 256, 1, 9, 8),
    (1, 1, 512, 32, 2, 12, 12),
]


@pytest.mark.parametrize('case', MAP_CASES, ids=lambda c: 'k%d_s%d_%dx%d' % (c[0], c[1], c[2], c[3]))
@pytest.mark.parametrize('tile', [0, 1, 3])
def test_conv_f8_operand_map_exact(gpu_device, case, tile):
    """Integer operands |v| <= 8, unit scales, fp32 output: bit-identical to the float64 conv (every partial sum is an
    integer below 2^24).  Input / output views at channel offsets, a residual at its own offset."""
    k, stride, Cin, Cout, N, H, W = case
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + k)
    Cs, xoff = Cin + 32, 16
    xi = torch.randint(-8, 9, (N, H, W, Cs), generator=g)
    wi = torch.randint(-8, 9, (Cout, k * k * Cin), generator=g)
    x8 = _codes_of_ints(xi).to(gpu_device)
    w8 = _codes_of_ints(wi).to(gpu_device)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    ri = torch.randint(-8, 9, (N, Ho, Wo, Cout + 8), generator=g)
    r8 = _codes_of_ints(ri).to(gpu_device)
    ycs, yoff = Cout + 5, 3
    y = _conv_f8(x8, w8, torch.ones(Cout), torch.zeros(Cout), k, stride, Cout, True, res8=r8, rv=(None, 8),
                 xv=(None, xoff), yv=(ycs, yoff), tile=tile)
    ref = _acc64(xi[..., xoff:xoff + Cin].double().to(gpu_device), w8, k, stride) + ri[..., 8:8 + Cout].double().to(gpu_device)
    got = y[..., yoff:yoff + Cout].double()
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    assert bool((y[..., :yoff] == -7.0).all()) and bool((y[..., yoff + Cout:] == -7.0).all())


# ---- 3. full epilogue ---------------------------------------------------------------------------------------------------
def _act64(v, act):
    a, slope = act
    if a == pkg._lib.ACT_MISH:
        return v * torch.tanh(F.softplus(v))
    if a == pkg._lib.ACT_LEAKY:
        return torch.where(v >= 0, v, v * slope)
    if a == pkg._lib.ACT_SWISH:
        return v * torch.sigmoid(v)
    return v


def _emulate_codes(acc, s1f, t1, act1, res_val, r_scale, s2, t2, act2, y_inv):
    """float64 epilogue -> (value, codes, epi): epi bounds what the kernel's fp32 epilogue operations can move the value by
    (2^-21 of the magnitudes that meet in its sums, through the slopes), in the codes' scaled domain."""
    a = acc * s1f.double()
    mag = a.abs() + t1.double().abs()
    v = _act64(a + t1.double(), act1)
    mag = 1.2 * mag
    if res_val is not None:
        rv = res_val * float(r_scale)
        mag = mag + rv.abs() + v.abs()
        v = v + rv
    if s2 is not None:
        mag = 1.2 * (mag * s2.double().abs() + t2.double().abs())
        v = _act64(v * s2.double() + t2.double(), act2)
    return v, (v * float(y_inv)).clamp(-448, 448).float().to(F8).view(torch.uint8), mag * 2.0 ** -21 * float(y_inv)


def _acc_bound(xv, w8, k, stride, s1f, s2, y_inv):
    """Where the accumulation can move a value: the bound of a K-term fp32 sum, K * 2^-24 * sum|x*w| per output, with K
    taken as at least 1024 -- the matrix core's fp8 sums are not as tight as a sequential fp32 sum at small K (measured up
    to 1e-5 * sum|x*w| at K = 128 and 256) -- through |s1'|, an activation slope <= 1.2 and |s2|, in units
    of the output codes' scaled domain."""
    absacc = _acc64(xv.abs(), w8 & 0x7F, k, stride)
    K = max(w8.shape[1], 1024)
    b = absacc * (K * 2.0 ** -24) * s1f.double().abs() * 1.2
    if s2 is not None:
        b = b * s2.double().abs() * 1.2
    return b * float(y_inv)


def _check_codes(got, exp, what, bound=None):
    """Each code equals the emulation's or is one code away; a larger distance only where the fp32 accumulation bound
    covers it (near zero the e4m3 code step, 2^-9 of the scale, is finer than what summation order can move)."""
    got, exp = got.cpu(), exp.cpu()
    d = (_ord(got) - _ord(exp)).abs()
    far = d > 1
    if bool(far.any()):
        assert bound is not None, f'{what}: a code differs by {int(d.max())}'
        dv = (got.view(F8).double() - exp.view(F8).double()).abs()
        ok = dv <= 2.0 * bound.cpu() + 2.0 ** -9
        nfar = int((far & ~ok).sum())
        if nfar:
            print(f'{what}: {nfar} of {got.numel()} codes beyond one code and the bound')
        assert nfar == 0, f'{what}: {nfar} codes differ by more than one code and the bound'
    frac = float((d != 0).double().mean())
    assert frac <= MAX_DIFF_FRAC, f'{what}: {frac:.2e} of the codes differ'
    return frac


ACTS = [(pkg._lib.ACT_MISH, 0.0), (pkg._lib.ACT_LEAKY, 0.1), (pkg._lib.ACT_SWISH, 0.0), (pkg._lib.ACT_NONE, 0.0)]


@pytest.mark.parametrize('act', ACTS, ids=['mish', 'leaky', 'silu', 'none'])
@pytest.mark.parametrize('shape', [(3, 1, 64, 128), (1, 1, 256, 96), (3, 2, 128, 256)], ids=['3x3', '1x1', '3x3s2'])
def test_conv_f8_full_epilogue(gpu_device, act, shape):
    k, stride, Cin, Cout = shape
    N, H, W = 2, 19, 17
    g = torch.Generator().manual_seed(Cin + Cout + act[0])
    x8 = _q(torch.randn(N, H, W, Cin, generator=g) * 100, 1.0).view(torch.uint8).to(gpu_device)
    wq, sw = P.quantize_weight_f8(torch.randn(Cout, k * k * Cin, generator=g) * 0.05)
    w8 = wq.view(torch.uint8).to(gpu_device)
    sx = 0.01
    s1 = torch.rand(Cout, generator=g) + 0.5
    s1f = P.fold_s1_f8(s1, sw, sx)
    t1 = torch.randn(Cout, generator=g) * 0.2
    s2, t2 = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    r8 = _q(torch.randn(N, Ho, Wo, Cout, generator=g) * 50, 1.0).view(torch.uint8).to(gpu_device)
    r_scale, sy = 0.02, 0.005
    y_inv = P.f8_inv(sy)
    y = _conv_f8(x8, w8, s1f, t1, k, stride, Cout, False, act1=act, s2=s2, t2=t2, act2=act, res8=r8, r_scale=r_scale,
                 y_inv=y_inv)
    acc = _acc64(x8.view(F8).double(), w8, k, stride)
    _, exp, epi = _emulate_codes(acc, s1f.to(gpu_device), t1.to(gpu_device), act, r8.view(F8).double(), r_scale,
                                 s2.to(gpu_device), t2.to(gpu_device), act, y_inv)
    bound = _acc_bound(x8.view(F8).double(), w8, k, stride, s1f.to(gpu_device), s2.to(gpu_device), y_inv)
    frac = _check_codes(y, exp, f'{shape} {act}', bound + epi)
    print(f'{shape} {act}: {frac:.2e} of the codes differ from the float64 emulation')
    assert (exp != 0).float().mean() > 0.3          # the data exercise the codes, not just zeros / saturation


# ---- 4. SPP on codes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(13, 13), (19, 19), (40, 40)])
def test_spp_f8_exact(gpu_device, hw):
    H, W = hw
    N, Cc, coff, cs = 2, 64, 16, 16 + 4 * 64 + 16
    g = torch.Generator().manual_seed(H)
    v = _q(torch.randn(N, H, W, Cc, generator=g) * 30, 1.0)
    buf = torch.zeros(N, H, W, cs, dtype=torch.uint8)
    buf[..., coff:coff + Cc] = v.view(torch.uint8)
    bd = buf.to(gpu_device)
    pkg._lib.check(_lib().yv4_spp_pool_fwd_f8(bd.data_ptr(), N, H, W, Cc, cs, coff, _stream()), 'spp f8')
    torch.cuda.synchronize()
    got = bd.cpu()
    xs = v.float().permute(0, 3, 1, 2)
    for i, kk in enumerate((5, 9, 13)):
        ref = F.max_pool2d(xs, kk, 1, kk // 2).permute(0, 2, 3, 1).to(F8).float()
        out = got[..., coff + (i + 1) * Cc:coff + (i + 2) * Cc].view(F8).float()
        assert torch.equal(out, ref), kk
    assert torch.equal(got[..., :coff], buf[..., :coff]) and torch.equal(got[..., coff + 4 * Cc:], buf[..., coff + 4 * Cc:])


# ---- 5. / 6. networks ---------------------------------------------------------------------------------------------------
def _detector(model, size, batch, dev):
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg(model))
    det.init_weights()
    det.eval().to(dev)
    img = bench.synthetic_images(batch, size, 1000, dev)
    plan = det.compile(batch, size, size, device=dev, rescale=True)
    calibrate_bn(plan, img)
    bench.init_head(det, plan, img, 1500.0)
    det._engines.clear()
    calibrate_fp8(det, img)
    return det, img


def _view_codes(view):
    b = view.buf
    return b.tensor.view(torch.uint8).view(b.N, b.H, b.W, b.C)[..., view.coff:view.coff + view.C]


def _teacher_forced(plan):
    """Every fp8 conv recomputed in float64 from the plan's own input buffer, weights and scales."""
    worst, nconv = 0.0, 0
    for op in plan.ops:
        if op.kind != 'conv' or not op.info.get('f8'):
            continue
        L, d = op.info['launch'], op.info['desc']
        x = op.info['x']
        xv = _view_codes(x).view(F8).double()
        acc = _acc64(xv, L['w'].view(torch.uint8), d.KH, d.stride)
        res = op.info['residual']
        res_val = _view_codes(res).view(F8).double() if res is not None else None
        s2 = L['s2'] if L['s2'] is not None else None
        act1, act2 = (d.act1, d.slope1), (d.act2, d.slope2)
        v, exp, epi = _emulate_codes(acc, L['s1f'], L['t1'], act1, res_val, L['r_scale'], s2, L['t2'], act2, L['y_inv'])
        out = op.info['out']
        bound = _acc_bound(xv, L['w'].view(torch.uint8), d.KH, d.stride, L['s1f'], s2, L['y_inv'])
        if out.buf.dtype == torch.float32:      # fp32 pred maps: within the fp32 accumulation / epilogue bound
            got = out.buf.tensor.view(out.N, out.H, out.W, out.cstride)[..., out.coff:out.coff + out.C].double()
            tol = 2.0 * (bound + epi) + 1e-6 * (1.0 + v.abs())
            e = (got - v).abs()
            i = int((e / tol).argmax())
            assert bool((e <= tol).all()), (f'{op.name}: fp32 pred map off the emulation: {int((e > tol).sum())} values, worst '
                                            f'err {float(e.reshape(-1)[i]):.3e} tol {float(tol.reshape(-1)[i]):.3e} '
                                            f'value {float(v.reshape(-1)[i]):.4f} got {float(got.reshape(-1)[i]):.4f}')
        else:
            worst = max(worst, _check_codes(_view_codes(out), exp, op.name, bound + epi))
        nconv += 1
    return nconv, worst


@pytest.mark.parametrize('model,size,batch', [('yolov4l', 608, 2), ('yolov4s', 416, 2), ('yolov5l', 640, 1)])
def test_fp8_plan_teacher_forced(gpu_device, model, size, batch):
    det, img = _detector(model, size, batch, gpu_device)
    plan = det.compile(batch, size, size, device=gpu_device, rescale=True, dtype=F8)
    plan.run(img)
    torch.cuda.synchronize()
    nconv, worst = _teacher_forced(plan)
    assert nconv >= 60
    print(f'{model}: {nconv} fp8 convs, worst fraction of differing codes {worst:.2e}')


def _pred_maps(plan):
    return [v.buf.tensor.view(v.N, v.H, v.W, v.C).clone() for v in plan.pred_views]


def test_fp8_plan_end_to_end(gpu_device):
    det, img = _detector('yolov4s', 416, 4, gpu_device)
    eager = det.compile(4, 416, 416, device=gpu_device, rescale=True, dtype=F8)
    eager.run(img)
    a = _pred_maps(eager)
    eager.run(img)
    b = _pred_maps(eager)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two eager runs differ'
    graph = det.compile(4, 416, 416, device=gpu_device, rescale=True, graph=True, dtype=F8)
    graph.run(img)
    c = _pred_maps(graph)
    assert all(torch.equal(x, y) for x, y in zip(a, c)), 'hipGraph replay differs from the eager run'
    ref = det.compile(4, 416, 416, device=gpu_device, rescale=True, dtype=torch.float32)
    ref.run(img)
    r = _pred_maps(ref)
    num = sum(float((x.double() - y.double()).pow(2).sum()) for x, y in zip(a, r))
    den = sum(float(y.double().pow(2).sum()) for y in r)
    rel = math.sqrt(num / den)
    print(f'yolov4s 416: relative L2 of the fp8 pred maps from the fp32 plan {rel:.4f}')
    assert rel < REL_L2_BOUND, rel
    # simple_test through the fp8 plan: the reference's result structure
    det.compute_dtype = F8
    metas = [dict(scale_factor=np.ones(4, dtype=np.float32)) for _ in range(4)]
    res = det.simple_test(img, metas, rescale=True)
    del det.compute_dtype
    assert len(res) == 4 and all(len(r) == 80 for r in res)
    assert all(x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 5 for r in res for x in r)
    assert sum(x.shape[0] for x in res[0]) > 0
