"""FP8 (e4m3) inference: the C-ABI symbols, their argument validation and the host helpers of the fp8 plans, without a
GPU (tests/test_gpu_fp8.py runs the kernels)."""
import ctypes
import os
import re

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn
SYMS = ('yv4_conv_bn_act_fwd_f8', 'yv4_conv_f8_pick_tile', 'yv4_quantize_f8', 'yv4_spp_pool_fwd_f8')


def tiny_detector():
    """The CSPDarknet + PAN + head of __graft_entry__.smoke() (random init, eval mode, on the CPU)."""
    scale = [['conv', 'bottleneck', 'csp', 'csp', 'csp', 'sppv4'], [None, 1, 1, 2, 2, 1], [32, 64, 64, 128, 128, 128]]
    cfg = dict(type='SingleStageDetector',
               backbone=dict(type='DarknetCSP', scale=scale, out_indices=[3, 4, 5]),
               neck=dict(type='YOLOV4Neck', in_channels=[128, 128, 128], out_channels=[64, 128, 256], csp_repetition=1),
               bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=[64, 128, 256]),
               train_cfg=None,
               test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65),
                             max_per_img=300))
    torch.manual_seed(0)
    return pkg.build_detector(cfg).eval()


def test_fp8_symbols_declared_bound_exported():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    assert re.search(r'#define\s+YV4_F8E4M3\s+3\b', text)
    assert pkg._lib.F8E4M3 == 3
    lib = pkg._lib.lib()
    for name in SYMS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in pkg._lib.SIGNATURES and name in pkg._lib.FEATURES['fp8'].symbols
        assert getattr(lib, name).argtypes == pkg._lib.SIGNATURES[name][1]
    assert pkg._lib.has('fp8')
    assert pkg._lib.ABI_VERSION == 8 and lib.yv4_abi_version() == 8


def _desc(Cin=32, Cout=64, k=3, stride=1):
    d = pkg._lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout = 2, 8, 8, Cin, Cout
    d.KH = d.KW = k
    d.stride, d.pad = stride, k // 2
    d.Ho = d.Wo = (8 + 2 * (k // 2) - k) // stride + 1
    d.x_cstride, d.y_cstride = Cin, Cout
    return d


def test_fp8_argument_validation_without_gpu():
    lib = pkg._lib.lib()
    d = _desc()
    assert lib.yv4_conv_bn_act_fwd_f8(ctypes.byref(d), 3, None, None, None, None, None, None, None, 1.0, 1.0, None,
                                      None) == -1
    assert b'null' in lib.yv4_last_error()
    fake = ctypes.c_void_p(4096)           # never dereferenced: validation returns first
    d = _desc(Cin=24)
    rc = lib.yv4_conv_bn_act_fwd_f8(ctypes.byref(d), 3, fake, fake, fake, fake, None, None, None, 1.0, 1.0, fake, None)
    assert rc == -2
    assert b'Cin = 24' in lib.yv4_last_error()
    d = _desc()
    d.x_cstride, d.x_coff = 48, 8          # an 8-channel offset: not a 16-byte chunk of codes
    assert lib.yv4_conv_bn_act_fwd_f8(ctypes.byref(d), 3, fake, fake, fake, fake, None, None, None, 1.0, 1.0, fake,
                                      None) == -2
    assert lib.yv4_conv_bn_act_fwd_f8(ctypes.byref(_desc()), 2, fake, fake, fake, fake, None, None, None, 1.0, 1.0, fake,
                                      None) == -1                     # bf16 is no output type of the fp8 conv
    assert lib.yv4_quantize_f8(None, 2, 1, 1, 1, 16, 16, 0, None, 16, 0, 1.0, None) == -1
    assert lib.yv4_quantize_f8(fake, 2, 1, 1, 1, 6, 6, 0, fake, 6, 0, 1.0, None) == -2
    assert lib.yv4_spp_pool_fwd_f8(None, 1, 4, 4, 16, 64, 0, None) == -1
    assert lib.yv4_spp_pool_fwd_f8(fake, 1, 4, 4, 16, 48, 0, None) == -1      # 4C channels do not fit the stride
    assert lib.yv4_conv_f8_pick_tile(ctypes.byref(_desc())) in (1, 2, 3)


def test_weight_quantization_per_output_channel():
    torch.manual_seed(0)
    w = torch.randn(40, 32, 3, 3) * torch.rand(40, 1, 1, 1)
    w[3] = 0.0
    wp, cp = P.pack_conv_weight(w, align=16)
    assert cp == 32 and wp.shape == (40, 288)
    codes, sw = P.quantize_weight_f8(wp)
    assert codes.dtype == F8 and codes.shape == wp.shape
    amax = wp.abs().amax(1)
    exp_sw = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.equal(sw, exp_sw) and sw[3] == 1.0
    exp = (wp * (1.0 / exp_sw)[:, None]).clamp(-448, 448).to(F8)
    assert torch.equal(codes.view(torch.uint8), exp.view(torch.uint8))
    # every row's largest magnitude lands on 448 (0x7E), the dequantized weight is within half a code step
    nz = amax > 0
    assert torch.equal(codes.float().abs().amax(1)[nz], torch.full((int(nz.sum()),), 448.0))
    deq = codes.float() * sw[:, None]
    assert bool(((deq - wp).abs() <= wp.abs() / 16 + sw[:, None] * 2.0 ** -10).all())


def test_s1_fold_formula():
    torch.manual_seed(1)
    s1 = torch.rand(64) + 0.5
    sw = torch.rand(64) / 448
    sx = 0.0123456
    got = P.fold_s1_f8(s1, sw, sx)
    exp = torch.tensor([float(float(a) * float(b) * sx) for a, b in zip(s1.double(), sw.double())], dtype=torch.float64).float()
    assert got.dtype == torch.float32 and torch.equal(got, exp)
    assert P.f8_scale(0.0) == 1.0 and P.f8_scale(448.0) == 1.0
    assert P.f8_inv(P.f8_scale(10.0)) == float(torch.tensor(1.0) / (torch.tensor(10.0) / 448.0))


def test_scale_groups_resample_edges_and_concat_buffers():
    """A concat buffer has one scale for all its producers; a resample's source joins its destination's group; the
    group's scale is max amax / 448 over its members."""
    pl = P.Plan('cpu', F8)
    x = pl.new_buf(1, 8, 8, 32, 'x')
    a = pl.conv(x, torch.randn(32, 32, 1, 1), torch.ones(32), torch.zeros(32), name='a')
    b = pl.conv(x, torch.randn(32, 32, 3, 3), torch.ones(32), torch.zeros(32), stride=2, name='b')
    cat = pl.new_buf(1, 8, 8, 64, 'cat')
    pl.conv(a, torch.randn(32, 32, 1, 1), torch.ones(32), torch.zeros(32), out=cat.slice(0, 32), name='c')
    pl.resample(b, cat.slice(32, 32), name='up')
    other = pl.conv(cat, torch.randn(16, 64, 1, 1), torch.ones(16), torch.zeros(16), name='d')
    keys = [bf.key for bf in pl.bufs]
    assert keys == ['0:x', '1:a', '2:b', '3:cat', '4:d']
    g = P.Plan.scale_group
    assert g(b.buf) is g(cat.buf)
    assert g(a.buf) is a.buf and g(x.buf) is x.buf and g(other.buf) is other.buf
    pl.fp8_amax = {'0:x': 1.0, '1:a': 2.0, '2:b': 896.0, '3:cat': 4.0, '4:d': 0.0}
    assert pl.buf_scale(cat.buf) == pl.buf_scale(b.buf) == 2.0
    assert pl.buf_scale(a.buf) == float(torch.tensor(2.0) / 448.0)
    assert pl.buf_scale(other.buf) == 1.0
    pl.finalize()
    ops = {o.name: o for o in pl.ops}
    Lc = ops['c'].info['launch']
    assert Lc['y_inv'] == P.f8_inv(2.0) and Lc['sx'] == pl.buf_scale(a.buf)
    assert torch.equal(Lc['s1f'].cpu(), P.fold_s1_f8(Lc['s1'], Lc['sw'], Lc['sx']))


def test_fp8_plan_stem_stays_16bit_and_quantizes_once():
    """The 3x3 stem and the stride-2 conv after it run on the bf16 kernels (fused into one launch), one quantize op
    converts the 16-bit buffer the first fp8 conv reads, and every other conv is fp8."""
    det = tiny_detector()
    p16 = det.build_plan(2, 64, 96, 'cpu', True, torch.bfloat16)
    det.fp8_amax = {b.key: 1.0 for b in p16.bufs}
    p8 = det.build_plan(2, 64, 96, 'cpu', True, F8)
    convs = [o for o in p8.ops if o.kind == 'conv']
    assert [o.info.get('fused') for o in convs if not o.info.get('f8')] == ['stem_down']
    assert [o.kind for o in p8.ops].count('quantize') == 1
    q = next(o for o in p8.ops if o.kind == 'quantize')
    assert q.info['launch']['src'].dtype == torch.bfloat16 and q.info['launch']['dst'].dtype == F8
    assert all(o.info['launch']['x'].dtype == F8 for o in convs if o.info.get('f8'))
    assert [v.buf.dtype for v in p8.pred_views] == [torch.float32] * 3
    # one calibration serves any geometry: the same keys at another size
    p8b = det.build_plan(1, 96, 64, 'cpu', True, F8)
    assert [b.key for b in p8b.bufs] == [b.key for b in p8.bufs]


def test_fp8_plan_dtype_accepted_and_compile_needs_calibration():
    P.Plan('cpu', F8)                       # no ValueError
    with pytest.raises(ValueError):
        P.Plan('cpu', torch.float8_e5m2)
    det = tiny_detector()
    with pytest.raises(RuntimeError, match='calibrate_fp8'):
        det.compile(2, 64, 96, device='cpu', dtype=F8)
