"""Exact tests of the training convolutions' gradients on integer-valued operands (tests/_exact_ref.py).

Every operand is a small integer, every partial sum stays below 2**24 (asserted per case), so every route -- whatever
its split of the reduction, its chunk order or its atomics -- must equal the float64 reference bit for bit; a 16-bit
result is rounded once, exactly as ``ref64.to(dtype)``.  Covered:
  a. the weight gradient through the C ABI, one case per route and dtype (WGRAD_CASES), in the deterministic form
     (several chunks, a ragged last chunk, run-to-run bits), the atomic form, single-chunk shapes without a workspace,
     and the YV4_WGRAD_WIDEN=1 / YV4_WGRAD_ATOMIC=1 fallbacks in a child process each;
  b. the data gradient through ``train_ops.conv2d(...).backward`` on every route of ``ConvFunction.backward``;
  c. the YOLOv4-L layer table (tools/conv_bench.py SHAPES at 608) in bf16 at the training batch and in fp16 / fp32 at
     batch 8, and the forward of every wide 3x3 tile id at 128 -> 128 @76 and 256 -> 256 @38, batch 32;
  d. the BatchNorm finalize over any replica count (bn_finalize_kernel), and its deterministic form.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib as L
from mmdet_yolov4_amd import train_ops as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CODE = {F32: L.F32, F16: L.F16, BF16: L.BF16}
DTYPES = [F32, BF16, F16]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module', autouse=True)
def _refs_checked():
    X.check_refs_cpu()


# ---------------------------------------------------------------------------------------------------------------------
# a. weight gradient through the ABI
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_route(dtype, N, H, W, Cin, Cout, K, s, p, x_cs, x_co):
    """The route wgrad_impl (conv_wgrad.hip) picks in the default build, from wgrad_fc_cin, wgrad3x3_applies and the v2
    conditions (maps far below 3 GB)."""
    Ho, Wo = X.out_size(H, K, s, p), X.out_size(W, K, s, p)
    M = N * Ho * Wo
    if dtype == F32:
        return 'fp32'
    if K == 3 and s == 1 and p == 1 and Cout in (32, 64) and 256 * 64 * 8 <= M < 2 ** 30:
        if Cin in (16, 32, 64):
            return 'fc_v2'
        if Cin == 8 and x_co + 16 <= x_cs:
            return 'fc_v2 stem'
    if K == 3 and s == 1 and p == 1 and Cin % 128 == 0 and M < 2 ** 30:
        return 'w3x3_v2'
    if K == 1 and s == 1 and p == 0:
        return 'v2 linear'
    if Cin >= 64:
        return 'v2 windowed'
    return 'generic h16'


# (route, dtypes, N, H, W, Cin, Cout, K, stride, pad): M = N * Ho * Wo is odd on every multi-chunk case, so the last
# chunk (a multiple of 32 or 64 rows) is ragged
_H16 = (BF16, F16)
WGRAD_CASES = [
    ('fc_v2', _H16, 1, 367, 367, 16, 32, 3, 1, 1),
    ('fc_v2', _H16, 1, 367, 367, 16, 64, 3, 1, 1),
    ('fc_v2', _H16, 1, 367, 367, 32, 32, 3, 1, 1),
    ('fc_v2', _H16, 3, 213, 211, 32, 64, 3, 1, 1),
    ('fc_v2', _H16, 1, 367, 367, 64, 32, 3, 1, 1),
    ('fc_v2', _H16, 3, 213, 211, 64, 64, 3, 1, 1),
    ('fc_v2 stem', _H16, 3, 213, 211, 8, 32, 3, 1, 1),
    ('w3x3_v2', _H16, 3, 21, 23, 128, 128, 3, 1, 1),
    ('w3x3_v2', _H16, 5, 19, 19, 256, 64, 3, 1, 1),
    ('v2 linear', _H16, 3, 37, 41, 128, 96, 1, 1, 0),
    ('v2 linear', _H16, 7, 39, 39, 64, 256, 1, 1, 0),
    ('v2 windowed', _H16, 7, 37, 37, 64, 128, 3, 2, 1),
    ('v2 windowed', _H16, 3, 31, 27, 64, 96, 3, 1, 1),
    ('generic h16', _H16, 3, 45, 41, 32, 64, 3, 2, 1),
    ('generic h16', _H16, 5, 33, 31, 48, 40, 3, 1, 1),
    ('fp32', (F32,), 3, 33, 31, 64, 96, 3, 1, 1),
    ('fp32', (F32,), 3, 37, 41, 128, 96, 1, 1, 0),
    ('fp32', (F32,), 3, 45, 41, 32, 64, 3, 2, 1),
]
# one chunk: no workspace is needed or given
WGRAD_SINGLE = [
    ('w3x3_v2', _H16, 1, 19, 19, 128, 128, 3, 1, 1),
    ('v2 linear', _H16, 1, 19, 21, 128, 64, 1, 1, 0),
    ('v2 windowed', _H16, 1, 19, 21, 64, 64, 3, 2, 1),
    ('generic h16', _H16, 1, 11, 13, 32, 64, 3, 1, 1),
    ('fp32', (F32,), 1, 9, 11, 32, 64, 3, 1, 1),
]


def _params(cases):
    return [pytest.param(c[0], dt, c[2:], id=f'{c[0].replace(" ", "_")}-{str(dt)[6:]}-{"x".join(map(str, c[2:7]))}k{c[7]}s{c[8]}')
            for c in cases for dt in c[1]]


class WgradCase:
    """Operands of one weight-gradient case, read through channel views: x channels [x_co, x_co + Cin) of x_cs,
    dY channels [y_co, y_co + Cout) of y_cs, the other channels a value outside the operand set."""

    def __init__(self, dtype, N, H, W, Cin, Cout, K, s, p, seed=0, dev='cuda'):
        al = 4 if dtype == F32 else 8
        self.dtype, self.K, self.s, self.p = dtype, K, s, p
        self.Ho, self.Wo = X.out_size(H, K, s, p), X.out_size(W, K, s, p)
        M = N * self.Ho * self.Wo
        if Cin == 8:                       # the stem: 16 channels read per pixel, the weight's 8 kept
            self.x_co, self.x_cs = al, al + 16
        else:
            self.x_co, self.x_cs = al, Cin + 2 * al
        self.y_co, self.y_cs = 2 * al, Cout + 3 * al
        xv = X.int_operand((N, H, W, Cin), seed + 1, dev, dtype)
        dyv = X.int_operand((N, self.Ho, self.Wo, Cout), seed + 2, dev, dtype)
        self.xbuf = torch.full((N, H, W, self.x_cs), 3, dtype=dtype, device=dev)
        self.xbuf[..., self.x_co:self.x_co + Cin] = xv
        self.ybuf = torch.full((N, self.Ho, self.Wo, self.y_cs), 3, dtype=dtype, device=dev)
        self.ybuf[..., self.y_co:self.y_co + Cout] = dyv
        self.base = 5 * X.int_operand((Cout, K, K, Cin), seed + 3, dev)     # already in dW: accumulate, not overwrite
        X.guard(M, X.amax(xv), X.amax(dyv), extra=X.amax(self.base))
        self.want = self.base.double() + X.wgrad_ref(xv, dyv, K, K, s, p)
        d = L.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, self.Ho, self.Wo, Cout
        d.KH, d.KW, d.stride, d.pad = K, K, s, p
        d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = self.x_cs, self.x_co, self.y_cs, self.y_co
        self.d, self.M = d, M
        self.route = wgrad_route(dtype, N, H, W, Cin, Cout, K, s, p, self.x_cs, self.x_co)

    def run(self, form):
        """form 'det': yv4_conv_wgrad_det with the workspace it asks for; 'atomic': yv4_conv_wgrad[_h16]."""
        lib = L.lib()
        dw = self.base.clone()
        code = CODE[self.dtype]
        if form == 'det':
            need = int(lib.yv4_conv_wgrad_workspace(C.byref(self.d), code))
            ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=dw.device) if need else None
            L.check(lib.yv4_conv_wgrad_det(C.byref(self.d), code, self.xbuf.data_ptr(), self.ybuf.data_ptr(),
                                           dw.data_ptr(), ws.data_ptr() if need else None, need, _stream()),
                    'yv4_conv_wgrad_det')
        elif self.dtype == F32:
            L.check(lib.yv4_conv_wgrad(C.byref(self.d), self.xbuf.data_ptr(), self.ybuf.data_ptr(), dw.data_ptr(),
                                       _stream()), 'yv4_conv_wgrad')
        else:
            L.check(lib.yv4_conv_wgrad_h16(C.byref(self.d), code, self.xbuf.data_ptr(), self.ybuf.data_ptr(),
                                           dw.data_ptr(), _stream()), 'yv4_conv_wgrad_h16')
        torch.cuda.synchronize()
        return dw

    def chunks(self):
        need = int(L.lib().yv4_conv_wgrad_workspace(C.byref(self.d), CODE[self.dtype]))
        return need // (4 * self.want.numel()) if need else 1


@pytest.mark.parametrize('route,dtype,shape', _params(WGRAD_CASES))
def test_wgrad_routes_exact(gpu_device, route, dtype, shape):
    """Several chunks with a ragged last one, channel views on both operands, a non-zero dW already in place: the
    deterministic form twice (same bits) and the atomic form, each equal to base + reference exactly."""
    c = WgradCase(dtype, *shape, dev=gpu_device)
    assert c.route == route, f'the case reaches {c.route}, not {route}'
    assert c.chunks() > 1 and c.M % 2 == 1, (c.chunks(), c.M)
    a = c.run('det')
    X.assert_exact(a, c.want, torch.float32, f'{route} det', X.WGRAD_NAMES)
    assert torch.equal(c.run('det'), a), 'the deterministic form changed between two runs'
    X.assert_exact(c.run('atomic'), c.want, torch.float32, f'{route} atomic', X.WGRAD_NAMES)


@pytest.mark.parametrize('route,dtype,shape', _params(WGRAD_SINGLE))
def test_wgrad_routes_single_chunk_exact(gpu_device, route, dtype, shape):
    c = WgradCase(dtype, *shape, seed=10, dev=gpu_device)
    assert c.route == route and c.chunks() == 1
    X.assert_exact(c.run('det'), c.want, torch.float32, f'{route} single chunk', X.WGRAD_NAMES)
    X.assert_exact(c.run('atomic'), c.want, torch.float32, f'{route} single chunk atomic', X.WGRAD_NAMES)


def child_main(mode):
    """Run in a fresh process (the switches are read once per process): 'widen' runs every 16-bit ABI case, several
    chunks and one, in both forms; 'atomic' a few layers of each dtype through ConvFunction.  One line per case."""
    dev = torch.device('cuda:0')
    if mode == 'widen':
        for cases in (WGRAD_CASES, WGRAD_SINGLE):
            for case in cases:
                for dt in case[1]:
                    if dt == F32:
                        continue
                    c = WgradCase(dt, *case[2:], dev=dev)
                    for form in ('det', 'atomic'):
                        X.assert_exact(c.run(form), c.want, torch.float32, f'widen {case[0]} {dt} {form}', X.WGRAD_NAMES)
                    print('OK', case[0], dt, flush=True)
    else:
        for dt in DTYPES:
            for (N, Cin, Cout, H, W, K, s, p) in [(3, 64, 96, 19, 23, 3, 1, 1), (2, 32, 64, 45, 39, 3, 2, 1),
                                                  (3, 128, 64, 21, 17, 1, 1, 0)]:
                _layer_grads(dev, dt, N, Cin, Cout, H, W, K, s, p, seed=5)
                print('OK', dt, N, Cin, Cout, H, W, K, s, flush=True)
    print('CHILD DONE', flush=True)


@pytest.mark.parametrize('mode,env', [('widen', {'YV4_WGRAD_WIDEN': '1'}), ('atomic', {'YV4_WGRAD_ATOMIC': '1'})])
def test_wgrad_fallbacks_exact_in_child(gpu_device, mode, env):
    """YV4_WGRAD_WIDEN=1 (the widening fp32-MFMA kernel for 16-bit operands) and YV4_WGRAD_ATOMIC=1 (ConvFunction's
    float-atomic weight gradient), one child process at a time."""
    code = (f'import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]; '
            f'import test_gpu_grad_exact as M; M.child_main({mode!r})')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'CHILD DONE' in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# b. data gradient through ConvFunction.backward
# ---------------------------------------------------------------------------------------------------------------------
def dgrad_route(dtype, Cin, Cout, H, W, K, s, p):
    """The route ConvFunction.backward takes (train_ops.py)."""
    h16 = dtype != F32
    if s == 2 and (K, p) == (3, 1) and Cout % (8 if h16 else 32) == 0:
        if T._ROWPAIR_ON and 2 * Cin <= 64 and H % 2 == 0 and W % 2 == 0 and Cin % (4 if h16 else 2) == 0:
            return 'rowpair'
        return 'parity'
    return f'dilated s{s}'


def _layer_grads(dev, dtype, N, Cin, Cout, H, W, K, s, p, seed=0, big=False, sink=False, cat=None, image=False):
    """x -> T.conv2d -> backward(dY) with integer operands; dW and dX (unless ``image``: the stem's input has no
    gradient) compared with the references exactly.  ``sink``: a parked residual gradient R is joined in the data
    gradient's epilogue -- dX = round(ref + R), ONE rounding (the fp32 accumulator plus R).  ``cat`` = (total, off):
    the conv writes a channel slice of a concat buffer and receives the whole buffer's gradient."""
    xc = (16 if dtype != F32 else 4) if image else Cin
    xv = X.int_operand((N, H, W, Cin), seed + 1, dev, dtype, big=big)
    if image:      # the image stored with zeros beyond its channels (image_to_nhwc16); its weight padded to match
        xv = torch.cat([xv, torch.zeros(N, H, W, xc - Cin, dtype=dtype, device=dev)], -1)
    w = X.int_operand((Cout, Cin, K, K), seed + 2, dev)
    Ho, Wo = X.out_size(H, K, s, p), X.out_size(W, K, s, p)
    total, off = cat if cat else (Cout, 0)
    dyv = X.int_operand((N, Ho, Wo, total), seed + 3, dev, dtype, big=big)
    dy = dyv[..., off:off + Cout]
    xr = xv.permute(0, 3, 1, 2).detach().requires_grad_(not image)
    wr = w.clone().requires_grad_(True)
    gs = T.GradSink() if sink else None
    y = T.conv2d(xr, wr, s, p, dtype=dtype, sink=gs, cat=T.CatSlot(total, off) if cat else None)
    R = None
    if sink:
        R = X.int_operand((N, H, W, Cin), seed + 4, dev, dtype) * 3
        gs.value, gs.cs = R.permute(0, 3, 1, 2), None
    y.backward(dyv.permute(0, 3, 1, 2))
    X.guard(N * Ho * Wo, X.amax(xv), X.amax(dy))
    X.assert_exact(wr.grad.permute(0, 2, 3, 1), X.wgrad_ref(xv[..., :Cin], dy, K, K, s, p), torch.float32,
                   f'dW {dtype} {Cin}->{Cout} k{K}s{s} @{H}x{W}', X.WGRAD_NAMES)
    if image:
        return
    X.guard(K * K * Cout, X.amax(w), X.amax(dy), extra=X.amax(R) if sink else 0)
    ref = X.dgrad_ref(dy, w, H, W, s, p, torch.float64 if sink else dtype)
    if sink:
        ref += R.double()
    X.assert_exact(xr.grad.permute(0, 2, 3, 1), ref, dtype,
                   f'dX {dgrad_route(dtype, Cin, Cout, H, W, K, s, p)} {dtype} {Cin}->{Cout} k{K}s{s} @{H}x{W}')


DGRAD_CASES = [
    # (route, N, Cin, Cout, H, W, K, stride, pad)
    ('dilated s1', 3, 64, 96, 19, 23, 3, 1, 1),
    ('dilated s1', 2, 128, 64, 21, 17, 1, 1, 0),
    ('dilated s2', 2, 24, 32, 18, 14, 1, 2, 0),     # even: the dilated grid is the input's
    ('dilated s2', 2, 24, 32, 17, 13, 1, 2, 0),     # odd: one row and column cropped
    ('dilated s2', 2, 16, 32, 19, 17, 3, 2, 0),     # odd, 3x3 without padding
    ('parity', 2, 48, 64, 22, 18, 3, 2, 1),
    ('parity', 2, 48, 64, 21, 17, 3, 2, 1),
    ('rowpair', 2, 16, 64, 22, 18, 3, 2, 1),
    ('rowpair', 2, 32, 64, 24, 20, 3, 2, 1),
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', DGRAD_CASES, ids=lambda c: f'{c[0].replace(" ", "_")}-{c[2]}to{c[3]}k{c[6]}s{c[7]}@{c[4]}x{c[5]}')
def test_dgrad_routes_exact(gpu_device, dtype, case):
    route, shape = case[0], case[1:]
    N, Cin, Cout, H, W, K, s, p = shape
    assert dgrad_route(dtype, Cin, Cout, H, W, K, s, p) == route
    _layer_grads(gpu_device, dtype, *shape, seed=20)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_dgrad_fp32_parity_domain(gpu_device, dtype):
    """Cout 40: fp32 falls back to the dilated form (Cout % 32), the 16-bit paths stay on the parity classes."""
    shape = (2, 48, 40, 22, 18, 3, 2, 1)
    assert dgrad_route(dtype, *shape[1:]) == ('dilated s2' if dtype == F32 else 'parity')
    _layer_grads(gpu_device, dtype, *shape, seed=30)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_dgrad_grad_sink_exact(gpu_device, dtype):
    """The GradSink residual join: stride 1 only (the stride-2 forms drop the sink), always on the dilated route whose
    epilogue adds R to the fp32 accumulator -- one rounding.  (The separate 16-bit ``dx + joined`` add is reached only
    when the sink's tensor is at a stride-2 conv, which ConvFunction never keeps.)"""
    _layer_grads(gpu_device, dtype, 2, 64, 96, 19, 23, 3, 1, 1, seed=40, sink=True)
    _layer_grads(gpu_device, dtype, 2, 64, 128, 15, 13, 1, 1, 0, seed=41, sink=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_dgrad_concat_slice_exact(gpu_device, dtype):
    """dY handed over as a channel slice of a concat buffer's gradient (``cat=``): dW and dX from the slice only."""
    _layer_grads(gpu_device, dtype, 2, 64, 64, 19, 23, 3, 1, 1, seed=50, cat=(192, 64))
    _layer_grads(gpu_device, dtype, 2, 32, 64, 24, 20, 3, 2, 1, seed=51, cat=(128, 64))
    _layer_grads(gpu_device, dtype, 2, 64, 64, 21, 17, 1, 1, 0, seed=52, cat=(96, 0))


# ---------------------------------------------------------------------------------------------------------------------
# c. the YOLOv4-L layer table
# ---------------------------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from conv_bench import SHAPES as YV4L_SHAPES  # noqa: E402


def _table_case(dtype, batch, row):
    cin, cout, k, s, h, _ = row
    p = k // 2
    ho = X.out_size(h, k, s, p)
    N = batch
    big = N * ho * ho * 4 >= X.EXACT_LIMIT     # {-1, 1} on the long reductions
    if N * ho * ho >= X.EXACT_LIMIT:           # even {-1, 1} is not exact: the stem at 608 runs at batch 40
        N = (X.EXACT_LIMIT - 1) // (ho * ho) // 8 * 8
    return N, big


@pytest.mark.parametrize('dtype,batch', [(BF16, 64), (F16, 8), (F32, 8)], ids=['bf16-b64', 'f16-b8', 'f32-b8'])
def test_yolov4l_layer_table_exact(gpu_device, dtype, batch):
    """Every layer shape of YOLOv4-L at 608 through the routes the product picks: dW and dX exact.  The batch is lowered
    only where the 2**24 guard demands it (bf16: the stem, 3 -> 32 at 608, runs at batch 40).  The head's 255 output
    channels are padded to 256 as YOLOCSPHead.fwd_raw pads them; the stem's input is an image without a gradient."""
    for row in YV4L_SHAPES:
        cin, cout, k, s, h, _ = row
        cout = -(-cout // 8) * 8
        N, big = _table_case(dtype, batch, row)
        _layer_grads(gpu_device, dtype, N, cin, cout, h, h, k, s, k // 2, seed=60 + cin + cout, big=big,
                     image=cin == 3)
        torch.cuda.empty_cache()


W3_TILES = [5, 13, 21, 29, 37, 45, 53, 61]      # test_gpu_h16.py: YV4_HTILE_W3x3 and its pinned shapes
W3F_TILES = [10, 26, 42, 58, 74, 90]            # test_gpu_parity.py: YV4_TILE_W3x3 and its pinned shapes


@pytest.mark.parametrize('shape', [(32, 76, 128, 128), (32, 38, 256, 256)], ids=['128to128@76', '256to256@38'])
def test_wide3x3_forward_exact_every_tile(gpu_device, shape):
    """The wide 3x3 kernels at full occupancy on real layer shapes: their zero padding comes from out-of-range LDS reads
    returning zero, so a border row or column that picked up anything shows here as an inexact output."""
    N, H, Cin, Cout = shape
    dev = gpu_device
    lib = L.lib()
    for dtype, tiles in ((BF16, W3_TILES), (F16, W3_TILES), (F32, W3F_TILES)):
        x = X.int_operand((N, H, H, Cin), 71, dev, dtype)
        w = X.int_operand((Cout, Cin, 3, 3), 72, dev)
        X.guard(9 * Cin, X.amax(x), X.amax(w))
        ref = X.fwd_ref(x, w, 1, 1, dtype)
        wp = w.permute(0, 2, 3, 1).contiguous().to(dtype)
        ones, zeros = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
        for tile in tiles:
            y = torch.full((N, H, H, Cout), 7, dtype=dtype, device=dev)
            d = L.ConvDesc()
            d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, H, Cin, H, H, Cout
            d.KH = d.KW = 3
            d.stride, d.pad = 1, 1
            d.x_cstride, d.y_cstride, d.r_cstride = Cin, Cout, Cout
            d.tile = tile
            if dtype == F32:
                rc = lib.yv4_conv_bn_act_fwd(C.byref(d), x.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(),
                                             None, None, None, y.data_ptr(), _stream())
            else:
                rc = lib.yv4_conv_bn_act_fwd_h16(C.byref(d), CODE[dtype], CODE[dtype], x.data_ptr(), wp.data_ptr(),
                                                 ones.data_ptr(), zeros.data_ptr(), None, None, None, y.data_ptr(),
                                                 _stream())
            L.check(rc, f'wide 3x3 forward tile {tile}')
            torch.cuda.synchronize()
            X.assert_exact(y, ref, dtype, f'forward {dtype} tile {tile} {Cin}->{Cout} @{H}')


# ---------------------------------------------------------------------------------------------------------------------
# d. BatchNorm finalize
# ---------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    ai = a.float().contiguous().view(torch.int32).long()
    bi = b.float().contiguous().view(torch.int32).long()
    return int((ai - bi).abs().max().item()) if a.numel() else 0


@pytest.mark.parametrize('C_', [1, 31, 33, 255])
@pytest.mark.parametrize('replicas', [1, 2, 7, 63, 64, 65, 100, 200])
def test_bn_finalize_any_replica_count(gpu_device, replicas, C_):
    """yv4_bn_finalize adds up ``replicas`` blocks of [sum (C) | sum of squares (C)] -- any count (SyncBN-style callers
    pass their own) -- and, with clear_work, leaves every one of them zero.  Integer-valued sums: the totals are exact,
    so mean is bit-exact and invstd / the running statistics are within one fp32 ulp of float64."""
    dev = gpu_device
    lib = L.lib()
    g = torch.Generator(device=dev).manual_seed(replicas * 1000 + C_)
    M = 4096 + replicas
    s1 = torch.randint(-300, 300, (replicas, C_), generator=g, device=dev).double()
    s2 = torch.randint(20000, 40000, (replicas, C_), generator=g, device=dev).double()
    eps, mom = 1e-3, 0.03
    S1, S2 = s1.sum(0), s2.sum(0)
    m = S1 / M
    var = (S2 / M - m * m).clamp_min(0)
    mom64 = float(torch.tensor(mom, dtype=torch.float32))
    eps64 = float(torch.tensor(eps, dtype=torch.float32))
    rm0 = torch.randn(C_, generator=g, device=dev)
    rv0 = torch.rand(C_, generator=g, device=dev) + 0.5
    for use_rows in (False, True):
        work = torch.empty(replicas + 1, 2, C_, dtype=torch.float64, device=dev)
        work[:replicas, 0], work[:replicas, 1] = s1, s2
        work[replicas] = 5.0                                      # a block past the last replica: neither read nor cleared
        zero_after = torch.full((4 * C_ + 1,), 9.0, dtype=torch.float64, device=dev)
        mean = torch.empty(C_, device=dev)
        invstd = torch.empty(C_, device=dev)
        rm, rv = rm0.clone(), rv0.clone()
        rows = torch.tensor([float(M)], dtype=torch.float64, device=dev)
        L.check(lib.yv4_bn_finalize(work.data_ptr(), replicas, 1 if use_rows else M, rows.data_ptr() if use_rows else None,
                                    C_, eps, mom, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1,
                                    zero_after.data_ptr(), _stream()), 'yv4_bn_finalize')
        torch.cuda.synchronize()
        tag = f'replicas {replicas} C {C_} rows_dev {use_rows}'
        assert torch.equal(mean, m.float()), tag
        assert _ulps(invstd, (1.0 / torch.sqrt(var + eps64)).float()) <= 1, tag
        assert _ulps(rm, ((1.0 - mom64) * rm0.double() + mom64 * m).float()) <= 1, tag
        assert _ulps(rv, ((1.0 - mom64) * rv0.double() + mom64 * var * M / (M - 1)).float()) <= 1, tag
        assert not bool(work[:replicas].any()), f'{tag}: {int((work[:replicas] != 0).sum())} words not cleared'
        assert bool((work[replicas] == 5.0).all()), tag
        assert not bool(zero_after[:4 * C_].any()) and float(zero_after[4 * C_]) == 9.0, tag


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_bn_finalize_deterministic_matches_default(gpu_device, dtype):
    """The statistics a conv epilogue leaves (yv4_conv_fwd_stats, 64 replicas): the fixed-point words of deterministic
    mode and the doubles of the default mode give the same mean / invstd / running statistics bit for bit on integer
    data, and both leave the buffer clean."""
    dev = gpu_device
    lib = L.lib()
    N, H, W, Cin, Cout = 4, 37, 29, 64, 96
    x = X.int_operand((N, H, W, Cin), 81, dev, dtype)
    w = X.int_operand((Cout, 3, 3, Cin), 82, dev, dtype)
    ones, zeros = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, H, W, Cout
    d.KH = d.KW = 3
    d.stride, d.pad = 1, 1
    d.x_cstride, d.y_cstride, d.r_cstride = Cin, Cout, Cout
    outs = []
    was = lib.yv4_get_deterministic()
    try:
        for det in (0, 1):
            lib.yv4_set_deterministic(det)
            y = torch.empty(N, H, W, Cout, dtype=dtype, device=dev)
            stats = torch.zeros(L.STATS_REPLICAS * 2 * Cout, dtype=torch.float64, device=dev)
            L.check(lib.yv4_conv_fwd_stats(C.byref(d), CODE[dtype], x.data_ptr(), w.data_ptr(), ones.data_ptr(),
                                           zeros.data_ptr(), y.data_ptr(), stats.data_ptr(), 1, _stream()),
                    'yv4_conv_fwd_stats')
            mean, invstd = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
            rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
            L.check(lib.yv4_bn_finalize(stats.data_ptr(), L.STATS_REPLICAS, N * H * W, None, Cout, 1e-3, 0.03,
                                        mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1, None,
                                        _stream()), 'yv4_bn_finalize')
            torch.cuda.synchronize()
            assert not bool(stats.any()), f'deterministic {det}: statistics buffer not cleared'
            if dtype == F32:     # (y itself is exact: the statistics of the stored values)
                yd = y.double().reshape(-1, Cout)
                assert torch.equal(mean, (yd.sum(0) / (N * H * W)).float()), f'deterministic {det}: mean'
            outs.append((mean, invstd, rm, rv))
    finally:
        lib.yv4_set_deterministic(was)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
