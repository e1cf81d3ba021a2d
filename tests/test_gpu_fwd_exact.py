"""Exact tests of the forward convolutions on integer-valued operands (tests/_exact_ref.py), through the C ABI.

Every operand is a small integer, every partial sum and every step of the fused epilogue
``y = act2((act1(conv * s1 + t1) + residual) * s2 + t2)`` stays exactly representable in fp32 (asserted per case:
``Epilogue.guard``), so every route -- whatever its tile, its split of K or its summation order -- must equal the float64
reference bit for bit; a 16-bit result is rounded once, exactly as ``ref64.to(dtype)``.  One dropped, duplicated or
misplaced product, slab or residual changes the result.  Every call reads x through a channel-offset view of a wider
buffer, writes y into a channel-offset view of a buffer pre-filled with a sentinel (asserted untouched outside the view)
and reads the residual through a view of its own.  Covered:
  a. the fp32 split-K path (yv4_conv_bn_act_fwd_splitk): the reported split, float64 equality, equality with the unsplit
     64 x 64 LDS-DMA tile, repeatability, a NaN-filled workspace of exactly the reported size with a guard region behind
     it, the shapes that do not split, the refusals, and float operands at the unsplit tiles' 1e-4 bound;
  b. the 16-bit split-K path over SPLITK_SHAPES of test_gpu_h16.py, the same way, at fp32 and at 16-bit output;
  c. every forward route by tile id, fp32 and 16-bit, on the shape lists of the tolerance tests (imported, so the files
     cannot drift), bare and with the full exact epilogue, and the fused stem + stride-2 launch.
"""
import ctypes as C
import os
import sys
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from mmdet_yolov4_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ref as X  # noqa: E402
import test_gpu_h16 as H  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_gpu_stem_down as SD  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CODE = {F32: L.F32, F16: L.F16, BF16: L.BF16}
H16 = [BF16, F16]
NAME = {F32: 'f32', BF16: 'bf16', F16: 'f16'}
SENTINEL = 7.0          # y outside the view, and the guard region behind a workspace
OUTSIDE = 3.0           # x and residual channels outside their views: a value outside the operand set


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module', autouse=True)
def _refs_checked():
    X.check_refs_cpu()
    X.check_epilogue_ref_cpu()


# ---------------------------------------------------------------------------------------------------------------------
# operands, epilogues and one launch
# ---------------------------------------------------------------------------------------------------------------------
def _needs_big(terms):
    """{-2 .. 2} operands through the largest epilogue would leave the exact range: fall back to {-1, 1}."""
    return (((terms * 4) * 2 + 3 + 2) * 2 + 3) * 4 >= X.EXACT_LIMIT


class Ops:
    """The integer operands of one convolution shape and its float64 convolution, shared by every dtype (the values do not
    depend on it), route and epilogue that the shape is run with.  Immutable once built."""

    def __init__(self, dev, shape):
        N, Hh, W, Cin, Cout, K, s, p = shape
        self.shape, self.dev = shape, dev
        self.Ho, self.Wo = X.out_size(Hh, K, s, p), X.out_size(W, K, s, p)
        self.terms = K * K * Cin
        big = _needs_big(self.terms)
        self.x = X.int_operand((N, Hh, W, Cin), 1, dev, big=big)
        self.w = X.int_operand((Cout, Cin, K, K), 2, dev, big=big)
        self.res = X.int_operand((N, self.Ho, self.Wo, Cout), 3, dev)
        self.ax, self.aw, self.ar = X.amax(self.x), X.amax(self.w), X.amax(self.res)
        X.guard(self.terms, self.ax, self.aw)
        self.conv64 = X.fwd_ref(self.x, self.w, s, p)
        self._packed = {}

    def weights(self, dtype):
        """(Cout, KH, KW, Cin), as the kernels read them."""
        if dtype not in self._packed:
            self._packed[dtype] = self.w.permute(0, 2, 3, 1).contiguous().to(dtype)
        return self._packed[dtype]

    def want(self, ep, residual):
        ep.guard(self.terms, self.ax, self.aw, res_max=self.ar if residual else 0)
        return X.epilogue_ref(self.conv64, ep, self.res if residual else None)


_OPS = OrderedDict()


def ops_for(dev, shape):
    """One reference per shape, kept for the neighbouring tests that run the same shape (the last three shapes)."""
    key = (str(dev), tuple(shape))
    if key in _OPS:
        _OPS.move_to_end(key)
        return _OPS[key]
    while len(_OPS) >= 3:
        _OPS.popitem(last=False)
    _OPS[key] = Ops(dev, shape)
    return _OPS[key]


def laid_out(shape, dtype):
    """The 3-channel image layers are stored with 4 (fp32) or 8 (16-bit) channels: the exact cases give every stored
    channel a non-zero operand, so the layer is a Cin = 4 / 8 convolution."""
    al = 4 if dtype == F32 else 8
    s = list(shape)
    s[3] = -(-s[3] // al) * al
    return tuple(s)


def epilogues(Cout, dev):
    """name -> (Epilogue, residual): 'bare' is the convolution alone (s1 = 1, t1 = 0); 'full' every stage with the
    slope-0.5 leaky activations; 'nores' the same without the residual (routes that take none); 'one' the first stage
    only (the stem)."""
    return {
        'bare': (X.Epilogue(Cout, 5, dev, affine1=False), False),
        'full': (X.Epilogue(Cout, 5, dev, True, X.ACT_LEAKY, True, X.ACT_LEAKY), True),
        'nores': (X.Epilogue(Cout, 5, dev, True, X.ACT_LEAKY, True, X.ACT_LEAKY), False),
        'one': (X.Epilogue(Cout, 5, dev, True, X.ACT_LEAKY), False),
    }


class Launch:
    """Buffers and descriptor of one call.  ``views``: x channels [al, al + Cin) of Cin + 2 al, y channels
    [2 ao, 2 ao + Cout) of Cout + 3 ao (rounded up to 8 for a 16-bit output), residual channels [al, al + Cout) of
    Cout + 3 al, with al / ao the vector width of the operand / output type (4 fp32, 8 16-bit).  Cout 255 gives odd
    fp32 pixel strides: the scalar store path."""

    def __init__(self, ops, dtype, odt, ep, residual, views=True, tile=0):
        N, Hh, W, Cin, Cout, K, s, p = ops.shape
        dev = ops.dev
        al, ao = (4 if dtype == F32 else 8), (4 if odt == F32 else 8)
        self.ops, self.dtype, self.odt, self.ep = ops, dtype, odt, ep
        self.x_co, self.x_cs = (al, Cin + 2 * al) if views else (0, Cin)
        self.y_co, self.y_cs = (2 * ao, Cout + 3 * ao) if views else (0, Cout)
        if odt != F32:
            self.y_cs = -(-self.y_cs // 8) * 8
        self.r_co, self.r_cs = (al, Cout + 3 * al) if views else (0, Cout)
        self.xbuf = torch.full((N, Hh, W, self.x_cs), OUTSIDE, dtype=dtype, device=dev)
        self.xbuf[..., self.x_co:self.x_co + Cin] = ops.x
        self.ybuf = torch.full((N, ops.Ho, ops.Wo, self.y_cs), SENTINEL, dtype=odt, device=dev)
        self.rbuf = None
        if residual:
            self.rbuf = torch.full((N, ops.Ho, ops.Wo, self.r_cs), OUTSIDE, dtype=dtype, device=dev)
            self.rbuf[..., self.r_co:self.r_co + Cout] = ops.res
        self.w = ops.weights(dtype)
        d = L.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, Hh, W, Cin, ops.Ho, ops.Wo, Cout
        d.KH, d.KW, d.stride, d.pad = K, K, s, p
        d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = self.x_cs, self.x_co, self.y_cs, self.y_co
        d.r_cstride, d.r_coff = self.r_cs, self.r_co
        d.act1, d.act2, d.slope1, d.slope2 = ep.act1, ep.act2, ep.slope, getattr(ep, 'slope2', ep.slope)
        d.tile = tile
        self.d = d

    def _tail(self):
        ep = self.ep
        two = ep.two_stage
        return (ep.s1.data_ptr(), ep.t1.data_ptr(), ep.s2.data_ptr() if two else None, ep.t2.data_ptr() if two else None,
                self.rbuf.data_ptr() if self.rbuf is not None else None, self.ybuf.data_ptr())

    def call(self, ws_ptr=None, ws_bytes=None):
        """The status of the plain entry (``ws_bytes`` None) or of the split-K entry of the operand type."""
        lib = L.lib()
        self.ybuf.fill_(SENTINEL)
        head = (C.byref(self.d),) if self.dtype == F32 else (C.byref(self.d), CODE[self.dtype], CODE[self.odt])
        args = head + (self.xbuf.data_ptr(), self.w.data_ptr()) + self._tail()
        if ws_bytes is None:
            fn = lib.yv4_conv_bn_act_fwd if self.dtype == F32 else lib.yv4_conv_bn_act_fwd_h16
            rc = fn(*args, _stream())
        else:
            fn = lib.yv4_conv_bn_act_fwd_splitk if self.dtype == F32 else lib.yv4_conv_bn_act_fwd_h16_splitk
            rc = fn(*args, ws_ptr, ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc

    def splitk_workspace(self):
        ks = C.c_int(-1)
        fn = L.lib().yv4_conv_splitk_workspace if self.dtype == F32 else L.lib().yv4_conv_h16_splitk_workspace
        return int(fn(C.byref(self.d), C.byref(ks))), ks.value

    def view(self):
        """y's view, after asserting that nothing outside it was written."""
        Cout = self.ops.shape[4]
        out = self.ybuf[..., :self.y_co], self.ybuf[..., self.y_co + Cout:]
        assert all(bool((o == SENTINEL).all()) for o in out), 'channels outside the output view were written'
        return self.ybuf[..., self.y_co:self.y_co + Cout]

    def untouched(self):
        return bool((self.ybuf == SENTINEL).all())


def run_exact(ops, dtype, odt, ep_name, tile, what, views=True):
    """One plain-entry call that must succeed and equal float64 (rounded once to ``odt``); returns y's view."""
    ep, residual = epilogues(ops.shape[4], ops.dev)[ep_name]
    la = Launch(ops, dtype, odt, ep, residual, views, tile)
    L.check(la.call(), what)
    y = la.view().clone()
    X.assert_exact(y, ops.want(ep, residual), odt, f'{what} [{ep_name}]')
    return y


def assert_refused(ops, dtype, odt, ep_name, tile, what):
    """A case outside a route's domain: an error status, and not one element of y written."""
    ep, residual = epilogues(ops.shape[4], ops.dev)[ep_name]
    la = Launch(ops, dtype, odt, ep, residual, True, tile)
    assert la.call() != 0, f'{what} [{ep_name}]: accepted'
    assert la.untouched(), f'{what} [{ep_name}]: refused, but y was written'


# ---------------------------------------------------------------------------------------------------------------------
# a / b. split-K
# ---------------------------------------------------------------------------------------------------------------------
def split_of(nk, ways):
    """(slices per split, splits, slices of the last split) of ``nk`` K slices split ``ways`` ways with no empty split."""
    per = -(-nk // ways)
    splits = -(-nk // per)
    return per, splits, nk - (splits - 1) * per


# (shape, K slices of 32, ways reported, splits, slices per split, slices of the last split, property)
SPLITK_F32 = [
    ((1, 8, 8, 64, 64, 3, 1, 1), 18, 2, 2, 9, 9, 'smallest split, one tile'),
    ((1, 7, 9, 96, 72, 3, 1, 1), 27, 2, 2, 14, 13, 'ragged last split, ragged M (63 rows), Cout tail in the second column tile'),
    ((1, 5, 5, 4128, 64, 1, 1, 0), 129, 16, 15, 9, 3, 'fewer splits than ways: workspace sized for 16, finish adds 15'),
    ((1, 19, 19, 1024, 255, 1, 1, 0), 32, 4, 4, 8, 8, 'head: slab pitch 256 over Cout 255, odd y pitch, scalar tail'),
    ((1, 38, 38, 128, 256, 3, 2, 1), 36, 4, 4, 9, 9, 'stride 2'),
    ((1, 19, 19, 512, 512, 3, 1, 1), 144, 16, 16, 9, 9, 'the deepest real layer'),
]
# (K slices of 64, ways reported, splits, slices per split, last) per entry of test_gpu_h16.py's SPLITK_SHAPES
SPLITK_H16 = [(72, 16, 15, 5, 2), (16, 4, 4, 4, 4), (36, 8, 8, 5, 1), (18, 4, 4, 5, 3), (16, 4, 4, 4, 4), (27, 4, 4, 7, 6),
              (18, 4, 4, 5, 3)]
GUARD_FLOATS = 4096


def _ids(shapes):
    return ['x'.join(map(str, s[:5])) + f'k{s[5]}s{s[6]}' for s in shapes]


class Workspace:
    """Exactly the reported bytes, NaN-filled, with a guard region of the sentinel directly behind them."""

    def __init__(self, dev, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.empty(self.n + GUARD_FLOATS, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.nbytes = nbytes
        self.reset()

    def reset(self):
        self.buf[:self.n] = float('nan')
        self.buf[self.n:] = SENTINEL

    def ptr(self):
        return self.buf.data_ptr()

    def guard_intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def _splitk_exact(dev, dtype, odt, shape, nk, ways, splits, per, last, variants):
    """The split-K entry on one shape: the reported split, then per variant (epilogue name, views) float64 equality,
    equality with the unsplit 64 x 64 tile of the same call, repeatability and the workspace's bounds."""
    ops = ops_for(dev, shape)
    N, Hh, W, Cin, Cout, K, s, p = shape
    M = N * ops.Ho * ops.Wo
    kbk = 32 if dtype == F32 else 64
    pad = 4 if dtype == F32 else 8
    unsplit_tile = L.TILE_DMA_64x64 if dtype == F32 else H.HT['t64x64']
    assert nk == K * K * Cin // kbk and split_of(nk, ways) == (per, splits, last)
    for ep_name, views in variants:
        ep, residual = epilogues(Cout, dev)[ep_name]
        la = Launch(ops, dtype, odt, ep, residual, views)
        nbytes, ks = la.splitk_workspace()
        ws_cs = -(-Cout // pad) * pad
        assert ks == ways and ks > 1, f'reported ksplit {ks}, expected {ways}'
        assert nbytes == ways * M * ws_cs * 4, (nbytes, ways, M, ws_cs)
        ws = Workspace(dev, nbytes)
        what = f'splitk {NAME[dtype]}->{NAME[odt]} {shape} [{ep_name}, views {views}]'
        L.check(la.call(ws.ptr(), ws.nbytes), what)
        y = la.view().clone()
        X.assert_exact(y, ops.want(ep, residual), odt, what)
        assert ws.guard_intact(), f'{what}: wrote behind the reported workspace'
        slabs = ws.buf[:ws.n].view(ways, M, ws_cs)
        assert not bool(slabs[:splits, :, :Cout].isnan().any()), f'{what}: a partial of a used slab was never written'
        assert bool(slabs[splits:].isnan().all()), f'{what}: a slab beyond the {splits} splits was written'
        ws.reset()
        L.check(la.call(ws.ptr(), ws.nbytes), what)
        assert torch.equal(la.view(), y), f'{what}: a second run gave other bits'
        la.d.tile = unsplit_tile
        L.check(la.call(), what + ' unsplit')
        assert torch.equal(la.view(), y), f'{what}: differs from the unsplit 64x64 tile'


F32_VARIANTS = [('bare', False), ('full', False), ('bare', True), ('full', True)]


@pytest.mark.parametrize('row', SPLITK_F32, ids=_ids([r[0] for r in SPLITK_F32]))
def test_splitk_f32_exact(gpu_device, row):
    shape, nk, ways, splits, per, last, _ = row
    _splitk_exact(gpu_device, F32, F32, shape, nk, ways, splits, per, last, F32_VARIANTS)


NOT_SPLIT_F32 = [
    (8, 38, 38, 256, 256, 3, 1, 1),     # enough tiles already
    (1, 12, 12, 24, 40, 3, 1, 1),       # Cin % 32 != 0: outside the LDS-DMA tiles
    (1, 8, 8, 64, 64, 1, 1, 0),         # two K slices: too few to split
]


@pytest.mark.parametrize('shape', NOT_SPLIT_F32, ids=_ids(NOT_SPLIT_F32))
def test_splitk_f32_forwards_when_not_split(gpu_device, shape):
    """ksplit 1, no workspace: the call (given none) is yv4_conv_bn_act_fwd, bit for bit, and exact."""
    ops = ops_for(gpu_device, shape)
    for ep_name in ('bare', 'full'):
        ep, residual = epilogues(shape[4], gpu_device)[ep_name]
        la = Launch(ops, F32, F32, ep, residual)
        assert la.splitk_workspace() == (0, 1)
        L.check(la.call(None, 0), f'splitk (not split) {shape}')
        y = la.view().clone()
        X.assert_exact(y, ops.want(ep, residual), F32, f'splitk (not split) {shape} [{ep_name}]')
        L.check(la.call(), f'plain {shape}')
        assert torch.equal(la.view(), y)


@pytest.mark.parametrize('dtype', [F32] + H16, ids=['f32', 'bf16', 'f16'])
def test_splitk_refuses_a_bad_workspace(gpu_device, dtype):
    """One byte too few, a pointer that is not 16-byte aligned and no workspace at all on a splitting shape: an error
    each, y keeps its sentinel; the same workspace given whole is accepted."""
    shape = SPLITK_F32[0][0] if dtype == F32 else (1, 11, 13, 192, 72, 3, 1, 1)
    ops = ops_for(gpu_device, shape)
    ep, residual = epilogues(shape[4], gpu_device)['full']
    la = Launch(ops, dtype, dtype, ep, residual)
    nbytes, ks = la.splitk_workspace()
    assert ks > 1 and nbytes > 0
    ws = Workspace(gpu_device, nbytes)
    for ptr, size, why in [(ws.ptr(), nbytes - 1, 'one byte too small'), (ws.ptr() + 4, nbytes, 'misaligned'),
                           (None, nbytes, 'null')]:
        assert la.call(ptr, size) != 0, f'{why}: accepted'
        assert la.untouched(), f'{why}: refused, but y was written'
        assert bool(ws.buf[:ws.n].isnan().all()) and ws.guard_intact(), f'{why}: refused, but the workspace was written'
    L.check(la.call(ws.ptr(), nbytes), 'splitk, whole workspace')
    X.assert_exact(la.view(), ops.want(ep, residual), dtype, f'splitk {shape}')


_ACTS64 = {0: lambda v: v, 1: lambda v: v * torch.tanh(F.softplus(v)), 2: lambda v: F.leaky_relu(v, 0.1),
           3: lambda v: v * torch.sigmoid(v)}


@pytest.mark.parametrize('row', SPLITK_F32, ids=_ids([r[0] for r in SPLITK_F32]))
def test_splitk_f32_float_operands(gpu_device, row):
    """randn operands, every activation, residual and two-stage epilogue through views: within the 1e-4 * (1 + |ref|)
    of the float64 convolution that test_gpu_parity.py holds the unsplit fp32 tiles to."""
    shape = row[0]
    dev = gpu_device
    N, Hh, W, Cin, Cout, K, s, p = shape
    g = torch.Generator(device=dev).manual_seed(11)
    rn = lambda *sz: torch.randn(*sz, generator=g, device=dev)
    ru = lambda *sz: torch.rand(*sz, generator=g, device=dev)
    x, w = rn(N, Hh, W, Cin), rn(Cout, Cin, K, K) * (1.0 / (Cin * K * K)) ** 0.5
    Ho, Wo = X.out_size(Hh, K, s, p), X.out_size(W, K, s, p)
    res = rn(N, Ho, Wo, Cout)
    s1, t1, s2, t2 = ru(Cout) + 0.5, rn(Cout) * 0.1, ru(Cout) + 0.5, rn(Cout) * 0.1
    conv64 = X.fwd_ref(x, w, s, p)
    wp = w.permute(0, 2, 3, 1).contiguous()
    xbuf = torch.full((N, Hh, W, Cin + 8), OUTSIDE, device=dev)
    xbuf[..., 4:4 + Cin] = x
    rbuf = torch.full((N, Ho, Wo, Cout + 12), OUTSIDE, device=dev)
    rbuf[..., 4:4 + Cout] = res
    ybuf = torch.empty(N, Ho, Wo, Cout + 12, device=dev)
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, Hh, W, Cin, Ho, Wo, Cout
    d.KH, d.KW, d.stride, d.pad = K, K, s, p
    d.x_cstride, d.x_coff, d.y_cstride, d.y_coff, d.r_cstride, d.r_coff = Cin + 8, 4, Cout + 12, 8, Cout + 12, 4
    d.slope1 = d.slope2 = 0.1
    ks = C.c_int(0)
    nbytes = int(L.lib().yv4_conv_splitk_workspace(C.byref(d), C.byref(ks)))
    assert ks.value == row[2]
    ws = Workspace(dev, nbytes)
    for act in (0, 1, 2, 3):
        d.act1 = d.act2 = act
        ybuf.fill_(SENTINEL)
        ws.reset()
        L.check(L.lib().yv4_conv_bn_act_fwd_splitk(C.byref(d), xbuf.data_ptr(), wp.data_ptr(), s1.data_ptr(), t1.data_ptr(),
                                                   s2.data_ptr(), t2.data_ptr(), rbuf.data_ptr(), ybuf.data_ptr(), ws.ptr(),
                                                   nbytes, _stream()), 'yv4_conv_bn_act_fwd_splitk')
        torch.cuda.synchronize()
        ref = _ACTS64[act](conv64 * s1.double() + t1.double()) + res.double()
        ref = _ACTS64[act](ref * s2.double() + t2.double())
        assert bool((ybuf[..., :8] == SENTINEL).all()) and bool((ybuf[..., 8 + Cout:] == SENTINEL).all())
        assert ws.guard_intact()
        P.close(ybuf[..., 8:8 + Cout], ref, 1e-4, f'splitk {shape} act {act}')


@pytest.mark.parametrize('dtype', H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('index', range(len(H.SPLITK_SHAPES)), ids=_ids(H.SPLITK_SHAPES))
def test_splitk_h16_exact(gpu_device, dtype, index):
    """The 16-bit split-K at fp32 output (nothing hidden by the output's rounding) and at 16-bit output (rounded once)."""
    shape = H.SPLITK_SHAPES[index]
    nk, ways, splits, per, last = SPLITK_H16[index]
    _splitk_exact(gpu_device, dtype, F32, shape, nk, ways, splits, per, last, [('bare', True), ('full', True)])
    _splitk_exact(gpu_device, dtype, dtype, shape, nk, ways, splits, per, last, [('bare', False), ('full', True)])


# ---------------------------------------------------------------------------------------------------------------------
# c. every forward route by tile id
# ---------------------------------------------------------------------------------------------------------------------
def _k(shapes, K, s, p):
    return [tuple(sh) + (K, s, p) for sh in shapes]


def _is_stem(sh):
    return sh[3] == 3 and sh[5:] == (3, 1, 1)


DMA_TILES = [L.TILE_DMA_64x64, L.TILE_DMA_128x64, L.TILE_DMA_128x128]
# name -> (tile ids, shapes, {output kind: epilogue names that the route takes}, {output kind: epilogues it must refuse})
# output kind 'same': the operand type; 'f32': fp32 from 16-bit operands
ROUTES_F32 = {
    'generic': ([L.TILE_128x128, L.TILE_128x64, L.TILE_64x128, L.TILE_64x64], P.SHAPES, {'same': ['bare', 'full']}, {}),
    'dma': (DMA_TILES, [s for s in P.SHAPES if s[3] % 32 == 0], {'same': ['bare', 'full']}, {}),
    'stem': ([L.TILE_STEM], [s for s in P.SHAPES if _is_stem(s)], {'same': ['bare', 'one']}, {'same': ['full', 'nores']}),
    'ws1x1': ([L.TILE_WS_1x1], _k(P.WS_SHAPES_F32, 1, 1, 0), {'same': ['bare', 'nores']}, {'same': ['full']}),
    'wide': (P.WGF_TILES, P.WGF_SHAPES, {'same': ['bare', 'full']}, {}),
    'w3x3': (P.W3F_TILES, _k(P.W3F_SHAPES, 3, 1, 1), {'same': ['bare', 'full']}, {}),
}
ROUTES_H16 = {
    'generic': ([0, 1, 2, 3], H.SHAPES, {'same': ['bare', 'full'], 'f32': ['bare', 'full']}, {}),
    'pp3x3': ([4], _k(H.PP3_SHAPES, 3, 1, 1), {'same': ['bare', 'full']}, {'f32': ['bare']}),
    'w3x3': (H.W3_TILES, _k([s for s in H.PP3_SHAPES if s[4] % 16 == 0], 3, 1, 1), {'same': ['bare', 'full']}, {'f32': ['bare']}),
    'wide': (H.WIDE_TILES, H.WIDE_SHAPES, {'same': ['bare', 'full']}, {'f32': ['bare']}),
    'ws1x1': ([6], _k(H.WS_SHAPES, 1, 1, 0), {'same': ['bare', 'full'], 'f32': ['bare', 'nores']}, {'f32': ['full']}),
    's3x3': ([7], _k(H.S3_SHAPES, 3, 1, 1), {'same': ['bare', 'full']}, {'f32': ['bare']}),
}


def _route_params(routes):
    return [pytest.param(name, sh, id=f'{name}-{_ids([sh])[0]}') for name, r in routes.items() for sh in r[1]]


def _route_exact(dev, routes, name, shape, dtype):
    tiles, _, takes, refuses = routes[name]
    shape = laid_out(shape, dtype)
    ops = ops_for(dev, shape)
    for kind, names in takes.items():
        odt = dtype if kind == 'same' else F32
        for ep_name in names:
            outs = [run_exact(ops, dtype, odt, ep_name, t, f'{name} {NAME[dtype]}->{NAME[odt]} tile {t} {shape}') for t in tiles]
            assert all(torch.equal(outs[0], o) for o in outs[1:])
    for kind, names in refuses.items():
        odt = dtype if kind == 'same' else F32
        for ep_name in names:
            for t in tiles:
                assert_refused(ops, dtype, odt, ep_name, t, f'{name} {NAME[dtype]}->{NAME[odt]} tile {t} {shape}')


@pytest.mark.parametrize('name,shape', _route_params(ROUTES_F32))
def test_fwd_routes_f32_exact(gpu_device, name, shape):
    """Every fp32 tile id on its tolerance test's shapes: the bare convolution and the largest epilogue the route takes
    equal float64 bit for bit, through views; an epilogue it does not take is refused with y untouched."""
    _route_exact(gpu_device, ROUTES_F32, name, shape, F32)


@pytest.mark.parametrize('dtype', H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('name,shape', _route_params(ROUTES_H16))
def test_fwd_routes_h16_exact(gpu_device, name, shape, dtype):
    """Every 16-bit tile id: at fp32 output where the route writes one (refused with y untouched where it does not),
    and at 16-bit output against the float64 result rounded once."""
    _route_exact(gpu_device, ROUTES_H16, name, shape, dtype)


@pytest.mark.parametrize('shape', P.SHAPES, ids=_ids(P.SHAPES))
def test_fwd_f32_dma_and_stem_tiles_refuse_other_shapes(gpu_device, shape):
    """The pairs test_conv_shapes_and_tiles skips ('fast-path kernels need Cin % 32 == 0', 'stem kernel: 3x3 s1 p1 on the
    3-channel image only') are refusals of the entry point, not wrong answers."""
    ops = ops_for(gpu_device, laid_out(shape, F32))
    tiles = (DMA_TILES if shape[3] % 32 else []) + ([] if _is_stem(shape) else [L.TILE_STEM])
    assert tiles
    for t in tiles:
        assert_refused(ops, F32, F32, 'bare', t, f'tile {t} {shape}')


@pytest.mark.parametrize('shape', _k(P.WS_SHAPES_F32, 1, 1, 0), ids=_ids(_k(P.WS_SHAPES_F32, 1, 1, 0)))
def test_fwd_f32_ws1x1_shares_the_dma_tiles_order(gpu_device, shape):
    """Documented as one summation order (a plan picks either by batch size): the weight-stationary 1x1 kernel and the
    LDS-DMA tiles, bit for bit and exact."""
    ops = ops_for(gpu_device, shape)
    outs = [run_exact(ops, F32, F32, 'nores', t, f'tile {t} {shape}') for t in [L.TILE_WS_1x1] + DMA_TILES]
    assert all(torch.equal(outs[0], o) for o in outs[1:])


SHARED_H16 = [
    # the wide 3x3, ping-pong 3x3 and general wide kernels against the generic 128x64 tile (test_gpu_h16.py: the
    # *_matches_generic_bitwise tests)
    ((2, 19, 19, 128, 128, 3, 1, 1), [2, 4] + H.W3_TILES + H.WIDE_TILES),
    ((2, 19, 19, 128, 128, 3, 2, 1), [2] + H.WIDE_TILES),
    ((2, 19, 19, 512, 256, 1, 1, 0), [2] + H.WIDE_TILES),
]


@pytest.mark.parametrize('dtype', H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape,tiles', SHARED_H16, ids=_ids([s for s, _ in SHARED_H16]))
def test_fwd_h16_wide_and_pp_share_the_generic_order(gpu_device, dtype, shape, tiles):
    ops = ops_for(gpu_device, shape)
    outs = [run_exact(ops, dtype, dtype, 'full', t, f'{NAME[dtype]} tile {t} {shape}') for t in tiles]
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize('dtype', H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape', SD.SHAPES, ids=['x'.join(map(str, s)) for s in SD.SHAPES])
def test_stem_down_exact(gpu_device, dtype, shape):
    """yv4_stem_down_fwd_h16 on {-1, 1} images and stem weights: the stem's stored 16-bit output (at most 57, in halves:
    seven bits) is exact, so the stride-2 convolution on it and its epilogue equal float64, rounded once."""
    dev = gpu_device
    N, Hh, W, C1, C2 = shape
    x = X.int_operand((N, Hh, W, 3), 21, dev, big=True)
    w1 = X.int_operand((C1, 3, 3, 3), 22, dev, big=True)
    w2 = X.int_operand((C2, C1, 3, 3), 23, dev)
    e1 = X.Epilogue(C1, 24, dev, True, X.ACT_LEAKY)
    e2 = X.Epilogue(C2, 25, dev, True, X.ACT_LEAKY)
    e1.guard(27, 1, 1)
    a = X.fwd_epilogue_ref(x, w1, 1, 1, e1)
    assert torch.equal(a.to(dtype).double(), a), 'the stem output is not exact in the 16-bit type'
    halves = X.guard(9 * C1, int((a.abs().max() * 2).item()), X.amax(w2))      # the second convolution, in halves
    X.guard(1, (halves * X.amax(e2.s1) + 2 * X.amax(e2.t1)) * 2)               # its epilogue: act2 adds a fractional bit
    ref = X.fwd_epilogue_ref(a, w2, 2, 1, e2)
    Ho, Wo = X.out_size(Hh, 3, 2, 1), X.out_size(W, 3, 2, 1)
    w1p = torch.zeros(C1, 3, 3, 4, device=dev)
    w1p[..., :3] = w1.permute(0, 2, 3, 1)
    w2p = w2.permute(0, 2, 3, 1).contiguous().to(dtype)
    xn = x.permute(0, 3, 1, 2).contiguous()
    for y_off in (0, 16):
        ys = C2 + y_off + (8 if y_off else 0)
        ybuf = torch.full((N, Ho, Wo, ys), SENTINEL, dtype=dtype, device=dev)
        L.check(L.lib().yv4_stem_down_fwd_h16(CODE[dtype], xn.data_ptr(), N, Hh, W, w1p.data_ptr(), e1.s1.data_ptr(),
                                              e1.t1.data_ptr(), C1, X.ACT_LEAKY, 0.5, w2p.data_ptr(), e2.s1.data_ptr(),
                                              e2.t1.data_ptr(), C2, X.ACT_LEAKY, 0.5, ybuf.data_ptr(), ys, y_off, _stream()),
                'yv4_stem_down_fwd_h16')
        torch.cuda.synchronize()
        assert bool((ybuf[..., :y_off] == SENTINEL).all()) and bool((ybuf[..., y_off + C2:] == SENTINEL).all())
        X.assert_exact(ybuf[..., y_off:y_off + C2], ref, dtype, f'stem_down {NAME[dtype]} {shape} y_off {y_off}')
