"""The SPP, nearest-resample and zero-dilation kernels (csrc/elementwise.hip, elementwise_h16.hip, spp_lds.h,
elementwise_bwd.hip) through the C ABI, bit for bit against the float64 references of tests/_pool_ref.py.

Operands are exact in every type (tests/_pool_ref.py: ``distinct_map`` has no tie in any window, ``tie_map`` ties in
nearly every one; gradients are integers from {-2, -1, 1, 2}), so every sum is an integer far below 2**24: the result
does not depend on the order of the atomics, and a correct kernel equals ``ref64.float()`` -- or ``ref64.to(dtype)``
where it writes a 16-bit tensor -- exactly.  Every tensor a kernel sees sits inside a larger allocation filled with a
canary, channel slices sit inside wider pixel strides filled with the same canary, and nothing but the view the kernel
is meant to write may change.

Dispatch of ``yv4_spp_pool_bwd``: the LDS-resident form runs while
``H*W*cg*(3*keybytes + accbytes) <= 64 KB`` and ``H*W*cg <= 4096``; above, the default mode takes the atomic form
and the deterministic mode refuses.  ``lds_limit`` restates that and ``BOUNDARY`` sits on both sides of each limit.
"""
import contextlib
import math

import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib, ops

import _exact_ref as X
import _pool_ref as P

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = {F32: 'f32', BF16: 'bf16', F16: 'f16'}
MAKERS = {'distinct': P.distinct_map, 'tie': P.tie_map}
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -2
PAD = 64                       # canary elements in front of and behind every tensor (keeps 16-byte alignment)
CANARY = 16384.0               # finite, exact in every type, larger than any operand: a kernel that reads it shows
GROUP_TAIL = {F32: 36, BF16: 20, F16: 20}       # the issue's channel counts; 20 leaves half an 8-channel group


def _hw(s):
    return 'x'.join(map(str, s))


@contextlib.contextmanager
def det_mode(on):
    was = pkg.deterministic()
    pkg.set_deterministic(on)
    try:
        yield
    finally:
        pkg.set_deterministic(was)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Boxed:
    """A tensor of ``shape`` inside a canary-filled allocation; ``written`` marks what a kernel may change."""

    def __init__(self, shape, dtype, dev, fill=CANARY):
        n = math.prod(shape)
        self.whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.t = self.whole[PAD:PAD + n].view(shape)
        self.mask = torch.zeros(n + 2 * PAD, dtype=torch.bool, device=dev)
        self.written = self.mask[PAD:PAD + n].view(shape)
        self.snap = None

    def arm(self):
        self.snap = self.whole.clone()
        return self

    def ptr(self):
        assert self.t.data_ptr() % 16 == 0
        return self.t.data_ptr()

    def assert_untouched_outside(self, what):
        keep = ~self.mask
        same = bits(self.whole)[keep] == bits(self.snap)[keep]
        assert bool(same.all()), f'{what}: {int((~same).sum())} elements outside the written view changed'


def nhwc(t, dev):
    return t.permute(0, 2, 3, 1).to(dev)


def status(st, what):
    return f'{what}: status {st}: ' + _lib.lib().yv4_last_error().decode('utf-8', 'replace')


_maps, _bwd_cases = {}, {}


def spp_map(shape, dtype, maker):
    """The input map of one SPP case, made once and left unchanged."""
    key = (tuple(shape), dtype, maker)
    if key not in _maps:
        x = MAKERS[maker](shape, dtype, 100)
        if maker == 'tie' and shape[2] * shape[3] > 1:
            x.view(-1)[:2] = torch.tensor([-0.0, 0.0], dtype=dtype)       # a -0 ahead of a +0 inside one window
        _maps[key] = x
    return _maps[key]


def spp_case(shape, dtype, maker):
    """x, the integer gradient of the concat and the float64 dx of one SPP case, computed once."""
    key = (tuple(shape), dtype, maker)
    if key not in _bwd_cases:
        N, C, H, W = shape
        x = spp_map(shape, dtype, maker)
        dcat = X.int_operand((N, 4 * C, H, W), 200, 'cpu', dtype)
        _bwd_cases[key] = (x, dcat, P.spp_cat_bwd_ref(x, dcat))
    return _bwd_cases[key]


def lds_limit(dtype, det):
    """The largest H*W that yv4_spp_pool_bwd keeps on the LDS form (the launcher's two conditions)."""
    cg, key = (4, 8) if dtype == F32 else (8, 4)
    return min(65536 // (cg * (3 * key + (8 if det else 4))), 4096 // cg)


def spp_bwd(dev, x, dcat, views=False, det=False, dx_fill=0.0, geom=None):
    """One yv4_spp_pool_bwd call.  ``views``: x and dcat as channel slices of wider pixel strides.  ``geom`` overrides
    (C, x_cstride, x_coff, d_cstride, d_coff) as passed to the ABI (for the refusals).  Returns (status, dx NCHW on the
    CPU); asserts that the inputs and everything around dx kept their bits."""
    N, C, H, W = x.shape
    xcs, xco, dcs, dco = (4 * C + 8, 4, 4 * C + 12, 8) if views else (4 * C, 0, 4 * C, 0)
    xb = Boxed((N, H, W, xcs), x.dtype, dev)
    xb.t[..., xco:xco + C] = nhwc(x, dev)                 # the pool slices of the concat stay canary: they are not read
    db = Boxed((N, H, W, dcs), x.dtype, dev)
    db.t[..., dco:dco + 4 * C] = nhwc(dcat, dev)
    ob = Boxed((N, H, W, C), F32, dev, fill=float('nan'))
    ob.t.fill_(dx_fill)
    aC, axcs, axco, adcs, adco = geom or (C, xcs, xco, dcs, dco)
    for b in (xb, db, ob):
        b.arm()
    with det_mode(det):
        st = _lib.lib().yv4_spp_pool_bwd(xb.ptr(), axcs, axco, db.ptr(), adcs, adco, ob.ptr(), N, H, W, aC,
                                         _lib.DTYPE_CODE[x.dtype], ops.stream_ptr())
    torch.cuda.synchronize()
    if st == OK:
        ob.written[...] = True
    for b, name in ((xb, 'xcat'), (db, 'dcat'), (ob, 'dx')):
        b.assert_untouched_outside(f'spp_pool_bwd {name}')
    return st, ob.t.permute(0, 3, 1, 2).cpu()


NCHW = ('n', 'c', 'h', 'w')


def assert_dx(got, ref64, what):
    X.assert_exact(got, ref64, F32, what, names=NCHW)


# ---- SPP backward ----------------------------------------------------------------------------------------------------
def test_lds_limits_are_the_documented_table():
    assert {(d, m): lds_limit(d, m) for d in (F32, BF16) for m in (False, True)} == {
        (F32, False): 585, (F32, True): 512, (BF16, False): 512, (BF16, True): 409}
    assert lds_limit(F16, False) == 512 and lds_limit(F16, True) == 409


BOUNDARY = [(15, 39), (2, 293), (16, 32), (19, 27), (1, 409), (10, 41)]       # 585 | 586, 512 | 513, 409 | 410 pixels


@pytest.mark.parametrize('hw', BOUNDARY, ids=_hw)
@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_spp_backward_on_both_sides_of_every_dispatch_boundary(gpu_device, dtype, det, hw):
    """At and one pixel above each limit of the table: on the LDS form the exact answer (deterministic mode: the same
    bits twice); above it the default mode gives the same exact answer through the atomic form and the deterministic
    mode refuses with YV4_E_UNSUPPORTED and leaves dx alone.  16 x 32 in 16 bits is the launch that asks for exactly
    64 KB of dynamic LDS."""
    H, W = hw
    shape = (2, GROUP_TAIL[dtype], H, W)
    for maker in MAKERS:
        x, dcat, ref = spp_case(shape, dtype, maker)
        what = f'{maker} {IDS[dtype]} {H}x{W} det={det}'
        if det and H * W > lds_limit(dtype, det):
            st, dx = spp_bwd(gpu_device, x, dcat, det=True, dx_fill=7.0)
            assert st == E_UNSUPPORTED, status(st, what)
            assert bool((dx == 7.0).all()), f'{what}: a refused call wrote dx'
            continue
        st, dx = spp_bwd(gpu_device, x, dcat, det=det)
        assert st == OK, status(st, what)
        assert_dx(dx, ref, what)
        if det:
            st2, dx2 = spp_bwd(gpu_device, x, dcat, det=True)
            assert st2 == OK and torch.equal(bits(dx), bits(dx2)), f'{what}: two runs differ'


GEOMETRY = [(3, 4, 19, 19), (1, 4, 1, 1), (2, 4, 1, 23), (1, 8, 3, 40), (2, 8, 40, 3), (3, 0, 7, 5), (1, 0, 13, 20),
            (2, 0, 24, 25)]                                                     # C = 0: the type's GROUP_TAIL count


@pytest.mark.parametrize('views', [False, True], ids=['dense', 'sliced'])
@pytest.mark.parametrize('shape', GEOMETRY, ids=_hw)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_spp_backward_sizes_geometry_and_channel_slices(gpu_device, dtype, shape, views):
    """N = 3, C = 4 and a C that ends inside a channel group, maps narrower or shorter than a window, a 600-pixel map on
    the atomic form (24 x 25), dense and as channel slices (x_cstride = 4C + 8 at 4, d_cstride = 4C + 12 at 8), in the
    default and the deterministic mode."""
    N, C, H, W = shape
    shape = (N, C or GROUP_TAIL[dtype], H, W)
    for maker in MAKERS:
        x, dcat, ref = spp_case(shape, dtype, maker)
        for det in (False, True):
            if det and H * W > lds_limit(dtype, True):
                continue
            what = f'{maker} {IDS[dtype]} {_hw(shape)} sliced={views} det={det}'
            st, dx = spp_bwd(gpu_device, x, dcat, views=views, det=det)
            assert st == OK, status(st, what)
            assert_dx(dx, ref, what)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_spp_backward_atomic_form_takes_a_second_grid_stride_trip(gpu_device, dtype):
    """2 x 40 x 36 x 736: N*H*W*C/4 = 529 920 items for a grid capped at 2048 x 256 = 524 288 threads."""
    shape = (2, 736, 40, 36)
    assert shape[0] * shape[2] * shape[3] * shape[1] // 4 > 2048 * 256
    x, dcat, ref = spp_case(shape, dtype, 'distinct')
    st, dx = spp_bwd(gpu_device, x, dcat, views=(dtype == BF16))
    assert st == OK, status(st, 'second trip')
    assert_dx(dx, ref, f'second trip {IDS[dtype]}')


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_spp_backward_deterministic_shared_exponent(gpu_device, dtype):
    """Real-valued gradients through the fixed-point accumulator: gradients k * 2**-20 (k in {-2, -1, 1, 2}) and, in
    the first channel group of image 0, one gradient of 1000.

    Bound, from the kernel's own arithmetic: a workgroup (one image x one channel group) takes e = the biased fp32
    exponent of its largest |g| and scale = 2**(166 - e); every contribution is rounded to an integer multiple of
    q = 1 / scale = 2**(e - 166), an error of at most q / 2 each; the integer sum is exact, and the conversion back
    rounds once to fp32.  So |dx - ref| <= terms * q / 2 + ulp32(ref) / 2 with ``terms`` the number of contributions
    the reference scattered to that element.  (Here q = 2**-30 next to the 1000 and 2**-58 elsewhere, both finer than
    the gradients' 2**-20 grid, so the first term is an allowance, not an observed error.)  Two runs give the same
    bits."""
    N, C, H, W = 2, 16, 13, 20
    cg = 4 if dtype == F32 else 8
    x = P.distinct_map((N, C, H, W), dtype, 31)
    dcat = (X.int_operand((N, 4 * C, H, W), 32, 'cpu').double() * 2.0 ** -20)
    dcat[0, C + 1, 5, 7] = 1000.0                          # a pool-5 gradient of channel 1
    dcat = dcat.to(dtype)
    assert torch.equal(dcat.double().to(dtype), dcat) and float(dcat[0, C + 1, 5, 7]) == 1000.0
    ref, terms = P.spp_cat_bwd_ref(x, dcat, return_terms=True)
    # e per workgroup: the largest |g| over the four branches of its channels
    gmax = dcat.double().abs().view(N, 4, C // cg, cg, H * W).amax((1, 3, 4))          # (N, groups)
    e = torch.frexp(gmax.float())[1] + 126                                             # biased exponent of a normal fp32
    q = torch.ldexp(torch.ones_like(gmax), (e - 166).to(torch.int32))
    assert float(q[0, 0]) == 2.0 ** -30 and float(q[1, 0]) == 2.0 ** -58
    q = q.view(N, C // cg, 1, 1, 1).expand(N, C // cg, cg, H, W).reshape(N, C, H, W)
    ulp = torch.ldexp(torch.ones_like(ref), (torch.frexp(ref.abs().float())[1] - 24).to(torch.int32))
    bound = terms * q / 2 + ulp / 2
    st, dx = spp_bwd(gpu_device, x, dcat, det=True)
    assert st == OK, status(st, 'shared exponent')
    err = (dx.double() - ref).abs()
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), (f'{IDS[dtype]}: error {float(err.view(-1)[worst]):.3e} above the bound '
                                        f'{float(bound.reshape(-1)[worst]):.3e} at flat index {worst}')
    st2, dx2 = spp_bwd(gpu_device, x, dcat, det=True)
    assert st2 == OK and torch.equal(bits(dx), bits(dx2))
    # the default mode on the same operands: float atomics in arrival order, every partial sum within fp32's reach
    st3, dx3 = spp_bwd(gpu_device, x, dcat, det=False)
    assert st3 == OK
    assert bool(((dx3.double() - ref).abs() <= terms * ulp).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_spp_backward_refusals(gpu_device, dtype):
    """Channel counts, strides or offsets that are no multiple of 4, and views that exceed their pixel stride: refused
    with YV4_E_INVALID before anything is written."""
    C = 8
    x, dcat, _ = spp_case((1, C, 7, 5), dtype, 'distinct')
    full = (C, 4 * C + 8, 4, 4 * C + 12, 8)
    bad = {'C % 4': (6,) + full[1:], 'x_cstride % 4': (C, 4 * C + 6, 4, 4 * C + 12, 8), 'x_coff % 4': (C, 4 * C + 8, 2, 4 * C + 12, 8),
           'd_cstride % 4': (C, 4 * C + 8, 4, 4 * C + 10, 8), 'd_coff % 4': (C, 4 * C + 8, 4, 4 * C + 12, 6),
           'x view beyond its stride': (C, 4 * C + 8, 4 * C + 4, 4 * C + 12, 8),
           'd view beyond its stride': (C, 4 * C + 8, 4, 4 * C + 12, 16)}
    for name, geom in bad.items():
        st, dx = spp_bwd(gpu_device, x, dcat, views=True, dx_fill=7.0, geom=geom)
        assert st == E_INVALID, status(st, name)
        assert bool((dx == 7.0).all()), f'{name}: a refused call wrote dx'
    st, _ = spp_bwd(gpu_device, x, dcat, views=True, geom=full)
    assert st == OK, status(st, 'the same call with a valid geometry')


# ---- SPP forward -----------------------------------------------------------------------------------------------------
def spp_fwd(dev, x, views):
    """yv4_spp_pool_fwd / _h16 on a concat buffer whose x slice is filled and whose pool slices hold the canary.
    Returns (status, the 4C-channel concat NCHW on the CPU)."""
    N, C, H, W = x.shape
    al = 4 if x.dtype == F32 else 8
    cs, co = (4 * C + 2 * al, al) if views else (4 * C, 0)
    b = Boxed((N, H, W, cs), x.dtype, dev)
    b.t[..., co:co + C] = nhwc(x, dev)
    b.arm()
    b.written[..., co + C:co + 4 * C] = True
    L = _lib.lib()
    if x.dtype == F32:
        st = L.yv4_spp_pool_fwd(b.ptr(), N, H, W, C, cs, co, ops.stream_ptr())
    else:
        st = L.yv4_spp_pool_fwd_h16(b.ptr(), N, H, W, C, cs, co, _lib.DTYPE_CODE[x.dtype], ops.stream_ptr())
    torch.cuda.synchronize()
    b.assert_untouched_outside('spp_pool_fwd')
    return st, b.t[..., co:co + 4 * C].permute(0, 3, 1, 2).cpu()


# (N, C or 0 for the smallest aligned count, H, W): the LDS form up to 512 pixels (kSppLdsMaxHW), the chained 5x5 pools
# above it, and the 169-tap form once N*H no longer fits a grid dimension, at its smallest shape
FWD = [(2, 0, 16, 32), (2, 0, 19, 27), (3, 24, 19, 19), (1, 0, 1, 1), (2, 0, 3, 40), (2, 8, 1, 23), (128, 0, 513, 1)]


def check_spp_fwd(dev, shape, dtype, maker, views):
    x = spp_map(shape, dtype, maker)
    st, cat = spp_fwd(dev, x, views)
    what = f'spp forward {maker} {IDS[dtype]} {_hw(shape)} sliced={views}'
    assert st == OK, status(st, what)
    assert cat.dtype == dtype
    assert torch.equal(cat.double(), P.spp_cat_ref(x)), what       # torch.equal: -0 == +0, the one freedom of a maximum


@pytest.mark.parametrize('views', [False, True], ids=['dense', 'sliced'])
@pytest.mark.parametrize('shape', FWD, ids=_hw)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_spp_forward_every_form(gpu_device, dtype, shape, views):
    N, C, H, W = shape
    C = C or (4 if dtype == F32 else 8)
    if N == 128:
        assert H * W > 512 and N * H > 65535                       # the 169-tap form
    for maker in MAKERS:
        check_spp_fwd(gpu_device, (N, C, H, W), dtype, maker, views)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_spp_forward_169_tap_form_takes_a_second_grid_stride_trip(gpu_device, dtype):
    """128 x 513 x 1 with nine 16-byte vectors per pixel: 590 976 items for a grid capped at 2048 x 256 threads."""
    al = 4 if dtype == F32 else 8
    N, C, H, W = 128, 9 * al, 513, 1
    assert N * H > 65535 and N * H * W * (C // al) > 2048 * 256
    check_spp_fwd(gpu_device, (N, C, H, W), dtype, 'distinct', True)


# ---- nearest resample ------------------------------------------------------------------------------------------------
RESAMPLE_FWD = [(2, 16, 7, 9, 14, 18), (1, 8, 10, 10, 19, 19), (2, 8, 13, 13, 20, 20), (1, 24, 5, 5, 5, 5),
                (2, 8, 3, 5, 24, 10), (1, 16, 4, 3, 4, 24)]


@pytest.mark.parametrize('geom', RESAMPLE_FWD, ids=_hw)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_resample_forward_into_a_slice(gpu_device, dtype, geom):
    """A channel slice of one buffer resampled into a channel slice of another: integer factors, unequal factors, the
    plain copy, and the non-integer sizes of the inference plans (10 -> 19, 13 -> 20).  The kernel moves fp32 words: a
    16-bit map is passed as an fp32 map of half the channels, the pairing ResampleIntoFunction uses."""
    check_resample_fwd(gpu_device, dtype, geom)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_resample_forward_takes_a_second_grid_stride_trip(gpu_device, dtype):
    """2 x 76 x 76 pixels of 48 16-byte words: 554 496 items for a grid capped at 2048 x 256 threads."""
    C = 192 if dtype == F32 else 384
    assert 2 * 76 * 76 * (C * dtype.itemsize // 16) > 2048 * 256
    check_resample_fwd(gpu_device, dtype, (2, C, 38, 38, 76, 76))


def check_resample_fwd(gpu_device, dtype, geom):
    N, C, Hs, Ws, Hd, Wd = geom
    k = 1 if dtype == F32 else 2
    x = P.distinct_map((N, C, Hs, Ws), dtype, 41)
    ref = P.resample_nearest_ref(x, Hd, Wd)
    scs, sco, dcs, dco = C + 8, 8, 2 * C + 16, C + 8
    sb = Boxed((N, Hs, Ws, scs), dtype, gpu_device)
    sb.t[..., sco:sco + C] = nhwc(x, gpu_device)
    db = Boxed((N, Hd, Wd, dcs), dtype, gpu_device)
    sb.arm(), db.arm()
    db.written[..., dco:dco + C] = True
    st = _lib.lib().yv4_resample_nearest_fwd(sb.ptr(), db.ptr(), N, Hs, Ws, Hd, Wd, C // k, scs // k, sco // k, dcs // k,
                                             dco // k, ops.stream_ptr())
    torch.cuda.synchronize()
    assert st == OK, status(st, 'resample forward')
    sb.assert_untouched_outside('resample source'), db.assert_untouched_outside('resample destination')
    got = db.t[..., dco:dco + C].permute(0, 3, 1, 2).cpu()
    assert torch.equal(got.double(), ref)


def resample_bwd(dev, dy, Hs, Ws, sliced, dims=None):
    N, C, Hd, Wd = dy.shape
    dcs, dco = (2 * C + 8, C + 4) if sliced else (C, 0)
    yb = Boxed((N, Hd, Wd, dcs), dy.dtype, dev)
    yb.t[..., dco:dco + C] = nhwc(dy, dev)
    xb = Boxed((N, Hs, Ws, C), dy.dtype, dev, fill=float('nan'))
    xb.t.fill_(7.0)
    yb.arm(), xb.arm()
    aHs, aWs, aHd, aWd, aC, adcs, adco = dims or (Hs, Ws, Hd, Wd, C, dcs, dco)
    st = _lib.lib().yv4_resample_nearest_bwd(yb.ptr(), xb.ptr(), N, aHs, aWs, aHd, aWd, aC, adcs, adco,
                                             _lib.DTYPE_CODE[dy.dtype], ops.stream_ptr())
    torch.cuda.synchronize()
    if st == OK:
        xb.written[...] = True
    yb.assert_untouched_outside('resample backward dy'), xb.assert_untouched_outside('resample backward dx')
    return st, xb.t.permute(0, 3, 1, 2).cpu()


RESAMPLE_BWD = [(2, 16, 7, 9, 2, 2), (3, 8, 5, 4, 3, 2), (1, 8, 3, 5, 8, 8), (2, 4, 6, 7, 1, 4), (1, 12, 4, 4, 8, 1),
                (2, 8, 5, 5, 1, 1)]


@pytest.mark.parametrize('sliced', [False, True], ids=['dense', 'sliced'])
@pytest.mark.parametrize('geom', RESAMPLE_BWD, ids=_hw)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_resample_backward(gpu_device, dtype, geom, sliced):
    """dx = the sum of the fy x fx gradient pixels that read each source pixel: equal and unequal factors, factor 8,
    factor 1 (which the code forwards as a copy), dy dense and as a slice at dy_coff = C + 4 of a 2C + 8 stride.
    Integer gradients: at most 64 terms of magnitude 2, exact in fp32, rounded once into a 16-bit dx."""
    check_resample_bwd(gpu_device, dtype, geom, sliced)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_resample_backward_takes_a_second_grid_stride_trip(gpu_device, dtype):
    """2 x 38 x 38 x 736: 531 392 four-channel items for a grid capped at 2048 x 256 threads."""
    assert 2 * 38 * 38 * (736 // 4) > 2048 * 256
    check_resample_bwd(gpu_device, dtype, (2, 736, 38, 38, 1, 2), True)


def check_resample_bwd(gpu_device, dtype, geom, sliced):
    N, C, Hs, Ws, fy, fx = geom
    dy = X.int_operand((N, C, Hs * fy, Ws * fx), 51, 'cpu', dtype)
    ref = P.resample_nearest_bwd_ref(dy, fy, fx)
    st, dx = resample_bwd(gpu_device, dy, Hs, Ws, sliced)
    assert st == OK, status(st, 'resample backward')
    X.assert_exact(dx, ref, dtype, f'resample backward {IDS[dtype]} {geom} sliced={sliced}', names=NCHW)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=IDS.get)
def test_resample_backward_refusals(gpu_device, dtype):
    """Factor 9, non-integer factors, misaligned channels and a view beyond its stride are refused and write nothing."""
    N, C, Hs, Ws = 1, 8, 2, 3
    dy = X.int_operand((N, C, 18, 27), 52, 'cpu', dtype)
    cs, co = 2 * C + 8, C + 4
    bad = {'factor 9': (2, 3, 18, 27, C, cs, co), 'non-integer': (4, 3, 18, 27, C, cs, co), 'C % 4': (2, 3, 16, 24, 6, cs, co),
           'coff % 4': (2, 3, 16, 24, C, cs, co + 2), 'beyond the stride': (2, 3, 16, 24, C, cs, cs - 4)}
    for name, dims in bad.items():
        st, dx = resample_bwd(gpu_device, dy, Hs, Ws, True, dims=dims)
        assert st == E_INVALID, status(st, name)
        assert bool((dx == 7.0).all()), f'{name}: a refused call wrote dx'


# ---- zero-dilation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 8, 5, 7), (1, 4, 1, 1), (3, 12, 9, 4), (2, 736, 19, 19)], ids=_hw)
@pytest.mark.parametrize('sliced', [False, True], ids=['dense', 'sliced'])
def test_dilate2_places_every_source_element_and_zeroes_the_rest(gpu_device, shape, sliced):
    """dst[n, 2y, 2x, c] = src[n, y, x, c] and exact zeros elsewhere: odd H and W, the source as a slice at
    src_coff = 4, and 2 x 38 x 38 x 736 (a second trip of the capped grid)."""
    N, C, H, W = shape
    if C == 736:
        assert N * 2 * H * 2 * W * (C // 4) > 2048 * 256
    src = X.int_operand(shape, 61, 'cpu')
    ref = P.dilate2_ref(src)
    cs, co = (C + 8, 4) if sliced else (C, 0)
    sb = Boxed((N, H, W, cs), F32, gpu_device)
    sb.t[..., co:co + C] = nhwc(src, gpu_device)
    db = Boxed((N, 2 * H, 2 * W, C), F32, gpu_device, fill=float('nan'))
    sb.arm(), db.arm()
    db.written[...] = True
    st = _lib.lib().yv4_dilate2_fwd(sb.ptr(), db.ptr(), N, H, W, C, cs, co, ops.stream_ptr())
    torch.cuda.synchronize()
    assert st == OK, status(st, 'dilate2')
    sb.assert_untouched_outside('dilate2 source'), db.assert_untouched_outside('dilate2 destination')
    got = db.t.permute(0, 3, 1, 2).cpu()
    assert torch.equal(bits(got), bits(ref.float())), 'dilate2: not the source in place over +0'
    assert int((got != 0).sum()) == src.numel()
