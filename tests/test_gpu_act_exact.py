"""The fused activations of the conv epilogues over their whole range, per route and tile id, through the C ABI.

A selector convolution (tests/_act_ref.py: 0 / 1 weights, integer operands, power-of-two affines) makes the argument
of the swept activation a known fp32 value in every route, so the activation itself is what is compared: Mish and
Swish against float64 within the bound derived from their operation count, LEAKY and NONE bit for bit, on a grid that
reaches the x >= 20 select, the packed form's exponent clamp, n + 2 == n, n + 2 == 2, flushed exponentials, +-0, tiny
and huge arguments (asserted per case from the tensors).  The rows of ``A.ROWS`` use different activation ids and
slopes in the two stages, so a route that took stage 1's id or slope in stage 2, or added the residual in the wrong
place, fails.  Every launch goes through channel-offset views into sentinel-filled buffers (test_gpu_fwd_exact.py's
Launch); an epilogue a route does not take must be refused with y untouched.

Each case prints ``ACT <route> <types> tile <id> [<row>]: worst err/bound <figure> at v = <argument>`` (a 16-bit or e4m3
output: the share of outputs that are not the reference's nearest code); DESIGN.md section 3 has the table.
"""
import ctypes as C
import os
import sys

import pytest
import torch

from mmdet_yolov4_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _act_ref as A  # noqa: E402
import test_gpu_fp8 as Q  # noqa: E402
import test_gpu_fwd_exact as E  # noqa: E402
import test_gpu_h16 as H  # noqa: E402
import test_gpu_stem_down as SD  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, A.F8
NAME = dict(E.NAME)
NAME[F8] = 'e4m3'
KINDS = ('one', 'two', 'res')


def smallest(shapes):
    """The shape of a route's list with the fewest outputs, M * Cout."""
    def outputs(s):
        N, Hh, W, Cin, Cout, K, st, p = s
        return N * A.out_size(Hh, K, st, p) * A.out_size(W, K, st, p) * Cout
    return min(shapes, key=outputs)


def row_kinds(names):
    """Which rows a route takes, from the epilogue names of test_gpu_fwd_exact.py's route tables."""
    names = set(names)
    if 'full' in names:
        return set(KINDS)
    return {'one', 'two'} if 'nores' in names else {'one'}


_CASES, _TRACES = {}, {}


def case_for(dev, shape, f8=False):
    key = (str(dev), tuple(shape), f8)
    if key not in _CASES:
        case = A.Case(shape, dev, f8)
        assert torch.equal(case.fwd64(), case.conv64)
        _CASES[key] = case
    return _CASES[key]


def trace_for(case, row, odt):
    """(Epi, Case with the row's residual, Trace): one reference per shape and row, shared by every tile and type; the
    coverage of the swept argument is asserted from the tensors, per output type."""
    key = (str(case.dev), case.shape, case.f8, row.name)
    if key not in _TRACES:
        ep = A.Epi(row, case.shape[4], case.dev)
        c = case.with_res(row.sweep)
        _TRACES[key] = (ep, c, A.Trace(c.conv64, ep, c.res if row.residual else None))
    ep, c, tr = _TRACES[key]
    gaps = A.coverage_gaps(tr.v, odt, A.act64(tr.v, A.ACT_MISH, 0.0))
    assert gaps == [], f'{row.name} {case.shape}: the grid misses {gaps}'
    return ep, c, tr


def judge(got, tr, odt, what, y_inv=1.0):
    ok, worst, at, msg = A.check(got, tr, odt, y_inv=y_inv)
    if odt == F32:
        print(f'ACT {what}: worst err/bound {worst:.3f} at v = {at!r} ({A.worst_ulps(got, tr.ref, tr.v >= -20):.2f} ulp over '
              f'v >= -20, {A.worst_ulps(got, tr.ref):.2f} ulp over all)')
    else:
        print(f'ACT {what}: {100 * worst:.2f} % of the outputs off the reference\'s nearest code, all inside the interval')
    assert ok, f'{what}: {msg}'


def run_rows(dev, shape, dtype, odt, tiles, kinds, what, call=None, rows=A.ROWS):
    """Every row on every tile: a row of a kind the route takes must pass on each tile and give the same bits on all of
    them, any other must be refused with y untouched.  ``call``: launch -> status (default: the plain entry)."""
    case = case_for(dev, shape)
    call = call or (lambda la: la.call())
    for row in rows:
        ep, c, tr = trace_for(case, row, odt)
        outs = []
        for t in tiles:
            la = E.Launch(c, dtype, odt, ep, row.residual, True, t)
            tag = f'{what} {NAME[dtype]}->{NAME[odt]} tile {t} [{row.name}]'
            if row.kind not in kinds:
                assert call(la) != 0, f'{tag}: accepted'
                assert la.untouched(), f'{tag}: refused, but y was written'
                continue
            L.check(call(la), tag)
            y = la.view().clone()
            judge(y, tr, odt, tag)
            outs.append(y)
        assert all(torch.equal(A._bits(outs[0]), A._bits(o)) for o in outs[1:]), f'{what} [{row.name}]: the tiles differ'


# ---------------------------------------------------------------------------------------------------------------------
# every tile id of the plain entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(E.ROUTES_F32))
def test_act_routes_f32(gpu_device, name):
    tiles, shapes, takes, _ = E.ROUTES_F32[name]
    shape = E.laid_out(smallest(shapes), F32)
    run_rows(gpu_device, shape, F32, F32, tiles, row_kinds(takes['same']), name)


@pytest.mark.parametrize('dtype', E.H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('name', list(E.ROUTES_H16))
def test_act_routes_h16(gpu_device, name, dtype):
    """16-bit operands: at 16-bit output (the interval of the rounded bound) and, where the route writes it, at fp32
    output, where nothing hides behind the output's rounding."""
    tiles, shapes, takes, _ = E.ROUTES_H16[name]
    shape = E.laid_out(smallest(shapes), dtype)
    for kind, names in takes.items():
        run_rows(gpu_device, shape, dtype, dtype if kind == 'same' else F32, tiles, row_kinds(names), name)


# ---------------------------------------------------------------------------------------------------------------------
# routes that share a form agree bit for bit
# ---------------------------------------------------------------------------------------------------------------------
GENERIC_F32 = E.ROUTES_F32['generic'][0]
AGREE_F32 = [
    # (shape, tiles, rows): every fp32 kernel family that takes the shape -- one scalar activation form, one order
    ((2, 19, 19, 64, 128, 3, 1, 1), GENERIC_F32 + E.DMA_TILES + E.P.W3F_TILES + E.P.WGF_TILES,
     ['leaky.5+r>mish', 'swish+r>leaky.5']),
    ((2, 19, 19, 128, 128, 1, 1, 0), GENERIC_F32 + E.DMA_TILES + [L.TILE_WS_1x1] + E.P.WGF_TILES, ['mish>none', 'swish']),
    ((1, 9, 37, 4, 16, 3, 1, 1), GENERIC_F32 + [L.TILE_STEM], ['mish', 'swish']),
]


@pytest.mark.parametrize('shape,tiles,rows', AGREE_F32, ids=E._ids([a[0] for a in AGREE_F32]))
def test_act_f32_tiles_agree(gpu_device, shape, tiles, rows):
    run_rows(gpu_device, shape, F32, F32, tiles, set(KINDS), 'f32 families', rows=[A.ROW[r] for r in rows])


@pytest.mark.parametrize('dtype', E.H16, ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape,tiles', E.SHARED_H16, ids=E._ids([s for s, _ in E.SHARED_H16]))
def test_act_h16_shared_order_tiles_agree(gpu_device, dtype, shape, tiles):
    """The tiles that test_fwd_h16_wide_and_pp_share_the_generic_order ties together, on the packed Mish in either stage."""
    rows = [A.ROW[r] for r in ('leaky.5+r>mish', 'mish+r>leaky.25', 'swish+r>leaky.5')]
    run_rows(gpu_device, shape, dtype, dtype, tiles, set(KINDS), 'h16 shared order', rows=rows)


# ---------------------------------------------------------------------------------------------------------------------
# split-K, the stem entry, the fused stem + stride-2 launch
# ---------------------------------------------------------------------------------------------------------------------
def _splitk_call(dev):
    state = {}

    def call(la):
        nbytes, ks = la.splitk_workspace()
        assert ks > 1 and nbytes > 0, 'the shape does not split'
        if state.get('n') != nbytes:
            state['n'], state['ws'] = nbytes, E.Workspace(dev, nbytes)
        ws = state['ws']
        ws.reset()
        rc = la.call(ws.ptr(), ws.nbytes)
        assert ws.guard_intact()
        return rc
    return call


def test_act_splitk_f32(gpu_device):
    shape = smallest([r[0] for r in E.SPLITK_F32])
    run_rows(gpu_device, shape, F32, F32, [0], set(KINDS), 'splitk', _splitk_call(gpu_device))


@pytest.mark.parametrize('dtype', E.H16, ids=['bf16', 'f16'])
def test_act_splitk_h16(gpu_device, dtype):
    shape = smallest(H.SPLITK_SHAPES)
    for odt in (dtype, F32):
        run_rows(gpu_device, shape, dtype, odt, [0], set(KINDS), 'splitk', _splitk_call(gpu_device))


@pytest.mark.parametrize('odt', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
def test_act_stem_entry(gpu_device, odt):
    """yv4_conv_stem_fwd (fp32 arithmetic, fp32 or 16-bit output): one stage, no residual."""
    shape = E.laid_out(smallest(E.ROUTES_F32['stem'][1]), F32)

    def call(la):
        la.ybuf.fill_(E.SENTINEL)
        rc = L.lib().yv4_conv_stem_fwd(C.byref(la.d), la.xbuf.data_ptr(), la.w.data_ptr(), la.ep.s1.data_ptr(),
                                       la.ep.t1.data_ptr(), la.ybuf.data_ptr(), E.CODE[odt], E._stream())
        torch.cuda.synchronize()
        return rc
    run_rows(gpu_device, shape, F32, odt, [0], {'one'}, 'stem entry', call, rows=[r for r in A.ROWS if r.kind == 'one'])


# (act1, slope1, act2, slope2): the first convolution stays exact (its 16-bit result is the operand of the second), the
# second sweeps the grid; ids and slopes differ between the two
STEM_DOWN = [
    (A.ACT_LEAKY, 1.0, A.ACT_MISH, 0.25), (A.ACT_LEAKY, 1.0, A.ACT_SWISH, 0.25), (A.ACT_LEAKY, 1.0, A.ACT_LEAKY, 0.25),
    (A.ACT_NONE, 0.25, A.ACT_LEAKY, 0.5), (A.ACT_LEAKY, 2.0, A.ACT_NONE, 0.25),
]


@pytest.mark.parametrize('dtype', E.H16, ids=['bf16', 'f16'])
def test_act_stem_down(gpu_device, dtype):
    """yv4_stem_down_fwd_h16: a selector stem (s = 1, t = 0, an activation that keeps k or halves it exactly) feeds a
    selector stride-2 convolution whose affine carries the grid."""
    dev = gpu_device
    N, Hh, W, C1, C2 = min(SD.SHAPES, key=lambda s: s[0] * ((s[1] - 1) // 2 + 1) * ((s[2] - 1) // 2 + 1) * s[4])
    Ho, Wo = A.out_size(Hh, 3, 2, 1), A.out_size(W, 3, 2, 1)
    # the image as the (N, H, W, 3) operand of a stride-2 selector: output (ho, wo) sees pixel (2 ho, 2 wo)
    img = A.Case((N, Hh, W, 3, C1, 3, 2, 1), dev)
    xn = img.x.permute(0, 3, 1, 2).contiguous()
    c1 = torch.arange(C1, device=dev)
    w1p = torch.zeros(C1, 3, 3, 4, device=dev)
    w1p[c1, 1, 1, c1 % 3] = 1.0
    c2 = torch.arange(C2, device=dev)
    w2 = torch.zeros(C2, 3, 3, C1, device=dev)
    w2[c2, 1, 1, c2 % C1] = 1.0
    w2p = w2.to(dtype)
    k = img.conv64[..., c2 % C1]                                 # (N, Ho, Wo, C2): the k that output channel c2 sees
    one, zero = torch.ones(C1, device=dev), torch.zeros(C1, device=dev)
    s2, t2 = A.band_affine(C2, dev)
    for act1, slope1, act2, slope2 in STEM_DOWN:
        a = A.act64(k, act1, slope1)
        assert torch.equal(a.to(dtype).double(), a), 'the stem output is not exact in the 16-bit type'
        row = A.Row(f'{A.ACT_NAMES[act1]}{slope1}>{A.ACT_NAMES[act2]}{slope2}', act2, slope2, False)
        ep = A.Epi(row, C2, dev)
        tr = A.Trace(a, ep)
        if act1 != A.ACT_LEAKY or slope1 == 1.0:
            gaps = A.coverage_gaps(tr.v, dtype, A.act64(tr.v, A.ACT_MISH, 0.0))
            assert gaps == [], gaps
        y_off = 16
        ys = C2 + y_off + 8
        ybuf = torch.full((N, Ho, Wo, ys), E.SENTINEL, dtype=dtype, device=dev)
        L.check(L.lib().yv4_stem_down_fwd_h16(E.CODE[dtype], xn.data_ptr(), N, Hh, W, w1p.data_ptr(), one.data_ptr(),
                                              zero.data_ptr(), C1, act1, slope1, w2p.data_ptr(), s2.data_ptr(),
                                              t2.data_ptr(), C2, act2, slope2, ybuf.data_ptr(), ys, y_off, E._stream()),
                'yv4_stem_down_fwd_h16')
        torch.cuda.synchronize()
        assert bool((ybuf[..., :y_off] == E.SENTINEL).all()) and bool((ybuf[..., y_off + C2:] == E.SENTINEL).all())
        judge(ybuf[..., y_off:y_off + C2].clone(), tr, dtype, f'stem_down {NAME[dtype]} [{row.name}]')


# ---------------------------------------------------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------------------------------------------------
F8_Y_INV = 0.5


@pytest.mark.parametrize('out', [F32, F8], ids=['f32', 'e4m3'])
@pytest.mark.parametrize('tile', [1, 2, 3])
def test_act_conv_f8(gpu_device, tile, out):
    """yv4_conv_bn_act_fwd_f8 on e4m3 integer codes, unit operand scales: fp32 output within the bound, e4m3 output
    inside the codes of the bound's ends (through y_inv and the +-448 clamp)."""
    dev = gpu_device
    k, stride, Cin, Cout, N, Hh, W = min(Q.MAP_CASES, key=lambda c: c[4] * (-(-c[5] // c[1])) * (-(-c[6] // c[1])) * c[3])
    case = case_for(dev, (N, Hh, W, Cin, Cout, k, stride, k // 2), f8=True)
    xoff, roff, yoff = 16, 8, 3
    x8 = torch.full((N, Hh, W, Cin + 32), 3.0, device=dev)
    x8[..., xoff:xoff + Cin] = case.x
    x8 = x8.to(F8).view(torch.uint8)
    w8 = case.weights(F32).reshape(Cout, -1).to(F8).view(torch.uint8)
    y_inv = F8_Y_INV if out == F8 else 1.0
    for row in A.ROWS:
        ep, c, tr = trace_for(case, row, F32)
        r8 = None
        if row.residual:
            r8 = torch.full((N, case.Ho, case.Wo, Cout + 16), 3.0, device=dev)
            r8[..., roff:roff + Cout] = c.res
            r8 = r8.to(F8).view(torch.uint8)
        two = row.two_stage
        y = Q._conv_f8(x8, w8, ep.s1, ep.t1, k, stride, Cout, out == F32, act1=(row.act1, row.slope1),
                       s2=ep.s2 if two else None, t2=ep.t2 if two else None, act2=(row.act2, row.slope2), res8=r8,
                       y_inv=y_inv, xv=(None, xoff), yv=(Cout + 5, yoff), rv=(None, roff), tile=tile)
        sentinel = -7.0 if out == F32 else 0x55
        assert bool((y[..., :yoff] == sentinel).all()) and bool((y[..., yoff + Cout:] == sentinel).all())
        got = y[..., yoff:yoff + Cout].clone()
        judge(got if out == F32 else got.view(F8), tr, out, f'f8 ->{NAME[out]} tile {tile} [{row.name}]', y_inv)
