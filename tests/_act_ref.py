"""References, error bounds and value grids for the fused activations of the conv epilogues
``y = act2((act1(conv * s1 + t1) + residual) * s2 + t2)`` (a helper module for the tests, not a conftest).

Driving the activation exactly: a selector convolution
------------------------------------------------------
The weights are 0 / 1 with one 1 per output channel, ``W[co, ci = co % Cin, kh = kw = pad] = 1``: output pixel
(n, ho, wo) of channel co is then x[n, ho * s, wo * s, co % Cin] -- one non-zero product, every other product 0 -- in
every route and summation order, bit for bit.  The operands are integers k that the operand type holds exactly
(|k| <= 256; for e4m3 the integers it represents).  Per output channel the affine is ``s = +-2**-j`` and
``t = b * 2**-j + base`` from ``BANDS``, chosen so that ``k * s + t`` is exact in fp32 whether the kernel uses an fma
or a multiply and an add (``k * s`` is a scaling by a power of two; the sum is asserted representable, ``Trace``).  The
pre-activation of the swept stage is therefore a known fp32 value.  'sweep1' rows put the bands into (s1, t1);
the 'sweep2' row (act1 NONE, s1 = 1, t1 = 0, a small-integer residual) puts them into (s2, t2).

References: float64, ``v * tanh(softplus(v))`` with softplus threshold 20, ``v * sigmoid(v)``, leaky.

Bounds (eps = 2**-23, one fp32 ulp in relative terms; a correctly rounded operation errs by eps / 2; the hardware
exp2 and reciprocal by eps each, as csrc/yv4_common.h states)
-----------------------------------------------------------------------------------------------------------------
LEAKY with a power-of-two slope and NONE: every step is exact, the result is the float64 value rounded once.

Mish, ``e = exp2(v * log2e); n = e * (e + 2); y = v * n * rcp(n + 2)`` (tanh(log1p(e^v)) == n / (n + 2) exactly):
  * t = fl(v * fl(log2 e)): the constant is off by < 2**-26 relative, the product by eps / 2: |dt| <= 0.63 eps |t|;
  * e = exp2(t): relative error  ln2 * |dt| + eps <= eps * (0.63 |v| + 1) =: eta;
  * n = e * (e + 2): d ln n / d ln e = (2e + 2) / (e + 2) <= 2, two roundings: rel(n) <= 2 eta + eps;
  * q = n / (n + 2): d ln q / d ln n = 2 / (n + 2) =: kappa (<= 1), so n's error arrives as kappa * (2 eta + eps);
  * the roundings behind n: n + 2 (eps / 2), rcp (eps), the two products (eps / 2 each): 2.5 eps.
  Sum: eps * ((1.26 |v| + 3) * kappa + 2.5) <= eps * ((2 |v| + 3) * kappa + 3), the form used (some slack on both terms).
  For v >= 20 the scalar form returns v, which is the reference; the packed form clamps the exponent at e^20, where
  n + 2 == n and n * rcp(n) is within 1.5 eps of 1.  Floor: where e or n is subnormal the hardware flushes it to 0
  (absolute error of the ratio < 2**-125, times |v|), and a subnormal result may be flushed: |v| * 2**-124 + 2**-125.
    |got - ref| <= eps * ((2 |v| + 3) * kappa + 3) * |ref| + |v| * 2**-124 + 2**-125
  The float64 reference with the softplus threshold differs from v * n / (n + 2) by < 1e-17 relative (v >= 20).

Swish, ``y = v * rcp(1 + exp2(-v * log2e))``: E = exp2(t) as above (eta); d = 1 + E has d ln d / d ln E = E / (1 + E)
<= min(1, e^-v), one rounding (eps / 2); rcp (eps); the product (eps / 2):
    |got - ref| <= eps * ((|v| + 2) * min(1, e^-v) + 3) * |ref| + |v| * 2**-124 + 2**-120
  Floor: for v <= -87.3 the reciprocal of d >= 2**126 is subnormal and flushed, losing < |v| * 2**-126; below v = -88.7
  exp2 overflows and the result is -0 where the reference is < 89 * 2**-128.

Two stages (``Trace``): an fp32 addition or fma whose exact result is representable and whose inputs are exact adds no
error; otherwise it adds half an ulp, 2**-24 * (|result| + incoming error) (+ 2**-149).  s2 is a power of two, so a
multiply-and-add rounds like the fma.  The error e_u of stage 2's argument reaches the output through the
activation's Lipschitz constant (``LIP``: Mish 1.09, Swish 1.10, leaky max(1, slope)), times 1 + 2**-12 because the
stage's own bound is evaluated at the reference argument and not at the perturbed one (its derivative is
< 2**-23 * 260 over the range), plus stage 2's own bound.

16-bit and e4m3 outputs: rounding is monotone, so ``got`` lies in [round(ref - bound), round(ref + bound)] (``check``);
the kernels round fp32 -> output type, so the interval ends are rounded float64 -> fp32 -> output type as well.
"""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_MISH, ACT_LEAKY, ACT_SWISH = 0, 1, 2, 3     # YV4_ACT_*
ACT_NAMES = {ACT_NONE: 'none', ACT_MISH: 'mish', ACT_LEAKY: 'leaky', ACT_SWISH: 'swish'}
LIP = {ACT_NONE: 1.0, ACT_MISH: 1.09, ACT_SWISH: 1.10}
EPS = 2.0 ** -23
F8 = torch.float8_e4m3fn


# ---------------------------------------------------------------------------------------------------------------------
# references and per-activation bounds
# ---------------------------------------------------------------------------------------------------------------------
def act64(v, act, slope):
    if act == ACT_MISH:
        return v * torch.tanh(F.softplus(v, threshold=20))
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == ACT_LEAKY:
        return torch.where(v >= 0, v, v * slope)
    return v


def mish_bound(v):
    """Bound on |mish_fast(v) - mish(v)| for an exact fp32 argument v (float64 tensor)."""
    ref = act64(v, ACT_MISH, 0.0).abs()
    e = torch.exp(v.clamp(max=60.0))
    kappa = torch.clamp(2.0 / (e * (e + 2.0) + 2.0), max=1.0)
    return EPS * ((2.0 * v.abs() + 3.0) * kappa + 3.0) * ref + v.abs() * 2.0 ** -124 + 2.0 ** -125


def swish_bound(v):
    ref = act64(v, ACT_SWISH, 0.0).abs()
    damp = torch.exp((-v).clamp(max=0.0))         # min(1, e^-v)
    return EPS * ((v.abs() + 2.0) * damp + 3.0) * ref + v.abs() * 2.0 ** -124 + 2.0 ** -120


def rep32(x64):
    """Where a float64 value is an fp32 value."""
    return x64.float().double() == x64


def _round_err(x64, err_in):
    """Error added by the fp32 rounding of an operation whose exact result is ``x64`` (+- err_in)."""
    exact = (err_in == 0) & rep32(x64)
    return torch.where(exact, torch.zeros_like(x64), 2.0 ** -24 * (x64.abs() + err_in) + 2.0 ** -149)


def _act_stage(u, err_u, act, slope):
    """(reference, bound) of one activation on the argument u +- err_u."""
    y = act64(u, act, slope)
    if act == ACT_NONE:
        return y, err_u
    if act == ACT_LEAKY:
        err = max(1.0, abs(slope)) * err_u
        return y, err + _round_err(y, err)          # v * slope: one product
    own = mish_bound(u) if act == ACT_MISH else swish_bound(u)
    return y, LIP[act] * err_u * (1.0 + 2.0 ** -12) + own


class Row:
    """One epilogue of the table: the stage-1 activation, whether a residual is added, the stage-2 activation (None: no
    second stage).  ``sweep``: which stage's affine carries the grid.  ``exact``: every step is exact (bound 0)."""

    def __init__(self, name, act1, slope1, residual, act2=None, slope2=0.0, sweep=1, exact=False):
        self.name, self.act1, self.slope1, self.residual = name, act1, slope1, residual
        self.two_stage, self.act2, self.slope2 = act2 is not None, (act2 if act2 is not None else ACT_NONE), slope2
        self.sweep, self.exact = sweep, exact

    @property
    def kind(self):
        """What a route has to take for this row: 'one' stage, 'two' stages without a residual, or 'res'."""
        return 'res' if self.residual else ('two' if self.two_stage else 'one')


ROWS = [
    Row('mish', ACT_MISH, 0.5, False),
    Row('swish', ACT_SWISH, 0.5, False),
    Row('leaky.25', ACT_LEAKY, 0.25, False, exact=True),
    Row('none+r>mish', ACT_NONE, 0.5, True, ACT_MISH, 0.25, sweep=2),       # the CSP concat form
    Row('mish>none', ACT_MISH, 0.5, False, ACT_NONE, 0.25),
    Row('leaky.5+r>mish', ACT_LEAKY, 0.5, True, ACT_MISH, 0.25),
    Row('mish+r>leaky.25', ACT_MISH, 0.5, True, ACT_LEAKY, 0.25),
    Row('swish+r>leaky.5', ACT_SWISH, 0.25, True, ACT_LEAKY, 0.5),
    Row('leaky.5+r>leaky.25', ACT_LEAKY, 0.5, True, ACT_LEAKY, 0.25, exact=True),
]
ROW = {r.name: r for r in ROWS}


# ---------------------------------------------------------------------------------------------------------------------
# the grid: operands k, bands (s, t) per channel
# ---------------------------------------------------------------------------------------------------------------------
# integers that e4m3 represents as well; the second list adds odd neighbours of the range limits for the wider types
K_F8 = [0, 1, -1, 20, 22, 18, 30, 9, 5, -5, -16, -18, -48, -80, -88, -96, -104, -112, -256, 256, 72, 96, 160, 176, 240,
        208, 128, -128, 2, -2, 12, -3]
K_INT = K_F8 + [21, 19, -17, -87, -100, -105, -110, 159, 161]
# name -> (sign, j, base, the residual and a non-trivial other-stage affine keep the row exact): v = sign*(k + b)*2**-j + base
BANDS = [
    ('ints', 1, 0, 0.0, True),          # v = k: every range limit from -256 to 256
    ('eighths', 1, 3, 0.0, True),       # v = k / 8: [-32, 32] in steps of 1/8 -- [8.7, 20), (20, 30]
    ('at20', 1, 19, 20.0, True),        # v = 20 + k 2**-19: exactly 20 and its fp32 neighbours
    ('tiny', 1, 28, 0.0, False),        # 0 < |v| <= 2**-20, +0
    ('negzero', -1, 28, -0.0, False),   # s < 0, t = -0: k = 0 gives -0
    ('x64', 1, -6, 0.0, True),          # up to 16384 >= 1e4
    ('x512', 1, -9, 0.0, True),         # up to 131072: beyond the fp16 maximum
    ('x2^100', 1, -100, 0.0, False),    # up to 3.2e32 >= 1e30
]
NB = len(BANDS)
RES_VALUES = [1, -2, 3, -1]


def out_size(H, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1


def _f8_ok(vals):
    t = torch.tensor(vals, dtype=torch.float32)
    return bool((t.to(F8).float() == t).all())


class Case:
    """The operands of one selector convolution (N, H, W, Cin, Cout, K, stride, pad) on ``device``; ``f8``: operands from
    the e4m3 integers.  Attributes as tests/test_gpu_fwd_exact.py's Ops, so that its Launch takes a Case: shape, dev,
    Ho, Wo, x (N, H, W, Cin) fp32, res, weights(dtype).  ``conv64``: the float64 convolution, i.e. the selected k."""

    def __init__(self, shape, device, f8=False):
        N, H, W, Cin, Cout, K, s, p = shape
        assert p < K and Cout >= NB
        self.shape, self.dev, self.f8 = tuple(shape), device, f8
        self.Ho, self.Wo = out_size(H, K, s, p), out_size(W, K, s, p)
        assert (self.Ho - 1) * s < H and (self.Wo - 1) * s < W, 'the selected tap must lie inside the image'
        ks = K_F8 if f8 else K_INT
        n = len(ks)
        M = N * self.Ho * self.Wo
        m = torch.arange(M).view(N, self.Ho, self.Wo, 1)
        ci = torch.arange(Cin).view(1, 1, 1, Cin)
        sel = torch.tensor(ks, dtype=torch.float32)[(m + 7 * ci) % n]                 # (N, Ho, Wo, Cin)
        # pixels no output selects: small non-zero integers (they meet zero weights only)
        fill = torch.tensor([3.0, -2.0, 5.0, -6.0])[(torch.arange(N * H * W).view(N, H, W, 1) + ci) % 4]
        x = fill.clone()
        x[:, 0:(self.Ho - 1) * s + 1:s, 0:(self.Wo - 1) * s + 1:s, :] = sel
        w = torch.zeros(Cout, Cin, K, K)
        co = torch.arange(Cout)
        w[co, co % Cin, p, p] = 1.0
        self.x, self.w = x.to(device), w.to(device)
        self.conv64 = sel[..., co % Cin].double().to(device)                          # (N, Ho, Wo, Cout)
        # residuals: zero on lap 0 of the even replicas of a band (those carry the coverage), small integers elsewhere;
        # res1 (rows that sweep stage 1) is zero too on the bands where an integer would not add exactly
        c = torch.arange(Cout).view(1, 1, 1, Cout)
        on = ((m // n + c // NB) % 2 == 1)
        r = torch.tensor(RES_VALUES, dtype=torch.float32)[(m + c) % len(RES_VALUES)] * on
        ok = torch.tensor([b[4] for b in BANDS])[c % NB]
        self.res2, self.res1 = r.to(device), (r * ok).to(device)
        self.res = self.res1
        self._packed = {}

    def with_res(self, sweep):
        """A shallow copy whose ``res`` is the residual of the rows that sweep stage ``sweep``."""
        o = object.__new__(Case)
        o.__dict__.update(self.__dict__)
        o.res = self.res1 if sweep == 1 else self.res2
        return o

    def weights(self, dtype):
        """(Cout, KH, KW, Cin), as the kernels read them."""
        if dtype not in self._packed:
            self._packed[dtype] = self.w.permute(0, 2, 3, 1).contiguous().to(dtype)
        return self._packed[dtype]

    def fwd64(self):
        """The float64 convolution computed the long way (for the check that ``conv64`` is the convolution)."""
        N, H, W, Cin, Cout, K, s, p = self.shape
        y = F.conv2d(self.x.double().permute(0, 3, 1, 2), self.w.double(), None, s, p)
        return y.permute(0, 2, 3, 1)


def band_affine(Cout, device):
    """(s, t) per channel of the swept stage: band c % NB, an integer offset b on the odd replicas of the first two."""
    s, t = torch.empty(Cout, dtype=torch.float64), torch.empty(Cout, dtype=torch.float64)
    for c in range(Cout):
        _, sign, j, base, _ = BANDS[c % NB]
        rep = c // NB
        b = (rep + 1) // 2 if (rep % 2 == 1 and c % NB < 2) else 0
        s[c] = sign * 2.0 ** -j
        t[c] = b * 2.0 ** -j + base if b else base          # (0 + -0 would lose the sign)
    assert bool(rep32(s).all()) and bool(rep32(t).all())
    return s.float().to(device), t.float().to(device)


def mild_affine(Cout, device):
    """(s, t) of the stage that is not swept: powers of two and small integers where the band stays exact under them,
    the identity elsewhere."""
    s, t = torch.ones(Cout), torch.zeros(Cout)
    for c in range(Cout):
        if BANDS[c % NB][4] and BANDS[c % NB][0] != 'at20':
            s[c] = [1.0, 0.5, 2.0][c % 3]
            t[c] = [0.0, 1.0, -1.0, 2.0][(c // NB) % 4]
    return s.to(device), t.to(device)


class Epi:
    """The descriptor side of a row on ``Cout`` channels: what tests/test_gpu_fwd_exact.py's Launch reads from an
    Epilogue (s1, t1, s2, t2, act1, act2, slope, slope2, two_stage)."""

    def __init__(self, row, Cout, device):
        self.row = row
        band, mild = band_affine(Cout, device), mild_affine(Cout, device)
        one, zero = torch.ones(Cout, device=device), torch.zeros(Cout, device=device)
        if row.sweep == 1:
            (self.s1, self.t1), (self.s2, self.t2) = band, mild
        else:
            (self.s1, self.t1), (self.s2, self.t2) = (one, zero), band
        self.act1, self.act2, self.slope, self.slope2 = row.act1, row.act2, row.slope1, row.slope2
        self.two_stage = row.two_stage


class Trace:
    """Float64 reference of a row on a convolution result, with the bound of the fp32 epilogue's error per element.
    ``v``: the argument of the swept activation.  Asserts what the construction promises: the first affine is exact,
    and for an exact row (or the swept stage-2 argument) the bound is zero."""

    def __init__(self, conv64, ep, res=None):
        row = ep.row
        zero = torch.zeros_like(conv64)
        prod = conv64 * ep.s1.double()
        p1 = prod + ep.t1.double()
        assert bool(rep32(prod).all()) and bool(rep32(p1).all()), 'k * s1 + t1 is not exact in fp32'
        y, err = _act_stage(p1, zero, row.act1, row.slope1)
        self.v = p1
        if row.residual:
            y = y + res.double()
            err = err + _round_err(y, err)
        if row.two_stage:
            u = y * ep.s2.double() + ep.t2.double()
            l2 = ep.s2.double().abs().log2()
            assert bool((l2 == l2.round()).all()), 's2 must be a power of two: then a multiply-and-add rounds like the fma'
            err = ep.s2.double().abs() * err
            err = err + _round_err(u, err)
            if row.sweep == 2:
                assert bool((err == 0).all()), 'the swept stage-2 argument is not exact in fp32'
                self.v = u
            y, err = _act_stage(u, err, row.act2, row.slope2)
        if row.exact:
            assert bool((err == 0).all()) and bool(rep32(y).all()), f'{row.name}: not exact'
        self.ref, self.bound = y, err


def coverage_gaps(v, odt, ref=None):
    """Names of the ranges of the issue's list that the swept arguments ``v`` (float64) miss; ``odt`` the output type."""
    v = v.reshape(-1)
    has = lambda m: bool(m.any())
    gaps = []
    checks = [
        ('v <= -104', v <= -104), ('[-104, -87.4]', (v >= -104) & (v <= -87.4)), ('[-87.4, -17]', (v >= -87.4) & (v <= -17)),
        ('[-17, -1]', (v >= -17) & (v <= -1)), ('[-1, 1]', (v >= -1) & (v <= 1)),
        ('+0', (v == 0) & ~torch.signbit(v)), ('-0', (v == 0) & torch.signbit(v)),
        ('0 < |v| <= 2^-20', (v != 0) & (v.abs() <= 2.0 ** -20)), ('[1, 8.7]', (v >= 1) & (v <= 8.7)),
        ('[8.7, 20)', (v >= 8.7) & (v < 20)), ('20', v == 20), ('20 - 2^-19', v == 20 - 2.0 ** -19),
        ('20 + 2^-19', v == 20 + 2.0 ** -19), ('(20, 30]', (v > 20) & (v <= 30)), ('>= 1e4', v >= 1e4),
    ]
    if odt == torch.float32:
        checks.append(('>= 1e30', v >= 1e30))
    if odt == torch.float16:
        checks.append(('result beyond 65504', (ref if ref is not None else v).reshape(-1) > 65504))
    for name, m in checks:
        if not has(m):
            gaps.append(name)
    return gaps


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def to_out(x64, odt, y_inv=1.0):
    """float64 -> fp32 -> the output type, as the kernels round (e4m3: times y_inv, clamped to +-448)."""
    x = x64.float()
    if odt == F8:
        return (x * y_inv).clamp(-448, 448).to(F8)
    return x.to(odt)


def worst_ulps(got, ref, where=None):
    """The largest |got - ref| in fp32 ulps of the reference (an fp32 ``got``), where |ref| >= 2**-100: below, the
    flushed exponentials and reciprocals (the bounds' floor terms) take over and an ulp count says nothing.  The count
    grows with |v| for negative v (the rounding of v * log2e is an absolute error of the exponent): ``where`` narrows it."""
    ok = torch.isfinite(ref) & (ref.abs() >= 2.0 ** -100) & (ref.abs() < 2.0 ** 127)
    if where is not None:
        ok = ok & where
    if not bool(ok.any()):
        return 0.0
    r = ref[ok]
    ulp = torch.exp2(torch.floor(torch.log2(r.abs())) - 23)
    return float(((got.double()[ok] - r).abs() / ulp).max())


def check(got, tr, odt, v=None, y_inv=1.0):
    """(ok, worst, v at worst, message): ``got`` (tensor of ``odt``) against the Trace ``tr``.  An exact row must equal the
    reference rounded once, bit for bit (the sign of a zero included; e4m3 has the clamp in between).  Otherwise got
    must lie in [round(ref - bound), round(ref + bound)].  ``worst``: for an fp32 output the largest err / bound; for a
    16-bit or e4m3 output, whose rounding hides the fp32 error, the fraction of outputs that are not the reference's own
    nearest code (each still inside the interval)."""
    ref, bound = tr.ref, tr.bound
    v = tr.v if v is None else v
    g64 = got.float().double()
    if tr.bound.max() == 0:
        want = to_out(ref, odt, y_inv)
        same = _bits(got) == _bits(want)
        if bool(same.all()):
            return True, 0.0, 0.0, ''
        i = int((~same).reshape(-1).nonzero()[0])
        return False, math.inf, float(v.reshape(-1)[i]), (
            f'{int((~same).sum())} of {same.numel()} differ; first at v = {float(v.reshape(-1)[i])!r}: got '
            f'{float(g64.reshape(-1)[i])!r}, want {float(want.float().reshape(-1)[i])!r}')
    lo, hi = to_out(ref - bound, odt, y_inv).float().double(), to_out(ref + bound, odt, y_inv).float().double()
    inside = (g64 >= lo) & (g64 <= hi)                      # a NaN is outside
    if odt == torch.float32:
        dev = (g64 - ref).abs()
        inside = dev <= bound                               # the bound itself, not its ends rounded to fp32
        ratio = torch.where(dev == 0, torch.zeros_like(dev), dev / bound)
    else:       # the fp32 error is hidden behind the rounding: report how many outputs are not the reference's own code
        near = to_out(ref, odt, y_inv).float().double()
        off = (g64 != near) & ~(torch.isnan(g64) & torch.isnan(near))
        ratio = off.double() * float(off.double().mean())
    ratio = torch.where(inside, ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.reshape(-1).argmax())
    worst, at = float(ratio.reshape(-1)[i]), float(v.reshape(-1)[i])
    if bool(inside.all()):
        return True, worst, at, ''
    return False, worst, at, (f'{int((~inside).sum())} of {inside.numel()} outside the bound; first at v = {at!r}: got '
                              f'{float(g64.reshape(-1)[i])!r}, allowed [{float(lo.reshape(-1)[i])!r}, '
                              f'{float(hi.reshape(-1)[i])!r}] (ref {float(ref.reshape(-1)[i])!r})')
