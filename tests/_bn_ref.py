"""Float64 reference of the train-mode BatchNorm + activation passes, with a first-order error scale for every output
(a helper module for the tests, not a conftest).

The operation (bn_train.hip's header, darknetcsp.py's Conv: conv -> BatchNorm2d -> activation, plus the shortcut) on an NHWC
view of M rows and C channels:

  statistics   s1 = sum x, s2 = sum x^2, mean = s1 / M, var = max(s2 / M - mean^2, 0) (biased),
               invstd = 1 / sqrt(var + fp32(eps)); running statistics take the unbiased variance var * M / (M - 1)
  forward      xhat = (x - mean) * invstd, z = xhat * gamma + beta, y = act(z) (+ residual)
  backward     g = dy * act'(z), dbeta = sum g, dgamma = sum g * xhat,
               dx = gamma * invstd * (g - dbeta / M_total - xhat * dgamma / M_total);  eval mode: dx = gamma * invstd * g
  SyncBN       a rank reduces its own rows (local dgamma / dbeta); dx takes the totals over all ranks' M_total rows

Everything is evaluated on the very values a kernel reads: the fp32 / bf16 / fp16 tensors converted exactly, and the
fp32 mean / invstd / gamma / beta where an entry point takes them as inputs.  ``dt=torch.float32`` evaluates the same
textbook expressions in fp32 with torch's own sums; its distance from float64 in units of the scale is ``K32``.

Scales.  Every fp32 rounding is taken as one u = 2**-24 relative to the magnitude it acts on, and every magnitude is
bounded by a sum of absolute values, so the scale of an output is what one rounding of each of its terms can move it by:

  amp      = (|x| + |mean|) * invstd           bounds |xhat| and one rounding of x - mean
  Sz       = amp * |gamma| + |beta|            bounds |z| and its roundings
  S_y      = |y| + Sz (+ |res|)                |act'| <= 1.09 for all four activations: z's error passes through unscaled
  S_g      = |dy| * (1 + Sz)                   act' is O(1), and |act''| <= 1 turns z's error into an error of act'
  S_dbeta  = sum S_g
  S_dgamma = sum |dy| * ((1 + Sz) * |xhat| + amp)       g's error times |xhat|, plus |g| <= 1.09 |dy| times xhat's error
  S_dx     = |gamma invstd| * (S_g + (|dbeta| + S_dbeta) / M + (|xhat| + amp) * (|dgamma| + S_dgamma) / M)
             (the sums enter dx with their OWN errors, hence S_dbeta / M and S_dgamma / M beside the values: where dbeta
             cancels to nothing the value alone would under-scale the term)
  S_mean   = mean |x|
  S_var    = mean x^2 + 2 |mean| mean |x|      var = s2 / M - mean^2: the error of mean enters through 2 |mean| d(mean)
  S_invstd = invstd^3 / 2 * S_var + invstd     d invstd = -invstd^3 / 2 d var, and its own last rounding

No scale is computed from a kernel's output.
"""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_MISH, ACT_LEAKY, ACT_SWISH = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: 'none', ACT_MISH: 'mish', ACT_LEAKY: 'leaky', ACT_SWISH: 'swish'}
U = 2.0 ** -24
F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
_CHUNK_ELEMS = 1 << 25         # elements per row chunk of a reference (256 MB in float64)
AMBIGUOUS_U = 8                # Leaky: |z| within 8 u Sz of zero has no defined sign in an fp32 evaluation


def f32(v):
    """The value a C ``float`` argument carries, as a Python float."""
    return float(torch.tensor(v, dtype=F32))


def row_step(C):
    return max(1, _CHUNK_ELEMS // max(1, C))


# ---------------------------------------------------------------------------------------------------------------------
# activations (any floating dtype)
# ---------------------------------------------------------------------------------------------------------------------
def softplus(z):
    return z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))


def act_fwd(z, act, slope):
    if act == ACT_MISH:
        return z * torch.tanh(softplus(z))
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * slope)
    if act == ACT_SWISH:
        return z * torch.sigmoid(z)
    return z


def act_grad(z, act, slope):
    """d act / d z; Leaky in torch's convention (leaky_relu_backward: ``x > 0``), which gives ``slope`` AT zero."""
    if act == ACT_MISH:
        t = torch.tanh(softplus(z))
        return t + z * (1 - t * t) * torch.sigmoid(z)
    if act == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if act == ACT_SWISH:
        s = torch.sigmoid(z)
        return s + z * s * (1 - s)
    return torch.ones_like(z)


# ---------------------------------------------------------------------------------------------------------------------
# the passes
# ---------------------------------------------------------------------------------------------------------------------
def stats(x, eps, dt=F64):
    """Per-channel statistics of x (M, C) and their scales (module docstring)."""
    M, C = x.shape
    s1 = torch.zeros(C, dtype=dt, device=x.device)
    s2, sa = s1.clone(), s1.clone()
    step = row_step(C)
    for r0 in range(0, M, step):
        xc = x[r0:r0 + step].to(dt)
        s1 += xc.sum(0)
        s2 += (xc * xc).sum(0)
        sa += xc.abs().sum(0)
    mean = s1 / M
    var = (s2 / M - mean * mean).clamp_min(0)
    invstd = 1 / torch.sqrt(var + torch.tensor(eps, dtype=F32).to(dt))
    S_var = s2 / M + 2 * mean.abs() * sa / M
    return dict(sum=s1, sumsq=s2, mean=mean, var=var, invstd=invstd, S_mean=sa / M, S_var=S_var,
                S_invstd=invstd ** 3 / 2 * S_var + invstd)


def running(rm0, rv0, mean, var, M_total, momentum):
    """The running statistics after one update: unbiased variance over M_total rows, fp32(momentum)."""
    mom = f32(momentum)
    unbiased = var * M_total / (M_total - 1) if M_total > 1 else var
    return (1.0 - mom) * rm0.double() + mom * mean, (1.0 - mom) * rv0.double() + mom * unbiased


class _Chan:
    """The per-channel inputs of a pass in the evaluation dtype."""

    def __init__(self, mean, invstd, gamma, beta, dt):
        self.m, self.i, self.g, self.b = (t.to(dt) for t in (mean, invstd, gamma, beta))

    def z(self, x):
        xhat = (x - self.m) * self.i
        return xhat, xhat * self.g + self.b

    def scales(self, x):
        amp = (x.abs() + self.m.abs()) * self.i
        return amp, amp * self.g.abs() + self.b.abs()


def forward(x, mean, invstd, gamma, beta, act, slope, res=None, dt=F64, want_scale=True):
    """y and S_y of rows x (m, C) (and res, same shape).  Callers with large maps pass row slices."""
    ch = _Chan(mean, invstd, gamma, beta, dt)
    xd = x.to(dt)
    _, z = ch.z(xd)
    y = act_fwd(z, act, slope)
    if res is not None:
        y = y + res.to(dt)
    if not want_scale:
        return y, None
    _, Sz = ch.scales(xd)
    S = y.abs() + Sz
    if res is not None:
        S = S + res.to(dt).abs()
    return y, S


def backward_sums(x, dy, mean, invstd, gamma, beta, act, slope, dt=F64):
    """dbeta, dgamma of the rows given and their scales, summed a chunk of rows at a time."""
    M, C = x.shape
    ch = _Chan(mean, invstd, gamma, beta, dt)
    out = {k: torch.zeros(C, dtype=dt, device=x.device) for k in ('dbeta', 'dgamma', 'S_dbeta', 'S_dgamma')}
    step = row_step(C)
    for r0 in range(0, M, step):
        xd, dyd = x[r0:r0 + step].to(dt), dy[r0:r0 + step].to(dt)
        xhat, z = ch.z(xd)
        g = dyd * act_grad(z, act, slope)
        out['dbeta'] += g.sum(0)
        out['dgamma'] += (g * xhat).sum(0)
        amp, Sz = ch.scales(xd)
        out['S_dbeta'] += (dyd.abs() * (1 + Sz)).sum(0)
        out['S_dgamma'] += (dyd.abs() * ((1 + Sz) * xhat.abs() + amp)).sum(0)
    return out


def backward_dx(x, dy, mean, invstd, gamma, beta, act, slope, sums, M_total, eval_mode=False, dt=F64, want_scale=True):
    """dx and S_dx of rows x, dy (m, C) given the sums over all M_total rows (``backward_sums``; ignored in eval mode)."""
    ch = _Chan(mean, invstd, gamma, beta, dt)
    xd, dyd = x.to(dt), dy.to(dt)
    xhat, z = ch.z(xd)
    g = dyd * act_grad(z, act, slope)
    k1 = ch.g * ch.i
    if eval_mode:
        dx = k1 * g
    else:
        dx = k1 * (g - sums['dbeta'].to(dt) / M_total - xhat * (sums['dgamma'].to(dt) / M_total))
    if not want_scale:
        return dx, None
    amp, Sz = ch.scales(xd)
    S = dyd.abs() * (1 + Sz)
    if not eval_mode:
        S = S + (sums['dbeta'].abs() + sums['S_dbeta']) / M_total \
            + (xhat.abs() + amp) * (sums['dgamma'].abs() + sums['S_dgamma']) / M_total
    return dx, k1.abs() * S


# ---------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------
def half_ulp(ref64, dtype):
    """Half a unit in the last place of ``dtype`` at |ref64| (what one rounding of the exact value to a 16-bit output can
    add); 0 for fp32, whose last rounding the scale already counts."""
    if dtype == F32:
        return torch.zeros_like(ref64)
    _, e = torch.frexp(ref64.abs().clamp_min(1e-300))          # |v| = m 2^e, m in [0.5, 1)
    e = e.double() - 1
    if dtype == BF16:
        return torch.exp2(e.clamp_min(-126) - 7) / 2
    return torch.exp2(e.clamp_min(-14) - 10) / 2


def k_of(got, ref64, S, dtype=F32):
    """max_i |got_i - ref64_i| / (u S_i + h_i), every element counted; a non-finite or misplaced value gives inf.
    Returns (K, flat index of the worst element)."""
    got = got.to(ref64.device).double()
    err = (got - ref64).abs()
    den = U * S + half_ulp(ref64, dtype)
    k = torch.where(den > 0, err / den, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    k = torch.nan_to_num(k, nan=float('inf'), posinf=float('inf'))
    if k.numel() == 0:
        return 0.0, 0
    i = int(k.argmax())
    return float(k.flatten()[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """Inputs of one comparison: x, dy, res (M, C) in ``dtype``; gamma, beta fp32; mean / invstd are the float64
    statistics of x rounded to fp32 -- what the forward and backward entry points are handed.  ``claims`` are
    (description, bool) pairs a generator fills in: what the input was built to contain."""

    def __init__(self, name, dtype, x, dy, res, gamma, beta, eps=1e-3):
        self.name, self.dtype, self.x, self.dy, self.res = name, dtype, x, dy, res
        self.gamma, self.beta, self.eps = gamma.float(), beta.float(), eps
        self.M, self.C = x.shape
        self.claims = []
        self.restat()

    def restat(self):
        self.st = stats(self.x, self.eps)
        self.mean, self.invstd = self.st['mean'].float(), self.st['invstd'].float()

    def z64(self):
        ch = _Chan(self.mean, self.invstd, self.gamma, self.beta, F64)
        return ch.z(self.x.double())[1], ch.scales(self.x.double())[1]

    def ratio(self):
        """mean / std per channel (biased std of the values as stored)."""
        return self.st['mean'].abs() / torch.sqrt(self.st['var']).clamp_min(1e-300)

    def claim(self, what, ok):
        self.claims.append((what, bool(ok)))

    def check_claims(self):
        bad = [w for w, ok in self.claims if not ok]
        assert not bad, f'{self.name} ({self.dtype}): the input does not contain: {bad}'
        assert self.claims, f'{self.name}: no claims'
        for t in (self.x, self.dy, self.res):
            assert bool(torch.isfinite(t.float()).all()), f'{self.name}: non-finite input'


def _randn(shape, seed, device):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F32).to(device)


def _base(name, dtype, xf, seed, device, gamma=None, beta=None, dy_scale=1.0):
    M, C = xf.shape
    g = torch.Generator(device='cpu').manual_seed(seed + 7)
    if gamma is None:
        gamma = torch.empty(C).uniform_(0.5, 1.5, generator=g)
    if beta is None:
        beta = torch.randn(C, generator=g) * 0.3
    dy = (_randn((M, C), seed + 1, device) * dy_scale).to(dtype)
    res = _randn((M, C), seed + 2, device).to(dtype)
    return Case(name, dtype, xf.to(dtype), dy, res, gamma.to(device), beta.to(device))


def gen_usual(dtype, M, C, seed, device):
    """randn * 1.5 + 0.3, gamma in [0.5, 1.5], beta ~ 0.3 randn: what every earlier test used."""
    c = _base('usual', dtype, _randn((M, C), seed, device) * 1.5 + 0.3, seed, device)
    c.claim('mean/std below 1 on every channel', c.ratio().max() < 1)
    return c


def gen_ratio(ratio, dtype, M, C, seed, device):
    """Unit-variance channels around a mean of 1.1 x ``ratio`` (alternating sign): mean/std >= ratio as stored."""
    sign = torch.where(torch.arange(C, device=device) % 2 == 0, 1.0, -1.0)
    c = _base(f'ratio{ratio}', dtype, _randn((M, C), seed, device) + 1.1 * ratio * sign, seed, device)
    c.claim(f'mean/std >= {ratio} on every channel', c.ratio().min() >= ratio)
    c.claim('the type resolves the spread (std as stored within 2x of 1)',
            0.5 < float(torch.sqrt(c.st['var']).min()) and float(torch.sqrt(c.st['var']).max()) < 2)
    return c


def ratios_for(dtype):
    """The mean/std ladder as far as the type resolves a unit spread around the mean (bf16 steps by 8 at 1100)."""
    return [10, 100] if dtype == BF16 else [10, 100, 1000]


def gen_const_channel(dtype, M, C, seed, device):
    """Channels 1 and C - 2 hold one value in every row (0.3 as the type stores it, and -17): var = 0 in float64, while
    an fp32 sum of squares may land on either side of mean^2 (the var < 0 clamp)."""
    xf = _randn((M, C), seed, device) * 1.5 + 0.3
    xf[:, 1] = 0.3
    xf[:, C - 2] = -17.0
    c = _base('const_channel', dtype, xf, seed, device)
    c.claim('var == 0 in float64 on the constant channels', c.st['var'][1] == 0 and c.st['var'][C - 2] == 0)
    c.claim('invstd == 1/sqrt(eps) there', abs(float(c.invstd[1]) - f32(1e-3) ** -0.5) < 1e-4)
    return c


def gen_tiny_std(dtype, M, C, seed, device):
    """A spread far below sqrt(eps) around 0.5: eps rules invstd, xhat stays small."""
    std = 1e-3 if dtype == F32 else 2.0 ** -6
    c = _base('tiny_std', dtype, _randn((M, C), seed, device) * std + 0.5, seed, device)
    sd = torch.sqrt(c.st['var'])
    c.claim('0 < std <= 1.5 x the nominal one', float(sd.min()) > 0 and float(sd.max()) <= 1.5 * std)
    c.claim('var below eps', float(c.st['var'].max()) < c.eps)
    return c


def gen_big_gamma(dtype, M, C, seed, device):
    """gamma = 6 (even channels) and 25 (odd): z spans both Mish asymptotes -- beyond +-20 (the asymptote selects and
    exponent clamps) and beyond +-45 (n = e (e + 2) overflows fp32 from z = 44.4 on; 1 - u cancels completely below)."""
    gamma = torch.where(torch.arange(C) % 2 == 0, 6.0, 25.0)
    c = _base('big_gamma', dtype, _randn((M, C), seed, device) * 1.5 + 0.3, seed, device, gamma=gamma)
    z, _ = c.z64()
    for lo, hi in ((20, 45), (45, 1e9)):
        c.claim(f'z in ({lo}, {hi})', ((z > lo) & (z < hi)).any())
        c.claim(f'z in (-{hi}, -{lo})', ((z < -lo) & (z > -hi)).any())
    c.claim('|z| < 1 as well', (z.abs() < 1).any())
    return c


def gen_huge_gamma(dtype, M, C, seed, device):
    """gamma = 1e24 / 1e-24 / -1e24 by channel: z up to 1e24 (z * a * e overflows fp32 above z = 1.4e21 unless z is the
    clamped one) and denormal-small products; dy is scaled down so that dx stays in range."""
    gamma = torch.tensor([1e24, 1e-24, -1e24, 1.0])[torch.arange(C) % 4]
    c = _base('huge_gamma', dtype, _randn((M, C), seed, device) * 1.5 + 0.3, seed, device, gamma=gamma, dy_scale=2.0 ** -40)
    z, _ = c.z64()
    c.claim('z beyond +-1e22', (z > 1e22).any() and (z < -1e22).any())
    return c


def gen_gamma_signs(dtype, M, C, seed, device):
    """gamma = 0 on channels 0 mod 3, negative on 1 mod 3; beta = 0 on the first gamma = 0 channel."""
    g = torch.Generator(device='cpu').manual_seed(seed + 9)
    gamma = torch.empty(C).uniform_(0.5, 1.5, generator=g)
    gamma[0::3] = 0.0
    gamma[1::3] *= -1.0
    beta = torch.randn(C, generator=g) * 0.3
    beta[0] = 0.0
    c = _base('gamma_signs', dtype, _randn((M, C), seed, device) * 1.5 + 0.3, seed, device, gamma=gamma, beta=beta)
    c.claim('gamma == 0, gamma < 0 and gamma > 0 channels', (c.gamma == 0).any() and (c.gamma < 0).any() and (c.gamma > 0).any())
    c.claim('a channel with gamma == 0 and beta == 0', ((c.gamma == 0) & (c.beta == 0)).any())
    return c


def gen_fp16_range(M, C, seed, device):
    """fp16 values up to the type's largest (65504) and denormals (below 6.1e-5) in one map; gamma = 1/64 on the wide
    channels keeps y = O(|xhat|) in range."""
    xf = _randn((M, C), seed, device)
    xf[:, 0::2] *= 16000.0
    xf[:, 1::2] *= 2.0 ** -16
    xf[0, 0], xf[1, 0], xf[2, 1] = 65504.0, -65504.0, 2.0 ** -24
    c = _base('fp16_range', F16, xf.clamp(-65504.0, 65504.0), seed, device)
    c.claim('the largest fp16 value of both signs', c.x.max() == 65504 and c.x.min() == -65504)
    c.claim('fp16 denormals', ((c.x.float().abs() < 2.0 ** -14) & (c.x != 0)).any())
    return c


def gen_leaky_zero(dtype, M, C, seed, device):
    """Leaky with z == 0 exactly: channels 0 mod 4 hold integers from {-2, -1, 0, 0, 1, 2} in equal numbers (so the mean
    is exactly 0 in any arithmetic), with beta = 0 -- z = (0 - 0) * invstd * gamma + 0 is zero in fp32 and in float64
    alike.  M must be a multiple of 6."""
    assert M % 6 == 0
    xf = _randn((M, C), seed, device) * 1.5 + 0.3
    pat = torch.tensor([-2.0, -1.0, 0.0, 0.0, 1.0, 2.0], device=device).repeat(M // 6)
    g = torch.Generator(device='cpu').manual_seed(seed + 11)
    for ch in range(0, C, 4):
        xf[:, ch] = pat[torch.randperm(M, generator=g).to(device)]
    gb = torch.Generator(device='cpu').manual_seed(seed + 12)
    beta = torch.randn(C, generator=gb) * 0.3
    beta[0::4] = 0.0
    c = _base('leaky_zero', dtype, xf, seed, device, beta=beta)
    z, Sz = c.z64()
    c.claim('mean exactly 0 on the built channels', (c.st['mean'][0::4] == 0).all() and (c.mean[0::4] == 0).all())
    c.claim('z == 0 exactly on a third of their rows', int((z[:, 0::4] == 0).sum()) == (M // 3) * len(range(0, C, 4)))
    c.claim('with Sz == 0 there (no rounding can move it)', (Sz[:, 0::4][z[:, 0::4] == 0] == 0).all())
    return c


def ambiguous(case):
    """Elements whose sign of z an fp32 evaluation cannot be held to: |z64| <= 8 u Sz, except where Sz == 0 (every term
    of z is exactly zero: z is zero in any arithmetic)."""
    z, Sz = case.z64()
    return (z.abs() <= AMBIGUOUS_U * U * Sz) & (Sz > 0)


def settle_leaky(case, rounds=20):
    """Move the ambiguous elements of a Leaky case away from zero (by four widths of their band, or one step of the type
    if that is larger), re-derive the statistics, and repeat until none remain.  Nothing is excluded afterwards."""
    for _ in range(rounds):
        amb = ambiguous(case)
        if not bool(amb.any()):
            break
        z, Sz = case.z64()
        slope_x = (case.invstd.double() * case.gamma.double()).expand_as(z)          # dz / dx
        xd = case.x.double()
        step = 4 * AMBIGUOUS_U * U * Sz / slope_x.abs().clamp_min(1e-300)
        ulp = 4 * half_ulp(xd, case.dtype) if case.dtype != F32 else xd.abs().clamp_min(2.0 ** -126) * 2.0 ** -22
        direction = torch.where(z >= 0, 1.0, -1.0) * torch.where(slope_x >= 0, 1.0, -1.0)
        moved = (xd + direction * torch.maximum(step, ulp)).to(case.dtype)
        case.x = torch.where(amb & (slope_x != 0), moved, case.x)
        case.restat()
    n = int(ambiguous(case).sum())
    assert n == 0, f'{case.name}: {n} elements still within {AMBIGUOUS_U} u Sz of z = 0'
    case.claim('no element within 8 u Sz of z = 0', True)
    return case


# ---------------------------------------------------------------------------------------------------------------------
# self-check
# ---------------------------------------------------------------------------------------------------------------------
def torch_reference(x, dy, gamma, beta, eps, act, slope, res=None, eval_stats=None):
    """torch.nn.functional.batch_norm + torch's activations + autograd in float64: y, dx, dgamma, dbeta (, dres)."""
    x = x.double().clone().requires_grad_(True)
    ga, be = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    xn = x.t().unsqueeze(0)                                        # (1, C, M)
    if eval_stats is None:
        z = F.batch_norm(xn, None, None, ga, be, True, 0.0, f32(eps))
    else:
        z = F.batch_norm(xn, eval_stats[0].double(), eval_stats[1].double(), ga, be, False, 0.0, f32(eps))
    z = z.squeeze(0).t()
    y = {ACT_NONE: lambda t: t, ACT_MISH: F.mish, ACT_LEAKY: lambda t: F.leaky_relu(t, slope), ACT_SWISH: F.silu}[act](z)
    if res is not None:
        y = y + res.double()
    y.backward(dy.double())
    return y.detach(), x.grad, ga.grad, be.grad


def check_refs_cpu():
    """The reference against torch in float64 on the CPU: every activation with a residual in train mode, one in eval
    mode, and Leaky AT zero.  (tests/test_bn_ref_host.py holds the full set.)"""
    M, C = 61, 8
    x, dy, res = (_randn((M, C), s, 'cpu') for s in (1, 2, 3))
    gamma, beta = torch.linspace(-1.5, 1.5, C), torch.linspace(-0.4, 0.4, C)
    slope = f32(0.1)
    st = stats(x, 1e-3)
    for act in ACT_NAMES:
        want = torch_reference(x, dy, gamma, beta, 1e-3, act, slope, res)
        y, _ = forward(x, st['mean'], st['invstd'], gamma, beta, act, slope, res)
        sums = backward_sums(x, dy, st['mean'], st['invstd'], gamma, beta, act, slope)
        dx, _ = backward_dx(x, dy, st['mean'], st['invstd'], gamma, beta, act, slope, sums, M)
        for name, a, b in zip(('y', 'dx', 'dgamma', 'dbeta'), (y, dx, sums['dgamma'], sums['dbeta']), want):
            assert float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max())), (ACT_NAMES[act], name)
    z0 = torch.zeros(1, dtype=F64)
    assert float(act_grad(z0, ACT_LEAKY, slope)) == slope and float(act_grad(-z0, ACT_LEAKY, slope)) == slope
