"""The optimizer-side kernels (csrc/optim.hip: yv4_grad_prepare, yv4_sgd_step, yv4_ema_update) through the C ABI on raw
tensors, bit for bit against a float64 restatement.

Exact operands: parameters, gradients, momentum and EMA values are small integers; lr, momentum and weight decay are
powers of two (or zero) and so is the gradient multiplier ``ctrl[0]``.  Every product and sum of the update is then a
multiple of 2**-11 below 16 -- 15 significant bits -- so each fp32 operation is exact, fused or not, and the float64
restatement (which asserts that every intermediate survives a round trip through fp32) must be matched bit for bit.
Every segment of a hyper-parameter table gets a row that differs from its neighbours' in lr, momentum, weight decay
and Nesterov flag, so a lookup that is off by one segment changes four floats.  The squares of integer gradients sum
exactly in double in any order, which pins the sum of squares, its deterministic per-workgroup slots and the norm.

Grid caps (optim.hip): ``stream_grid`` launches at most 4096 workgroups of 256 threads, one 16-byte word per thread and
trip; ``sumsq_kernel`` at most 2048 workgroups with four words per thread and trip.  The large cases pass them.

Every arena sits inside a larger allocation filled with a canary, and nothing beyond ``n`` floats may change.
"""
import contextlib

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib, ops

pytestmark = pytest.mark.gpu

OK, E_INVALID = 0, -1
PAD = 64
CANARY = 12345.0
SGD_TRIP = 4096 * 256            # 16-byte words per trip of sgd_step_kernel / ema_kernel at the capped grid
SUMSQ_TRIP = 2048 * 256 * 4      # ... of sumsq_kernel
MAX_SEG = 4096


@contextlib.contextmanager
def det_mode(on):
    was = pkg.deterministic()
    pkg.set_deterministic(on)
    try:
        yield
    finally:
        pkg.set_deterministic(was)


def status(st, what):
    return f'{what}: status {st}: ' + _lib.lib().yv4_last_error().decode('utf-8', 'replace')


def ints(n, seed, amp=4):
    """n integers from [-amp, amp] as fp32 (CPU, seeded)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (n,), generator=g, dtype=torch.int32).float()


class Arena:
    """``values`` (fp32 or fp64, CPU) on the device with PAD canary elements in front and behind."""

    def __init__(self, values, dev):
        n = values.numel()
        self.n = n
        self.whole = torch.full((n + 2 * PAD,), CANARY, dtype=values.dtype, device=dev)
        self.t = self.whole[PAD:PAD + n]
        self.t.copy_(values)
        self.snap = self.whole.clone()

    def ptr(self):
        assert self.t.data_ptr() % 16 == 0
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu()

    def assert_pads_intact(self, what):
        i32 = lambda t: t.view(torch.int32)
        assert torch.equal(i32(self.whole[:PAD]), i32(self.snap[:PAD])) and \
            torch.equal(i32(self.whole[PAD + self.n:]), i32(self.snap[PAD + self.n:])), f'{what}: written outside the arena'

    def assert_unchanged(self, what):
        assert torch.equal(self.whole.view(torch.int32), self.snap.view(torch.int32)), f'{what}: changed'


def exact32(t, what):
    assert torch.equal(t.float().double(), t), f'{what} is not exact in fp32: the case is not an exact one'
    return t


# ---- yv4_sgd_step ----------------------------------------------------------------------------------------------------
LRS = [2.0 ** -1, 2.0 ** -3, 2.0 ** -2, 2.0 ** -4]
MOMS = [2.0 ** -1, 0.0, 2.0 ** -2]
WDS = [2.0 ** -3, 2.0 ** -5, 0.0, 2.0 ** -4, 2.0 ** -2]
NESTEROV = [1.0, 0.0]


def hyper_rows(nseg):
    """Row s = (lr, momentum, weight decay, nesterov) cycling with periods 4, 3, 5 and 2: neighbouring rows differ in
    every column, and momentum = 0, wd = 0 and both Nesterov settings all occur."""
    return torch.tensor([[LRS[s % 4], MOMS[s % 3], WDS[s % 5], NESTEROV[s % 2]] for s in range(nseg)], dtype=torch.float32)


def sgd_ref(p, g, b, lens, hyper, mul, exact=True):
    """float64 restatement of the update, element by element; returns (p, b)."""
    lens = torch.tensor(lens, dtype=torch.int64)
    lr, mom, wd, nes = (torch.repeat_interleave(hyper[:, k], lens).double() for k in range(4))
    chk = exact32 if exact else (lambda t, what: t)
    p, g, b = p.double(), g.double(), b.double()
    gr = chk(chk(g * mul, 'g * ctrl[0]') + chk(wd * p, 'wd * p'), 'gr')
    nb = chk(chk(mom * b, 'mom * b') + gr, 'b')
    step = torch.where(nes != 0, chk(gr + chk(mom * nb, 'mom * b_new'), 'nesterov step'), nb)
    return chk(p - chk(lr * step, 'lr * step'), 'p'), nb


def run_sgd(dev, p, g, b, lens, hyper, ctrl=None, nseg=None, n=None):
    """One yv4_sgd_step.  ``ctrl``: None or 4 floats.  Returns (status, p arena, b arena) after asserting that the
    gradient and everything around the arenas kept its bits."""
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    P_, G_, B_ = Arena(p, dev), Arena(g, dev), Arena(b, dev)
    H_ = hyper.to(dev).contiguous()
    C_ = torch.tensor(ctrl, dtype=torch.float32, device=dev) if ctrl is not None else None
    st = _lib.lib().yv4_sgd_step(P_.ptr(), G_.ptr(), B_.ptr(), int(off[-1]) if n is None else n, off.data_ptr(),
                                 H_.data_ptr(), len(lens) if nseg is None else nseg,
                                 C_.data_ptr() if C_ is not None else None, ops.stream_ptr())
    torch.cuda.synchronize()
    G_.assert_unchanged('sgd_step gradient')
    P_.assert_pads_intact('sgd_step parameters'), B_.assert_pads_intact('sgd_step momentum')
    return st, P_, B_


def assert_bits(got, ref64, what):
    want = ref64.float()
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().view(-1)
    i = int(bad[0])
    raise AssertionError(f'{what}: {bad.numel()} of {got.numel()} floats differ; first at {i} (word {i // 4}): got '
                         f'{float(got[i])!r}, want {float(want[i])!r}')


TABLES = {
    'one': [4000],
    'two_inside_a_workgroup': [400, 2400],
    'two_on_a_workgroup_edge': [1024, 2048],                    # 256 threads x 4 floats = 1024 floats per workgroup
    'fours': [4] * 300,
    'empty_at_start_middle_end': [0, 0, 12, 0, 4, 0, 0, 1008, 8, 1024, 0],
    'max_4096': [(4, 8, 4, 0, 12, 4)[s % 6] for s in range(MAX_SEG)],
}


@pytest.mark.parametrize('ctrl', [None, 0.25, 1.0], ids=['noctrl', 'mul0.25', 'mul1'])
@pytest.mark.parametrize('table', list(TABLES), ids=list(TABLES))
def test_sgd_step_segment_tables(gpu_device, table, ctrl):
    """Tables of 1, 2 and 4096 segments, segments of exactly 4 floats, empty segments (repeated offsets) at the start,
    in the middle and at the end, boundaries inside a workgroup and on a workgroup edge; momentum = 0, wd = 0 and both
    Nesterov settings occur in the rows; with and without ``ctrl``.  The allocation is longer than seg_off[nseg]."""
    lens = TABLES[table]
    n = sum(lens)
    p, g, b = ints(n, 1), ints(n, 2), ints(n, 3)
    hyper = hyper_rows(len(lens))
    rp, rb = sgd_ref(p, g, b, lens, hyper, 1.0 if ctrl is None else ctrl)
    st, P_, B_ = run_sgd(gpu_device, p, g, b, lens, hyper, None if ctrl is None else [ctrl, 99.0, 0.0, 77.0])
    assert st == OK, status(st, table)
    assert_bits(P_.cpu(), rp, f'{table}: parameters')
    assert_bits(B_.cpu(), rb, f'{table}: momentum')
    assert not torch.equal(rp.float(), p)


def test_sgd_step_refuses_bad_tables(gpu_device):
    """4097 segments, no segment, and a length that is no multiple of 4: YV4_E_INVALID, nothing written."""
    lens = [4] * (MAX_SEG + 1)
    n = sum(lens)
    p, g, b = ints(n, 1), ints(n, 2), ints(n, 3)
    for what, kw in {'4097 segments': {}, 'no segment': dict(nseg=0), 'n % 4': dict(nseg=8, n=30)}.items():
        st, P_, B_ = run_sgd(gpu_device, p, g, b, lens, hyper_rows(len(lens)), **kw)
        assert st == E_INVALID, status(st, what)
        P_.assert_unchanged(what), B_.assert_unchanged(what)
    st, P_, _ = run_sgd(gpu_device, p, g, b, lens[:MAX_SEG], hyper_rows(MAX_SEG))
    assert st == OK, status(st, '4096 segments of the same table')


def test_sgd_step_takes_a_second_grid_stride_trip(gpu_device):
    """n / 4 = 2 * 4096 * 256 + 777 words: two full trips of the capped grid and a ragged third, with segment boundaries
    on the trip edges, one word to either side of them and inside the tail."""
    n4 = 2 * SGD_TRIP + 777
    cuts = [0, 4 * 1000, 4 * (SGD_TRIP - 1), 4 * SGD_TRIP, 4 * (SGD_TRIP + 1), 4 * (2 * SGD_TRIP), 4 * (2 * SGD_TRIP + 300),
            4 * n4]
    lens = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    n = 4 * n4
    p, g, b = ints(n, 4), ints(n, 5), ints(n, 6)
    hyper = hyper_rows(len(lens))
    rp, rb = sgd_ref(p, g, b, lens, hyper, 0.5)
    st, P_, B_ = run_sgd(gpu_device, p, g, b, lens, hyper, [0.5, 0.0, 0.0, 0.0])
    assert st == OK, status(st, 'second trip')
    assert_bits(P_.cpu(), rp, 'second trip: parameters')
    assert_bits(B_.cpu(), rb, 'second trip: momentum')


def test_sgd_step_skipped_step_keeps_every_bit(gpu_device):
    """ctrl[2] = 1 (non-finite gradients found): parameters and momentum keep every bit, whatever the gradients hold."""
    lens = TABLES['empty_at_start_middle_end']
    n = sum(lens)
    p, g, b = ints(n, 1), ints(n, 2), ints(n, 3)
    g[5], g[n - 1] = float('inf'), float('nan')
    p[7], b[9] = -0.0, -0.0
    st, P_, B_ = run_sgd(gpu_device, p, g, b, lens, hyper_rows(len(lens)), [0.25, 3.0, 1.0, 0.25])
    assert st == OK, status(st, 'skipped step')
    P_.assert_unchanged('skipped step: parameters'), B_.assert_unchanged('skipped step: momentum')


def rel_err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def assert_within_reference_error(got, cpu32, ref64, what):
    """DESIGN.md 4.7's bound: e(kernel) <= 4 * e32 + 8 * 2**-24 with e(x) = max |x - ref64| / max |ref64| and e32 the
    measure of torch's own fp32 evaluation on the CPU.  It comes from the reference, not from the kernel."""
    e32, ek = rel_err(cpu32, ref64), rel_err(got, ref64)
    bound = 4 * e32 + 8 * 2.0 ** -24
    print(f'{what}: e32 = {e32:.3e}, e(kernel) = {ek:.3e}, bound = {bound:.3e}')
    assert ek <= bound, f'{what}: e(kernel) = {ek:.3e} above 4 * e32 + 8 * 2**-24 = {bound:.3e} (e32 = {e32:.3e})'


def test_sgd_step_recipe_values_against_float64(gpu_device):
    """Real operands at the recipe's lr = 0.01, momentum = 0.937, weight decay = 5e-4, Nesterov, and a second segment
    without decay (the biases' group), gradient multiplier 1 / 1024 * 0.7."""
    g_ = torch.Generator().manual_seed(7)
    lens = [6000, 2000]
    n = sum(lens)
    p, g, b = (torch.randn(n, generator=g_) * s for s in (0.5, 300.0, 0.1))
    hyper = torch.tensor([[0.01, 0.937, 5e-4, 1.0], [0.02, 0.937, 0.0, 1.0]], dtype=torch.float32)
    mul = float(np.float32(0.7) / np.float32(1024.0))
    rp, rb = sgd_ref(p, g, b, lens, hyper, mul, exact=False)
    # torch's fp32 evaluation of the same expressions on the CPU, one rounding per operation
    lr, mom, wd, _ = (torch.repeat_interleave(hyper[:, k], torch.tensor(lens)) for k in range(4))
    gr = g * mul + wd * p
    nb32 = mom * b + gr
    p32 = p - lr * (gr + mom * nb32)
    st, P_, B_ = run_sgd(gpu_device, p, g, b, lens, hyper, [mul, 0.0, 0.0, 0.0])
    assert st == OK, status(st, 'recipe values')
    assert_within_reference_error(P_.cpu(), p32, rp, 'sgd parameters')
    assert_within_reference_error(B_.cpu(), nb32, rb, 'sgd momentum')


# ---- yv4_ema_update --------------------------------------------------------------------------------------------------
def run_ema(dev, ema, x, m, n=None):
    E_, X_ = Arena(ema, dev), Arena(x, dev)
    st = _lib.lib().yv4_ema_update(E_.ptr(), X_.ptr(), ema.numel() if n is None else n, m, ops.stream_ptr())
    torch.cuda.synchronize()
    X_.assert_unchanged('ema_update online values'), E_.assert_pads_intact('ema_update')
    return st, E_


@pytest.mark.parametrize('n4', [1, 1000, SGD_TRIP + 333], ids=['one_word', 'small', 'second_trip'])
@pytest.mark.parametrize('m', [0.5, 0.75])
def test_ema_update_exact(gpu_device, m, n4):
    """ema = m * ema + (1 - m) * x on integers with m = 0.5 and 0.75: multiples of 0.25, exact; one word, a ragged size,
    and 4096 * 256 + 333 words (a second trip of the capped grid)."""
    n = 4 * n4
    ema, x = ints(n, 11, 8), ints(n, 12, 8)
    ref = exact32(exact32(ema.double() * m, 'm * ema') + exact32(x.double() * (1.0 - m), '(1 - m) * x'), 'ema')
    st, E_ = run_ema(gpu_device, ema, x, m)
    assert st == OK, status(st, 'ema_update')
    assert_bits(E_.cpu(), ref, f'ema m={m} n={n}')


def test_ema_update_of_nothing_and_refusals(gpu_device):
    ema, x = ints(64, 11, 8), ints(64, 12, 8)
    st, E_ = run_ema(gpu_device, ema, x, 0.5, n=0)
    assert st == OK, status(st, 'n = 0')
    E_.assert_unchanged('n = 0')
    st, E_ = run_ema(gpu_device, ema, x, 0.5, n=30)
    assert st == E_INVALID, status(st, 'n % 4')
    E_.assert_unchanged('n % 4')


def test_ema_update_recipe_momentum_against_float64(gpu_device):
    g_ = torch.Generator().manual_seed(8)
    n = 8000
    ema, x = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m32 = np.float32(0.9999)
    om32 = np.float32(1.0 - float(m32))                   # the launcher's (float)(1.0 - (double)momentum)
    ref = ema.double() * float(m32) + x.double() * float(om32)
    cpu32 = ema * float(m32) + x * float(om32)
    st, E_ = run_ema(gpu_device, ema, x, float(m32))
    assert st == OK, status(st, 'ema recipe')
    assert_within_reference_error(E_.cpu(), cpu32, ref, 'ema')


# ---- yv4_grad_prepare ------------------------------------------------------------------------------------------------
def run_prepare(dev, g, scale=None, max_norm=35.0, det=False, n=None):
    """One yv4_grad_prepare.  ``work`` has the 2 doubles the default mode uses, or the deterministic mode's
    2 + GRAD_PREPARE_MAX_WG, every one poisoned with NaN; ``ctrl`` is poisoned too.  Returns (status, ctrl, work) on
    the CPU."""
    G_ = Arena(g, dev)
    slots = 2 + (_lib.GRAD_PREPARE_MAX_WG if det else 0)
    W_ = Arena(torch.full((slots,), float('nan'), dtype=torch.float64), dev)
    C_ = Arena(torch.full((4,), float('nan')), dev)
    S_ = torch.tensor([scale, 5.0], dtype=torch.float32, device=dev) if scale is not None else None
    with det_mode(det):
        st = _lib.lib().yv4_grad_prepare(G_.ptr(), g.numel() if n is None else n, S_.data_ptr() if S_ is not None else None,
                                         max_norm, W_.ptr(), C_.ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    G_.assert_unchanged('grad_prepare gradients')
    C_.assert_pads_intact('grad_prepare ctrl'), W_.assert_pads_intact('grad_prepare work')
    return st, C_.cpu(), W_.cpu()


def check_prepare(ctrl, ss, scale, max_norm, what):
    """ctrl against the exact sum of squares ``ss`` (a Python int)."""
    inv = 1.0 / scale if scale is not None else 1.0                 # a power of two
    norm32 = float(np.float32(np.sqrt(np.float64(ss)))) * inv       # float32(sqrt(ss)) * inv_scale, the product exact
    assert float(ctrl[1]) == norm32, f'{what}: ctrl[1] = {float(ctrl[1])!r}, want {norm32!r} (ss = {ss})'
    assert float(ctrl[2]) == 0.0 and float(ctrl[3]) == inv, f'{what}: ctrl[2:] = {ctrl[2:].tolist()}'
    norm64 = float(np.sqrt(np.float64(ss))) * inv
    want0 = inv * (min(1.0, max_norm / (norm64 + 1e-6)) if max_norm > 0 else 1.0)
    assert abs(float(ctrl[0]) - want0) <= 2.0 ** -22 * want0, f'{what}: ctrl[0] = {float(ctrl[0])!r}, want {want0!r}'
    if max_norm <= 0 or max_norm / (norm64 + 1e-6) > 1.0 + 2.0 ** -20:
        assert float(ctrl[0]) == inv, f'{what}: an unclipped multiplier is 1 / scale exactly'


PREPARE_SIZES = {'nothing': 0, 'one_word': 1, 'small': 1000, 'inside_the_unroll': 2048 * 256 * 2 + 77,
                 'below_one_trip': SUMSQ_TRIP - 1, 'one_trip': SUMSQ_TRIP, 'above_one_trip': SUMSQ_TRIP + 1,
                 'two_trips_and_a_tail': 2 * SUMSQ_TRIP + 2048 * 256 + 5}


def _grads(n4):
    return ints(4 * n4, 21 + n4 % 7, 3)


def sumsq_grid(n4):
    """Workgroups yv4_grad_prepare launches for n4 16-byte words: one thread per four words, 256 threads, at most 2048."""
    return min(max(-(-(-(-n4 // 4)) // 256), 1), _lib.GRAD_PREPARE_MAX_WG) if n4 else 0


def _sumsq(g):
    return int((g.double() ** 2).sum().item())


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('size', list(PREPARE_SIZES), ids=list(PREPARE_SIZES))
def test_grad_prepare_sum_of_squares_is_exact(gpu_device, size, det):
    """Integer gradients: the double sum of squares is exact in any order, so ctrl[1] = float32(sqrt(ss)) / scale
    exactly (scale 1024), ctrl[0] within 2**-22 relative of the float64 value (the fp32 roundings of the norm, of
    ``+ 1e-6f``, of the division and of the product).  Sizes: nothing, one word, and n / 4 just below, at and above one
    trip of the capped grid (2048 x 256 x 4 words), ending inside the 4-way unroll, and two trips with a tail (75 MB).
    Deterministic mode: the same exact value from the per-workgroup slots, the same bits twice, and the slots beyond
    the launched grid (poisoned with NaN) are not read; default mode: work[2:] is not touched."""
    n4 = PREPARE_SIZES[size]
    g = _grads(max(n4, 1))                                  # n = 0: a valid pointer all the same
    ss = _sumsq(g) if n4 else 0
    assert ss < 2 ** 53
    st, ctrl, work = run_prepare(gpu_device, g, scale=1024.0, det=det, n=4 * n4)
    assert st == OK, status(st, size)
    check_prepare(ctrl, ss, 1024.0, 35.0, f'{size} det={det}')
    assert float(work[1]) == 0.0
    if det:
        grid = sumsq_grid(n4)
        assert float(work[2:2 + grid].sum()) == float(ss) and bool(torch.isnan(work[2 + grid:]).all())
        st2, ctrl2, work2 = run_prepare(gpu_device, g, scale=1024.0, det=True, n=4 * n4)
        assert st2 == OK and torch.equal(ctrl.view(torch.int32), ctrl2.view(torch.int32))
        assert torch.equal(work[:2 + grid].view(torch.int64), work2[:2 + grid].view(torch.int64))
    else:
        assert float(work[0]) == float(ss)


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_grad_prepare_clip_settings(gpu_device, det):
    """No loss scale (NULL: scale 1), clipping off (max_norm <= 0), a norm below max_norm (multiplier 1 / scale exactly)
    and above it."""
    g = _grads(1000)
    ss = _sumsq(g)
    for scale, max_norm in [(None, 35.0), (None, 0.0), (4.0, -1.0), (2.0 ** 20, 35.0), (1.0, 1e6), (65536.0, 0.5)]:
        st, ctrl, _ = run_prepare(gpu_device, g, scale=scale, max_norm=max_norm, det=det)
        assert st == OK, status(st, f'scale={scale} max_norm={max_norm}')
        check_prepare(ctrl, ss, scale, max_norm, f'scale={scale} max_norm={max_norm} det={det}')


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('where', ['last_word', 'second_trip', 'first_and_unroll'])
def test_grad_prepare_finds_non_finite_values(gpu_device, where, det):
    """One non-finite value in the last word of the array, in the second trip, or in the first word and inside the
    4-way unroll: ctrl[2] = 1.  A finite value whose fp32 square would overflow does not set it."""
    n4 = SUMSQ_TRIP + 2048 * 256 + 9
    g = _grads(n4)
    n = g.numel()
    if where == 'last_word':
        g[n - 1] = float('inf')
    elif where == 'second_trip':
        g[4 * (SUMSQ_TRIP + 3) + 2] = float('nan')
    else:
        g[0], g[4 * (2048 * 256 * 3 + 5) + 1] = float('-inf'), float('nan')
    st, ctrl, _ = run_prepare(gpu_device, g, scale=1024.0, det=det)
    assert st == OK, status(st, where)
    assert float(ctrl[2]) == 1.0 and float(ctrl[3]) == 2.0 ** -10
    if where == 'last_word':
        big = torch.zeros(1000 * 4)
        big[-1] = 3e38
        st, ctrl, _ = run_prepare(gpu_device, big, scale=None, max_norm=0.0, det=det)
        assert st == OK and float(ctrl[2]) == 0.0 and float(ctrl[1]) == float(np.float32(3e38)), ctrl.tolist()


def test_grad_prepare_refuses_a_ragged_length(gpu_device):
    st, ctrl, work = run_prepare(gpu_device, _grads(10), n=30)
    assert st == E_INVALID, status(st, 'n % 4')
    assert bool(torch.isnan(ctrl).all()) and bool(torch.isnan(work).all())
