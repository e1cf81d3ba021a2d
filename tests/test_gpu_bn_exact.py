"""The train-mode BatchNorm + activation kernels (bn_train.hip: bn_stats, bn_finalize, bn_act_fwd, bn_act_bwd_reduce,
bn_act_bwd_apply and the pipelined bn16_* forms) through the C ABI, against tests/_bn_ref.py.

  a. exact coverage on integer operands (tests/_exact_ref.py): mean = 0, invstd = 1, gamma = 1 are handed in, so
     xhat = x; with act = none, or Mish at beta = 64 (every z >= 62: act' is exactly 1 in both kernel forms,
     tests/test_bn_ref_host.py), sums, forward outputs and eval-mode gradients are integers and need no tolerance.  The
     shapes walk the row and thread maps where they change form; each case asserts, from the launch arithmetic restated
     below, that it reaches what it names.  The YOLOv4-L BatchNorm table runs the same checks at full size, and one
     child process per measurement switch runs the coverage set through the forms the product never selects.
  b. per element against float64 on inputs that stress the arithmetic: max |got - ref64| / (u S + h) <= max(4 K32, R)
     with the scales S of _bn_ref.py, h half an ulp of a 16-bit output, K32 the same measure of the reference's own
     fp32 evaluation on the CPU, and R the fp32 roundings on the longest path of the kernel form.
  c. the SyncBN halves against the whole batch, and the refusals.

Every case runs in the default mode and in deterministic mode (twice: same bits); every output buffer is wider than
its view and must keep its canary outside it.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import mmdet_yolov4_amd as pkg  # noqa: F401
from mmdet_yolov4_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_ref as B  # noqa: E402
import _exact_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bn_bench import SHAPES as BN_SHAPES  # noqa: E402  (map side, channels, count) of YOLOv4-L at 608

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: L.F32, F16: L.F16, BF16: L.BF16}
NAME = {F32: 'f32', BF16: 'bf16', F16: 'f16'}
DTYPES = [F32, BF16, F16]
NONE, MISH, LEAKY, SWISH = B.ACT_NONE, B.ACT_MISH, B.ACT_LEAKY, B.ACT_SWISH
EPS, MOM, SLOPE = 1e-3, 0.03, 0.1
CANARY, PAD = 7.0, 3.0              # outside an output view / outside an input view
ACCUM_BASE_MAX = 10                 # publish == 2 starts from integers of at most this size
MEASURE_LIB = os.path.join(ROOT, 'mmdet-yolov4_amd', 'lib_alt', 'libyv4_hip_measure.so')


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module', autouse=True)
def _refs_checked():
    B.check_refs_cpu()


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic of bn_train.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
def switches():
    """(bn16 on, bn16 channels per thread, general kernels' 8-channel form): the product library reads no environment
    variable, the measurement build (``make measure``) reads these three once per process."""
    if os.path.basename(L.LIB_PATH) != os.path.basename(MEASURE_LIB):
        return True, 4, False
    e = os.environ
    return e.get('YV4_BN16', '1') != '0', int(e.get('YV4_BN16_V', '4')), e.get('YV4_BN_VEC8', '0') == '1'


def kernel_form(dtype, act, al):
    """('bn16' | 'general', channels per thread) of the row passes for this dtype, activation and view alignment."""
    bn16, v16, vec8 = switches()
    if dtype != F32 and act == MISH and bn16:
        return 'bn16', 8 if v16 == 8 and al % 8 == 0 else 4
    return 'general', 8 if dtype != F32 and vec8 and al % 8 == 0 else 4


def rows_per_block(M):                      # bn_rows_per_block: >= ~1024 workgroups, 32 .. 8192 rows each
    return min(max(32, -(-M // 1024)), 8192)


def red_map(CV):                            # red_map: 256 threads over CV channel vectors
    if CV <= 256:
        rpp = 256 // CV
        return dict(active=rpp * CV, rstep=rpp, passes=1)
    return dict(active=256, rstep=1, passes=-(-CV // 256))


def red_groups(C_):                         # bn_bwd_impl: channel groups of the backward reduction (grid.y)
    g = 1
    if C_ % 64 == 0 and C_ // 64 >= 2:
        g = min(C_ // 64, 16)
    while g > 1 and (C_ % g or (C_ // g) % 8):
        g -= 1
    return g


def _thread_rows(M, rb, rstep):
    sizes = {min(rb, M)} | ({M % rb} if M % rb and M > rb else set())
    return {-(-(n - rsub) // rstep) for n in sizes for rsub in range(rstep) if n > rsub}


def features(M, C_, V):
    """What a launch over (M, C_) with V channels per thread reaches.  Row passes (stats, forward, apply): 'inactive'
    threads, 'passes' over a row wider than 256 vectors, 'blocks1/2/3' (3 = three or more), a 'ragged' last block,
    and per-thread row counts: 'T<k>' = the bn16 double stage runs (>= 4 rows) and leaves a tail of k rows, 't<k>' = only a
    tail.  The backward reduction, with its own blocks and groups: 'g<groups>', 'r_inactive', 'r_passes', 'r_ragged',
    'R<k>' / 'r<k>'."""
    f = set()
    rb = rows_per_block(M)
    mp = red_map(C_ // V)
    if mp['active'] < 256:
        f.add('inactive')
    if mp['passes'] > 1:
        f.add('passes')
    nb = -(-M // rb)
    f.add(f'blocks{min(nb, 3)}')
    if M % rb and nb > 1:
        f.add('ragged')
    for n in _thread_rows(M, rb, mp['rstep']):
        f.add(f'T{n % 4}' if n >= 4 else f't{n % 4}')
    g = red_groups(C_)
    f.add(f'g{g}')
    rrb = min(rb * g, 8192)
    rm = red_map(C_ // g // V)
    if rm['active'] < 256:
        f.add('r_inactive')
    if rm['passes'] > 1:
        f.add('r_passes')
    if M % rrb and M > rrb:
        f.add('r_ragged')
    for n in _thread_rows(M, rrb, rm['rstep']):
        f.add(f'R{n % 4}' if n >= 4 else f'r{n % 4}')
    return f


# (M, C, alignment of strides and offsets, what the case is there for with 4 channels per thread)
COVER = [
    (1, 4, 4, {'blocks1', 't1', 'g1'}),
    (31, 8, 8, {'blocks1', 't1'}),
    (33, 24, 8, {'inactive', 'r_inactive', 'blocks2', 'ragged'}),
    (101, 36, 4, {'inactive', 'blocks3', 'ragged', 'r_ragged', 't2'}),
    (37, 64, 8, {'g1', 'ragged', 'r2'}),
    (1029, 128, 8, {'g2', 'blocks3', 'r_ragged', 'R0'}),
    (168, 192, 8, {'g3', 'inactive', 'T2', 'T3', 'R0', 'R1', 'R2'}),
    (356, 512, 8, {'g8', 'R3', 'T0'}),
    (37, 1024, 8, {'g16', 'T1', 'r3'}),
    (38, 1024, 4, {'g16', 'T2'}),
    (39, 1024, 8, {'g16', 'T3'}),
    (40, 1024, 8, {'g16', 'T0'}),
    (101, 1088, 8, {'passes', 'g8', 'r_inactive', 'R2', 'R3'}),
    (38, 2048, 8, {'passes', 'g16', 'T2'}),
    (77, 2048, 8, {'passes', 'g16', 'R1', 'R2'}),
    (33, 2056, 8, {'passes', 'r_passes', 'g1'}),
    (31, 4096, 8, {'passes', 'g16', 'T3'}),
    (40967, 64, 8, {'blocks3', 'ragged', 't3', 'r_ragged'}),
]
COVER_SHAPES = [(M, C_) for M, C_, _, _ in COVER]
EVERY_FEATURE = {'inactive', 'passes', 'blocks1', 'blocks2', 'blocks3', 'ragged', 'T0', 'T1', 'T2', 'T3', 't1', 't2', 't3',
                 'g1', 'g2', 'g3', 'g8', 'g16', 'r_inactive', 'r_passes', 'r_ragged', 'R0', 'R1', 'R2', 'R3', 'r1', 'r2', 'r3'}


def test_cover_reaches_every_form():
    """The coverage set, by the arithmetic above: every case reaches what it names with 4 channels per thread, the set as a
    whole reaches every form with 4 channels per thread and with 8, and it holds every channel count and row count named
    in DESIGN 4.8."""
    for M, C_, al, names in COVER:
        assert names <= features(M, C_, 4), (M, C_, names - features(M, C_, 4))
    for V in (4, 8):
        got = set().union(*(features(M, C_, V) for M, C_, al, _ in COVER if C_ % V == 0 and al % V == 0))
        assert EVERY_FEATURE <= got, (V, EVERY_FEATURE - got)
    assert {4, 8, 24, 36, 64, 192, 1024, 1088, 2056, 4096} <= {c for _, c in COVER_SHAPES}
    assert {1, 31, 33} <= {m for m, _ in COVER_SHAPES}


# ---------------------------------------------------------------------------------------------------------------------
# views, canaries and the ABI calls
# ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """Channel views that differ between x, dy, dx, y and the residual: (cstride, coff) each, multiples of ``al``."""

    def __init__(self, C_, al):
        self.C, self.al = C_, al
        self.x, self.dy, self.dx = (C_ + al, al), (C_ + 2 * al, 0), (C_ + 3 * al, 2 * al)
        self.y, self.res = (C_ + al, 0), (C_ + 2 * al, al)


def put(val, view, fill):
    """``val`` (M, C) inside a (M, cstride) buffer of ``fill``."""
    cs, co = view
    buf = torch.full((val.shape[0], cs), fill, dtype=val.dtype, device=val.device)
    buf[:, co:co + val.shape[1]] = val
    return buf


def out_buf(M, view, dtype, dev):
    return torch.full((M, view[0]), CANARY, dtype=dtype, device=dev)


def take(buf, view, C_, what):
    """The view of an output buffer, after checking that every channel outside it kept the canary."""
    cs, co = view
    keep = torch.ones(cs, dtype=torch.bool, device=buf.device)
    keep[co:co + C_] = False
    assert bool((buf[:, keep] == CANARY).all()), f'{what}: channels outside [{co}, {co + C_}) of {cs} were written'
    return buf[:, co:co + C_]


def vec_out(C_, dev, dtype=F32, fill=CANARY):
    return torch.full((C_ + 8,), fill, dtype=dtype, device=dev)


def vec_take(v, C_, what, fill=CANARY):
    assert bool((v[C_:] == fill).all()), f'{what}: written beyond its {C_} channels'
    return v[:C_]


class Pass:
    """One set of operands in their views, and the entry points over it."""

    def __init__(self, dtype, x, dy, res, mean, invstd, gamma, beta, act, slope=SLOPE, al=8):
        self.dtype, self.act, self.slope = dtype, act, slope
        self.M, self.C = x.shape
        self.dev = x.device
        self.lay = Layout(self.C, al)
        self.x, self.dy, self.res = x, dy, res
        self.xb = put(x, self.lay.x, PAD)
        self.dyb = put(dy, self.lay.dy, PAD) if dy is not None else None
        self.resb = put(res, self.lay.res, PAD) if res is not None else None
        self.mean, self.invstd, self.gamma, self.beta = (t.float().contiguous() for t in (mean, invstd, gamma, beta))
        self.form = kernel_form(dtype, act, al)

    # -- argument groups
    def _xdy(self, with_dtype=True):
        a = (self.xb.data_ptr(),) + ((CODE[self.dtype],) if with_dtype else ()) + self.lay.x
        return a + (self.dyb.data_ptr(),) + self.lay.dy + self._chan()

    def _chan(self):
        return (self.mean.data_ptr(), self.invstd.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr())

    def work(self):
        return torch.full((4 * self.C + 8,), CANARY, dtype=torch.float64, device=self.dev)

    # -- entry points; each returns its status and outputs (taken from their views when the status is 0)
    def fwd(self, with_res):
        lib = L.lib()
        yb = out_buf(self.M, self.lay.y, self.dtype, self.dev)
        r = (self.resb.data_ptr() if with_res else None,) + self.lay.res
        tail = r + (yb.data_ptr(),) + self.lay.y + (self.M, self.C, self.act, self.slope, _stream())
        if self.dtype == F32:
            rc = lib.yv4_bn_act_fwd(self.xb.data_ptr(), *self.lay.x, *self._chan(), *tail)
        else:
            rc = lib.yv4_bn_act_fwd_h16(self.xb.data_ptr(), CODE[self.dtype], *self.lay.x, *self._chan(), *tail)
        torch.cuda.synchronize()
        return rc, (take(yb, self.lay.y, self.C, 'y') if rc == 0 else None)

    def bwd(self, entry, base=None, M_total=None, rows_dev=None, sums=None):
        """entry: 'train' (yv4_bn_act_bwd[_h16]), 'eval' (yv4_bn_eval_act_bwd), 'accum' / 'accum_eval' / 'accum_zero'
        (yv4_bn_act_bwd_accum with flags 0 / 1 / 2; ``base`` = (dgamma, dbeta) already in place), 'sums'
        (yv4_bn_act_bwd_sums: returns work), 'apply' (yv4_bn_act_bwd_apply on ``sums``)."""
        lib = L.lib()
        dxb = out_buf(self.M, self.lay.dx, self.dtype, self.dev)
        dg, db = vec_out(self.C, self.dev), vec_out(self.C, self.dev)
        if base is not None:
            dg[:self.C], db[:self.C] = base
        wk = self.work()
        dxa = (dxb.data_ptr(),) + self.lay.dx
        red = (dg.data_ptr(), db.data_ptr(), wk.data_ptr(), self.M, self.C, self.act, self.slope)
        if entry == 'train' and self.dtype == F32:
            rc = lib.yv4_bn_act_bwd(*self._xdy(False), *dxa, *red, _stream())
        elif entry == 'train':
            rc = lib.yv4_bn_act_bwd_h16(*self._xdy(), *dxa, *red, _stream())
        elif entry == 'eval':
            rc = lib.yv4_bn_eval_act_bwd(*self._xdy(), *dxa, *red, _stream())
        elif entry in ('accum', 'accum_eval', 'accum_zero'):
            flags = {'accum': 0, 'accum_eval': 1, 'accum_zero': 2}[entry]
            if flags == 2:
                wk[:4 * self.C] = 0
            rc = lib.yv4_bn_act_bwd_accum(*self._xdy(), *dxa, *red, flags, _stream())
        elif entry == 'sums':
            rc = lib.yv4_bn_act_bwd_sums(*self._xdy(), *red, _stream())
        elif entry == 'apply':
            wk[:2 * self.C] = sums
            rc = lib.yv4_bn_act_bwd_apply(*self._xdy(), *dxa, wk.data_ptr(), self.M, M_total,
                                          rows_dev.data_ptr() if rows_dev is not None else None, self.C, self.act,
                                          self.slope, _stream())
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
        out = dict(rc=rc)
        if rc != 0:
            assert bool((dxb == CANARY).all()), f'{entry}: refused, yet dx was written'
            return out
        assert float(wk[4 * self.C]) == CANARY, f'{entry}: work written beyond 4 C doubles'
        if entry != 'sums':
            out['dx'] = take(dxb, self.lay.dx, self.C, f'{entry} dx')
        else:
            assert bool((dxb == CANARY).all())
            out['work'] = wk[:2 * self.C].clone()
        if entry != 'apply':
            out['dgamma'], out['dbeta'] = vec_take(dg, self.C, 'dgamma'), vec_take(db, self.C, 'dbeta')
        return out

    def stats(self, rm0=None, rv0=None, mom=MOM):
        lib = L.lib()
        mean, invstd = vec_out(self.C, self.dev), vec_out(self.C, self.dev)
        rm, rv = vec_out(self.C, self.dev), vec_out(self.C, self.dev)
        rm[:self.C] = rm0 if rm0 is not None else 0
        rv[:self.C] = rv0 if rv0 is not None else 1
        wk = self.work()
        cs, co = self.lay.x
        tail = (self.M, self.C, cs, co, EPS, mom, wk.data_ptr(), mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
                rv.data_ptr(), _stream())
        if self.dtype == F32:
            rc = lib.yv4_bn_train_stats(self.xb.data_ptr(), *tail)
        else:
            rc = lib.yv4_bn_train_stats_h16(self.xb.data_ptr(), CODE[self.dtype], *tail)
        torch.cuda.synchronize()
        if rc != 0:
            return rc, None
        assert float(wk[4 * self.C]) == CANARY
        return rc, tuple(vec_take(v, self.C, n) for v, n in ((mean, 'mean'), (invstd, 'invstd'), (rm, 'rm'), (rv, 'rv')))

    def partial_sums(self):
        wk = self.work()
        cs, co = self.lay.x
        rc = L.lib().yv4_bn_partial_sums(self.xb.data_ptr(), CODE[self.dtype], self.M, self.C, cs, co, wk.data_ptr(),
                                         _stream())
        torch.cuda.synchronize()
        assert float(wk[4 * self.C]) == CANARY
        return rc, wk[:2 * self.C]


class modes:
    """Runs ``fn(det)`` in the default mode and twice in deterministic mode, restoring the mode afterwards; the two
    deterministic results (tuples / dicts of tensors) must have the same bits.  Returns {0: ..., 1: ...}."""

    @staticmethod
    def run(fn):
        lib = L.lib()
        was = lib.yv4_get_deterministic()
        out = {}
        try:
            for det in (0, 1):
                lib.yv4_set_deterministic(det)
                out[det] = fn(det)
                if det:
                    again = fn(det)
                    _same_bits(out[det], again)
        finally:
            lib.yv4_set_deterministic(was)
        return out


def _same_bits(a, b, where='deterministic mode, two runs'):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same_bits(a[k], b[k], f'{where}: {k}')
    elif isinstance(a, (tuple, list)):
        for i, (u, v) in enumerate(zip(a, b)):
            _same_bits(u, v, f'{where}[{i}]')
    elif torch.is_tensor(a):
        ai, bi = a.contiguous(), b.contiguous()
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        assert torch.equal(ai.view(it), bi.view(it)), f'{where}: bits differ'
    else:
        assert a == b, where


def _ulps(a, b64):
    ai = a.float().contiguous().view(torch.int32).long()
    bi = b64.float().contiguous().view(torch.int32).long()
    return int((ai - bi).abs().max().item()) if a.numel() else 0


# ---------------------------------------------------------------------------------------------------------------------
# R: fp32 roundings on the longest path of an output, counted from bn_train.hip (DESIGN 4.8 lists every path); an
# operation written in the source counts once whether or not the compiler contracts it, v_exp_f32 / v_rcp_f32 /
# expf / a division count as two, a select, a min and a multiplication by a power of two as none
# ---------------------------------------------------------------------------------------------------------------------
R_Z = 3            # sa = invstd * gamma -> (x - mean) * sa -> + beta             (general forward)
R_Z_BWD = 4        # x - mean -> * invstd -> * gamma -> + beta                     (general backward passes)
R_Z_16 = 4         # A = invstd * gamma -> mean * A -> beta - . -> fma(x, A, B)    (bn16, all three passes)
R_Y = {('general', NONE): R_Z + 1,               # + residual
       ('general', LEAKY): R_Z + 2,              # * slope, + residual
       ('general', SWISH): R_Z + 8,              # -z log2 e, exp2 (2), 1 + ., rcp (2), z * ., + residual
       ('general', MISH): R_Z + 10,              # z log2 e, exp2 (2), e + 2, e * ., n + 2, rcp (2), (z n) * r, + residual
       ('bn16', MISH): R_Z_16 + 11}              # ... the same nine, n * r, z * ., + residual
R_G = {('general', NONE): 0,                     # dy * 1
       ('general', LEAKY): 1,                    # dy * slope
       ('general', SWISH): R_Z_BWD + 9,          # expf (2), 1 + ., 1 / . (2), 1 - s, (z s) * ., s + ., dy * .
       ('general', MISH): R_Z_BWD + 10,          # z log2 e, exp2 (2), e + 1, fma(a, a, 1), rcp (2), iw * iw, fma, dy * .
       ('bn16', MISH): R_Z_16 + 10}              # the same ten (u = iw + iw is exact)


def r_dx(form, act, eval_mode):
    if form == 'bn16':
        return R_G[(form, act)] + 1              # fma(K1, g, fma(C1, x, C0)); the C1 / C0 path is 7 long
    if eval_mode:
        return max(R_G[(form, act)] + 1, 2)      # k1 * g; k1 = gamma * invstd itself is one
    return max(R_G[(form, act)] + 3, 5)          # (g - dbm) - xhat * dgm, * k1;  x - mean, * invstd, * dgm, -, * k1


R_MEAN = 32        # 31 fp32 additions of a run of 32 rows (kBnFloatRun x kBnRedUnroll) and the fp32 result
R_VAR = 33         # ... and the square


# ---------------------------------------------------------------------------------------------------------------------
# a. exact coverage on integer operands
# ---------------------------------------------------------------------------------------------------------------------
def _exact_operands(dtype, M, C_, seed, dev, big=False):
    x = X.int_operand((M, C_), seed, dev, dtype, big=big)
    dy = X.int_operand((M, C_), seed + 1, dev, dtype, big=big)
    res = X.int_operand((M, C_), seed + 2, dev, dtype, big=big)
    X.guard(M, X.amax(x), X.amax(dy), extra=ACCUM_BASE_MAX)
    return x, dy, res


def _chunked_exact(got, want_fn, dtype, what, names=('row', 'c')):
    """assert_exact a chunk of rows at a time; ``want_fn(r0, r1)`` gives the float64 reference of those rows."""
    M, C_ = got.shape
    step = B.row_step(C_)
    for r0 in range(0, M, step):
        X.assert_exact(got[r0:r0 + step], want_fn(r0, min(M, r0 + step)), dtype, f'{what} rows from {r0}', names)


def _check_k(got, ref64, S, dtype, bound, what):
    k, i = B.k_of(got, ref64, S, dtype)
    assert k <= bound, (f'{what}: K = {k:.3g} > {bound:.3g} at flat index {i}: got {float(got.flatten()[i])!r}, '
                        f'float64 {float(ref64.flatten()[i])!r}, u S = {B.U * float(S.flatten()[i]):.3g}')
    return k


def exact_case(dtype, M, C_, al, dev, seed=0, big=False, dx_train=True):
    """Every entry point over one integer-operand case, act = none (beta = 0) and Mish (beta = 64), both modes."""
    x, dy, res = _exact_operands(dtype, M, C_, seed + M + C_, dev, big)
    zeros, ones = torch.zeros(C_, device=dev), torch.ones(C_, device=dev)
    xd, dyd = x.double(), dy.double()
    s1, s2 = xd.sum(0), (xd * xd).sum(0)
    dbeta64, dgamma64 = dyd.sum(0), (dyd * xd).sum(0)
    base = (ACCUM_BASE_MAX // 5 * X.int_operand((C_,), seed + 5, dev), ACCUM_BASE_MAX // 2 * X.int_operand((C_,), seed + 6, dev))
    assert max(X.amax(base[0]), X.amax(base[1])) <= ACCUM_BASE_MAX and X.amax(base[0]) > 0
    tag0 = f'{NAME[dtype]} M={M} C={C_} al={al}'
    # --- statistics
    st64 = B.stats(x, EPS)
    rm0, rv0 = torch.linspace(-1, 1, C_, device=dev), torch.linspace(0.5, 1.5, C_, device=dev)
    rm64, rv64 = B.running(rm0, rv0, st64['mean'], st64['var'], M, MOM)
    p0 = Pass(dtype, x, dy, res, zeros, ones, ones, zeros, NONE, al=al)

    def stat_run(det):
        tag = f'{tag0} det={det}'
        limit = 2048 if det else 4096
        rc, ps = p0.partial_sums()
        rc2, st = p0.stats(rm0, rv0)
        if C_ > limit:
            assert rc != 0 and rc2 != 0, f'{tag}: {C_} channels must be refused'
            return None
        L.check(rc, 'yv4_bn_partial_sums')
        L.check(rc2, 'yv4_bn_train_stats')
        X.assert_exact(ps[:C_], s1, torch.float64, f'{tag} partial sums', ('c',))
        X.assert_exact(ps[C_:], s2, torch.float64, f'{tag} partial sums of squares', ('c',))
        mean, invstd, rm, rv = st
        assert torch.equal(mean, (s1 / M).float()), f'{tag}: mean != fp32(sum / M)'
        assert _ulps(invstd, st64['invstd']) <= 1, f'{tag}: invstd'
        assert _ulps(rm, rm64) <= 1 and _ulps(rv, rv64) <= 1, f'{tag}: running statistics'
        return ps.clone(), st
    modes.run(stat_run)

    # --- forward and backward, act = none and Mish at beta = 64
    for act, beta_v in ((NONE, 0.0), (MISH, 64.0)):
        beta = torch.full((C_,), beta_v, device=dev)
        p = Pass(dtype, x, dy, res, zeros, ones, ones, beta, act, al=al)
        form, V = p.form
        ref_args = (zeros, ones, ones, beta, act, B.f32(SLOPE))
        sums64 = B.backward_sums(x, dy, *ref_args) if dx_train else None
        if dx_train:      # the reference agrees that this setting is exact: act' == 1, xhat == x
            assert torch.equal(sums64['dbeta'], dbeta64) and torch.equal(sums64['dgamma'], dgamma64)

        def run(det):
            tag = f'{tag0} {B.ACT_NAMES[act]} {form} V={V} det={det}'
            out = {}
            for with_res in (False, True):
                rc, y = p.fwd(with_res)
                L.check(rc, 'yv4_bn_act_fwd')
                _chunked_exact(y, lambda a, b: xd[a:b] + beta_v + (res[a:b].double() if with_res else 0), dtype,
                               f'{tag} y res={with_res}')
                out[f'y{int(with_res)}'] = y
            if det and C_ // red_groups(C_) > 2048:
                assert p.bwd('train')['rc'] != 0, f'{tag}: {C_} channels in one group must be refused'
                return out
            for entry in ('train', 'eval', 'accum', 'accum_eval', 'accum_zero'):
                o = p.bwd(entry, base=base if entry.startswith('accum') else None)
                L.check(o['rc'], entry)
                add = (base[0].double(), base[1].double()) if entry.startswith('accum') else (0.0, 0.0)
                X.assert_exact(o['dgamma'], dgamma64 + add[0], F32, f'{tag} {entry} dgamma', ('c',))
                X.assert_exact(o['dbeta'], dbeta64 + add[1], F32, f'{tag} {entry} dbeta', ('c',))
                if entry in ('eval', 'accum_eval'):
                    _chunked_exact(o['dx'], lambda a, b: dyd[a:b], dtype, f'{tag} {entry} dx')
                elif dx_train:
                    dx64, S = B.backward_dx(x, dy, *ref_args, sums64, M)
                    _check_k(o['dx'], dx64, S, dtype, r_dx(form, act, False), f'{tag} {entry} dx')
                out[entry] = o
            _same_bits(out['accum_zero'], out['accum'], f'{tag}: flag 2 on a zeroed work against flag 0')
            # the two halves of the SyncBN backward: local sums exact, doubles leave the library in either mode
            o = p.bwd('sums')
            L.check(o['rc'], 'sums')
            X.assert_exact(o['work'][:C_], dbeta64, torch.float64, f'{tag} work dbeta', ('c',))
            X.assert_exact(o['work'][C_:], dgamma64, torch.float64, f'{tag} work dgamma', ('c',))
            X.assert_exact(o['dgamma'], dgamma64, F32, f'{tag} sums dgamma', ('c',))
            X.assert_exact(o['dbeta'], dbeta64, F32, f'{tag} sums dbeta', ('c',))
            a = p.bwd('apply', sums=o['work'], M_total=M)
            L.check(a['rc'], 'apply')
            _same_bits(a['dx'], out['train']['dx'], f'{tag}: apply on the sums against the one-call backward')
            out['sums'] = o
            return out
        modes.run(run)


@pytest.mark.parametrize('dtype', DTYPES, ids=[NAME[d] for d in DTYPES])
@pytest.mark.parametrize('M,C_,al,names', COVER, ids=[f'{m}x{c}a{a}' for m, c, a, _ in COVER])
def test_cover_exact(gpu_device, M, C_, al, names, dtype):
    """One shape of the coverage set through every entry point: sums, forward outputs and eval-mode gradients bit for
    bit, the train-mode dx within R of float64, accumulate-onto (publish == 2) exact, the two-call backward equal to
    the one-call backward, refusals where LDS does not hold a group in deterministic mode."""
    exact_case(dtype, M, C_, al, gpu_device)


def table_rows(batch, hw):
    """Rows and operand set of a layer-table map: {-1, 1} where 4 M would pass 2**24, and a batch lowered (to a multiple
    of 8 images) only where M itself would."""
    M = batch * hw * hw
    big = 4 * M + ACCUM_BASE_MAX >= X.EXACT_LIMIT
    if M + ACCUM_BASE_MAX >= X.EXACT_LIMIT:
        M = max(1, (X.EXACT_LIMIT - 1 - ACCUM_BASE_MAX) // (hw * hw) // 8 * 8) * hw * hw
    return M, big


TABLE_RUNS = [(BF16, 64), (F16, 8), (F32, 8)]


@pytest.mark.parametrize('dtype,batch', TABLE_RUNS, ids=['bf16-b64', 'f16-b8', 'f32-b8'])
def test_yolov4l_bn_table_exact(gpu_device, dtype, batch):
    """Every BatchNorm map of YOLOv4-L at 608 (tools/bn_bench.py SHAPES) at the training batch in bf16 and at batch 8 in
    fp16 / fp32, the batch lowered only where the 2**24 guard demands it (bf16 at 608 x 608 runs 40 images)."""
    for hw, C_, _ in BN_SHAPES:
        M, big = table_rows(batch, hw)
        exact_case(dtype, M, C_, 8, gpu_device, seed=hw, big=big, dx_train=False)
        torch.cuda.empty_cache()


def test_conv_epilogue_sums_exact(gpu_device):
    """yv4_conv_fwd_stats + yv4_conv_stats_fold on integer operands: the totals of the stored outputs, exactly, in both
    modes (the epilogue's fp32 partial sums are integers below 2**24)."""
    dev = gpu_device
    lib = L.lib()
    N, H, W, Cin, Cout = 3, 23, 19, 64, 96
    for dtype in (BF16, F16, F32):
        x = X.int_operand((N, H, W, Cin), 91, dev, dtype, big=True)
        w = X.int_operand((Cout, 3, 3, Cin), 92, dev, dtype, big=True)
        X.guard(9 * Cin, 1, 1)                          # |y| <= 576: an integer in fp32, rounded once where bf16 stores it
        ones, zeros = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
        d = L.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, H, W, Cout
        d.KH = d.KW = 3
        d.stride, d.pad = 1, 1
        d.x_cstride, d.y_cstride, d.r_cstride = Cin, Cout, Cout

        def run(det):
            y = torch.empty(N, H, W, Cout, dtype=dtype, device=dev)
            stats = torch.zeros(L.STATS_REPLICAS * 2 * Cout, dtype=torch.float64, device=dev)
            L.check(lib.yv4_conv_fwd_stats(C.byref(d), CODE[dtype], x.data_ptr(), w.data_ptr(), ones.data_ptr(),
                                           zeros.data_ptr(), y.data_ptr(), stats.data_ptr(), 1, _stream()), 'conv_fwd_stats')
            tot = torch.full((2 * Cout + 1,), CANARY, dtype=torch.float64, device=dev)
            L.check(lib.yv4_conv_stats_fold(stats.data_ptr(), Cout, 1, tot.data_ptr(), _stream()), 'conv_stats_fold')
            torch.cuda.synchronize()
            yd = y.double().reshape(-1, Cout)
            ref = X.fwd_ref(x, w.permute(0, 3, 1, 2).float(), 1, 1).reshape(-1, Cout)
            X.assert_exact(y.reshape(-1, Cout), ref, dtype, f'{NAME[dtype]} conv output', ('row', 'c'))
            # whatever rows a partial sum of the epilogue covers, it is an integer below 2**24
            assert float((yd * yd).sum(0).max()) < X.EXACT_LIMIT
            X.assert_exact(tot[:Cout], yd.sum(0), torch.float64, f'{NAME[dtype]} det={det} epilogue sums', ('c',))
            X.assert_exact(tot[Cout:2 * Cout], (yd * yd).sum(0), torch.float64, f'{NAME[dtype]} det={det} sums of squares', ('c',))
            assert float(tot[2 * Cout]) == CANARY and not bool(stats.any())
            return (tot,)
        modes.run(run)


def child_main():
    """In a fresh process (the switches are read once per process): the coverage set, one line per case."""
    dev = torch.device('cuda:0')
    B.check_refs_cpu()
    sw = switches()
    print('SWITCHES', sw, os.path.basename(L.LIB_PATH), flush=True)
    for M, C_, al, _ in COVER:
        for dtype in (BF16, F16):
            exact_case(dtype, M, C_, al, dev)
            print('OK', NAME[dtype], M, C_, al, kernel_form(dtype, MISH, al), kernel_form(dtype, NONE, al), flush=True)
    print('CHILD DONE', flush=True)


@pytest.mark.parametrize('env,want', [({'YV4_BN16': '0'}, (False, 4, False)), ({'YV4_BN16_V': '8'}, (True, 8, False)),
                                      ({'YV4_BN_VEC8': '1'}, (True, 4, True))],
                         ids=['YV4_BN16=0', 'YV4_BN16_V=8', 'YV4_BN_VEC8=1'])
def test_cover_exact_under_switch_in_child(gpu_device, env, want):
    """The forms the product never selects -- the general kernels on 16-bit Mish (YV4_BN16=0: what the 1-ulp test of
    test_gpu_train_ops.py trusts as its reference), 8 channels per thread in the pipelined kernels (YV4_BN16_V=8) and in
    the general ones (YV4_BN_VEC8=1) -- on the 16-bit coverage set, one child process at a time.  The product library
    reads no environment variable, so the child loads the measurement build (``make measure``, built by build())."""
    assert os.path.exists(MEASURE_LIB), f'{MEASURE_LIB} is missing: build() makes it (make -C csrc measure)'
    code = (f'import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]; '
            f'import test_gpu_bn_exact as M; M.child_main()')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, YV4_LIB_PATH=MEASURE_LIB, **env),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'CHILD DONE' in r.stdout, r.stdout[-2000:]
    assert f'SWITCHES {want}' in r.stdout, r.stdout[:300]


# ---------------------------------------------------------------------------------------------------------------------
# b. per element against float64
# ---------------------------------------------------------------------------------------------------------------------
_K32 = {}


def _report(case, dtype, act, tensor, k32, bound, ks):
    print(f'BNK | {case} | {NAME[dtype]} | {B.ACT_NAMES[act] if act is not None else "-"} | {tensor} | {k32:.2f} | '
          f'{bound:.1f} | {ks[0]:.2f} | {ks[1]:.2f} |', flush=True)


def _gen(name, dtype, M, C_, dev, act):
    gens = dict(usual=B.gen_usual, const_channel=B.gen_const_channel, tiny_std=B.gen_tiny_std, big_gamma=B.gen_big_gamma,
                huge_gamma=B.gen_huge_gamma, gamma_signs=B.gen_gamma_signs, leaky_zero=B.gen_leaky_zero)
    seed = 100 + sum(map(ord, name))
    if name.startswith('ratio'):
        c = B.gen_ratio(int(name[5:]), dtype, M, C_, seed, dev)
    elif name == 'fp16_range':
        c = B.gen_fp16_range(M, C_, seed, dev)
    else:
        c = gens[name](dtype, M, C_, seed, dev)
    if act == LEAKY:
        B.settle_leaky(c)
        assert int(B.ambiguous(c).sum()) == 0
    c.check_claims()
    return c


def _k32_fwd_bwd(c, act, with_res):
    """K32 of y, dx, dgamma, dbeta: the reference's own fp32 evaluation on the CPU against its float64 one."""
    cpu = [t.cpu() for t in (c.x, c.dy, c.res, c.mean, c.invstd, c.gamma, c.beta)]
    x, dy, res, args = cpu[0], cpu[1], cpu[2] if with_res else None, tuple(cpu[3:]) + (act, B.f32(SLOPE))
    y64, Sy = B.forward(x, *args, res)
    y32, _ = B.forward(x, *args, res, dt=F32, want_scale=False)
    s64, s32 = B.backward_sums(x, dy, *args), B.backward_sums(x, dy, *args, dt=F32)
    dx64, Sdx = B.backward_dx(x, dy, *args, s64, c.M)
    dx32, _ = B.backward_dx(x, dy, *args, s32, c.M, dt=F32, want_scale=False)
    return dict(y=B.k_of(y32, y64, Sy)[0], dx=B.k_of(dx32, dx64, Sdx)[0],
                dgamma=B.k_of(s32['dgamma'], s64['dgamma'], s64['S_dgamma'])[0],
                dbeta=B.k_of(s32['dbeta'], s64['dbeta'], s64['S_dbeta'])[0])


# (case, rows, dtypes, activations, residual forms); C = 24: six channel vectors, 252 of 256 threads active
ALL_ACTS = (NONE, MISH, LEAKY, SWISH)
STRESS = [
    ('usual', 200003, DTYPES, ALL_ACTS, (False, True)),
    ('ratio10', 8209, DTYPES, (MISH, LEAKY), (False,)),
    ('ratio100', 8209, DTYPES, (MISH, LEAKY), (True,)),
    ('ratio1000', 8209, (F32, F16), (MISH, SWISH), (False,)),
    ('const_channel', 4099, DTYPES, ALL_ACTS, (False,)),
    ('tiny_std', 4099, DTYPES, (MISH, LEAKY), (True,)),
    ('big_gamma', 8209, DTYPES, ALL_ACTS, (False, True)),
    ('huge_gamma', 4099, (F32, BF16), (MISH, SWISH, LEAKY), (False,)),
    ('gamma_signs', 4099, DTYPES, ALL_ACTS, (True,)),
    ('fp16_range', 4099, (F16,), ALL_ACTS, (False, True)),
    ('leaky_zero', 8208, DTYPES, (LEAKY,), (False, True)),
]
STRESS_PARAMS = [pytest.param(n, M, dt, a, r, id=f'{n}-{NAME[dt]}-{B.ACT_NAMES[a]}-{"res" if r else "plain"}')
                 for n, M, dts, acts, rs in STRESS for dt in dts for a in acts for r in rs]


@pytest.mark.parametrize('name,M,dtype,act,with_res', STRESS_PARAMS)
def test_forward_backward_per_element(gpu_device, name, M, dtype, act, with_res):
    """y, dx, dgamma, dbeta of the one-call forward and backward against float64, every element:
    K = max |got - ref64| / (u S + h) <= max(4 K32, R) for y and dx, <= 4 K32 + 2 for dgamma and dbeta."""
    C_ = 24
    c = _gen(name, dtype, M, C_, gpu_device, act)
    k32 = _k32_fwd_bwd(c, act, with_res)
    slope = B.f32(SLOPE)
    args = (c.mean, c.invstd, c.gamma, c.beta, act, slope)
    res = c.res if with_res else None
    y64, Sy = B.forward(c.x, *args, res)
    s64 = B.backward_sums(c.x, c.dy, *args)
    dx64, Sdx = B.backward_dx(c.x, c.dy, *args, s64, c.M)
    p = Pass(dtype, c.x, c.dy, c.res, c.mean, c.invstd, c.gamma, c.beta, act)
    form, _ = p.form
    bounds = dict(y=max(4 * k32['y'], R_Y[(form, act)]), dx=max(4 * k32['dx'], r_dx(form, act, False)),
                  dgamma=4 * k32['dgamma'] + 2, dbeta=4 * k32['dbeta'] + 2)

    def run(det):
        rc, y = p.fwd(with_res)
        L.check(rc, 'fwd')
        o = p.bwd('train')
        L.check(o['rc'], 'bwd')
        return dict(y=y, dx=o['dx'], dgamma=o['dgamma'], dbeta=o['dbeta'])
    outs = modes.run(run)
    ks = {}
    for det in (0, 1):
        o = outs[det]
        ks[det] = dict(y=B.k_of(o['y'], y64, Sy, dtype)[0], dx=B.k_of(o['dx'], dx64, Sdx, dtype)[0],
                       dgamma=B.k_of(o['dgamma'], s64['dgamma'], s64['S_dgamma'])[0],
                       dbeta=B.k_of(o['dbeta'], s64['dbeta'], s64['S_dbeta'])[0])
    for t in ('y', 'dx', 'dgamma', 'dbeta'):
        _report(f'{name}{"+res" if with_res else ""}', dtype, act, t, k32[t], bounds[t], (ks[0][t], ks[1][t]))
    tag = f'{name} {NAME[dtype]} {B.ACT_NAMES[act]} res={with_res} {form}'
    for det in (0, 1):
        o = outs[det]
        _check_k(o['y'], y64, Sy, dtype, bounds['y'], f'{tag} det={det} y')
        _check_k(o['dx'], dx64, Sdx, dtype, bounds['dx'], f'{tag} det={det} dx')
        _check_k(o['dgamma'], s64['dgamma'], s64['S_dgamma'], F32, bounds['dgamma'], f'{tag} det={det} dgamma')
        _check_k(o['dbeta'], s64['dbeta'], s64['S_dbeta'], F32, bounds['dbeta'], f'{tag} det={det} dbeta')


@pytest.mark.parametrize('dtype', DTYPES, ids=[NAME[d] for d in DTYPES])
@pytest.mark.parametrize('act', [MISH, SWISH, LEAKY], ids=['mish', 'swish', 'leaky'])
def test_eval_backward_per_element(gpu_device, dtype, act):
    """yv4_bn_eval_act_bwd on the usual and the big-gamma input: dx = gamma invstd g per element, the sums as in train
    mode."""
    for name in ('usual', 'big_gamma'):
        c = _gen(name, dtype, 8209, 24, gpu_device, act)
        args = (c.mean, c.invstd, c.gamma, c.beta, act, B.f32(SLOPE))
        s64 = B.backward_sums(c.x, c.dy, *args)
        dx64, Sdx = B.backward_dx(c.x, c.dy, *args, None, 0, eval_mode=True)
        cpu = [t.cpu() for t in (c.x, c.dy, c.mean, c.invstd, c.gamma, c.beta)]
        cargs = tuple(cpu[2:]) + (act, B.f32(SLOPE))
        dx32, _ = B.backward_dx(cpu[0], cpu[1], *cargs, None, 0, eval_mode=True, dt=F32, want_scale=False)
        s32 = B.backward_sums(cpu[0], cpu[1], *cargs, dt=F32)
        k32 = dict(dx=B.k_of(dx32, dx64.cpu(), Sdx.cpu())[0],
                   dgamma=B.k_of(s32['dgamma'], s64['dgamma'].cpu(), s64['S_dgamma'].cpu())[0],
                   dbeta=B.k_of(s32['dbeta'], s64['dbeta'].cpu(), s64['S_dbeta'].cpu())[0])
        p = Pass(dtype, c.x, c.dy, c.res, c.mean, c.invstd, c.gamma, c.beta, act)
        form, _ = p.form
        bound = max(4 * k32['dx'], r_dx(form, act, True))

        def run(det):
            o = p.bwd('eval')
            L.check(o['rc'], 'eval')
            return o
        outs = modes.run(run)
        for det in (0, 1):
            tag = f'eval {name} {NAME[dtype]} {B.ACT_NAMES[act]} {form} det={det}'
            k = _check_k(outs[det]['dx'], dx64, Sdx, dtype, bound, f'{tag} dx')
            _check_k(outs[det]['dgamma'], s64['dgamma'], s64['S_dgamma'], F32, 4 * k32['dgamma'] + 2, f'{tag} dgamma')
            _check_k(outs[det]['dbeta'], s64['dbeta'], s64['S_dbeta'], F32, 4 * k32['dbeta'] + 2, f'{tag} dbeta')
            if det:
                _report(f'{name} (eval)', dtype, act, 'dx', k32['dx'], bound,
                        (B.k_of(outs[0]['dx'], dx64, Sdx, dtype)[0], k))


STAT_CASES = [('usual', 200003, DTYPES), ('ratio10', 8209, DTYPES), ('ratio100', 8209, DTYPES), ('ratio1000', 8209, (F32, F16)),
              ('const_channel', 4099, DTYPES), ('tiny_std', 4099, DTYPES), ('fp16_range', 4099, (F16,))]


@pytest.mark.parametrize('name,M,dtype', [pytest.param(n, M, dt, id=f'{n}-{NAME[dt]}') for n, M, dts in STAT_CASES for dt in dts])
def test_statistics_per_channel(gpu_device, name, M, dtype):
    """yv4_bn_train_stats[_h16] against float64 per channel: mean on S_mean, the variance (read back from the running
    variance at momentum 1) on S_var, invstd on S_invstd; bounds max(4 K32, R).  For the mean/std ladder the achieved
    relative error of invstd is printed beside torch's own fp32 batch_norm on the same device and data.

    ``fp16_range`` in deterministic mode is what gave the statistics' fixed-point words their eight extra fraction bits
    (yv4_common.h, kFxStatFr): at a resolution of 2**-40 the variance of its channels of fp16 denormals (x^2 ~ 2e-10) came
    out 1e-4 off, K = 2 279 against a bound of 33 (0.87 in the default mode)."""
    C_ = 24
    c = _gen(name, dtype, M, C_, gpu_device, None)
    st = c.st
    s32 = B.stats(c.x.cpu(), EPS, dt=F32)
    k32 = dict(mean=B.k_of(s32['mean'], st['mean'].cpu(), st['S_mean'].cpu())[0],
               var=B.k_of(s32['var'], st['var'].cpu(), st['S_var'].cpu())[0],
               invstd=B.k_of(s32['invstd'], st['invstd'].cpu(), st['S_invstd'].cpu())[0])
    bounds = dict(mean=max(4 * k32['mean'], R_MEAN), var=max(4 * k32['var'], R_VAR), invstd=max(4 * k32['invstd'], R_VAR))
    p = Pass(dtype, c.x, None, None, c.mean, c.invstd, c.gamma, c.beta, NONE)
    zeros = torch.zeros(C_, device=gpu_device)

    def run(det):
        rc, o = p.stats(zeros, zeros, mom=1.0)
        L.check(rc, 'stats')
        return o
    outs = modes.run(run)
    ks = {}
    for det in (0, 1):
        mean, invstd, rm, rv = outs[det]
        assert torch.equal(rm, mean), 'running mean at momentum 1 is the mean'
        var = rv.double() * (M - 1) / M                      # the unbiased variance, scaled back exactly
        ks[det] = dict(mean=B.k_of(mean, st['mean'], st['S_mean'])[0], var=B.k_of(var, st['var'], st['S_var'])[0],
                       invstd=B.k_of(invstd, st['invstd'], st['S_invstd'])[0])
    for t in ('mean', 'var', 'invstd'):
        _report(name, dtype, None, t, k32[t], bounds[t], (ks[0][t], ks[1][t]))
    if name.startswith('ratio') or name == 'usual':
        xt = c.x.float().t().reshape(1, C_, M, 1).contiguous()
        _, _, t_invstd = torch.native_batch_norm(xt, None, None, None, None, True, 0.0, B.f32(EPS))
        rel = lambda v: float(((v.double() - st['invstd']).abs() / st['invstd']).max())
        print(f'BNLADDER | {name} | {NAME[dtype]} | {float(c.ratio().min()):.0f} | {rel(outs[0][1]):.2e} | {rel(outs[1][1]):.2e} | '
              f'{rel(t_invstd):.2e} |', flush=True)
    for det in (0, 1):
        for t in ('mean', 'var', 'invstd'):
            assert ks[det][t] <= bounds[t], f'{name} {NAME[dtype]} det={det} {t}: K = {ks[det][t]:.3g} > {bounds[t]:.3g}'


# ---------------------------------------------------------------------------------------------------------------------
# c. the entry points against each other, and the refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=[NAME[d] for d in DTYPES])
@pytest.mark.parametrize('act', [MISH, LEAKY], ids=['mish', 'leaky'])
def test_syncbn_halves_against_the_whole(gpu_device, dtype, act):
    """yv4_bn_act_bwd_sums on two row halves, the caller adding the two ``work`` arrays, then yv4_bn_act_bwd_apply on
    each half with M_total = 2 M -- once as a host count, once through ``rows_dev`` (beside a host count of M, which the
    device-resident one must override): dx equals the float64 reference of the whole batch, each half's dgamma / dbeta
    that half's reference."""
    Mh, C_ = 4099, 24
    c = _gen('usual', dtype, 2 * Mh, C_, gpu_device, act)
    slope = B.f32(SLOPE)
    args = (c.mean, c.invstd, c.gamma, c.beta, act, slope)
    cpu = [t.cpu() for t in (c.x, c.dy, c.mean, c.invstd, c.gamma, c.beta)]
    cargs = tuple(cpu[2:]) + (act, slope)
    whole64 = B.backward_sums(c.x, c.dy, *args)
    whole32 = B.backward_sums(cpu[0], cpu[1], *cargs, dt=F32)
    dx64, Sdx = B.backward_dx(c.x, c.dy, *args, whole64, 2 * Mh)
    dx32, _ = B.backward_dx(cpu[0], cpu[1], *cargs, whole32, 2 * Mh, dt=F32, want_scale=False)
    halves = (slice(0, Mh), slice(Mh, 2 * Mh))
    ps = [Pass(dtype, c.x[h], c.dy[h], None, c.mean, c.invstd, c.gamma, c.beta, act) for h in halves]
    form, _ = ps[0].form
    bound_dx = max(4 * B.k_of(dx32, dx64.cpu(), Sdx.cpu())[0], r_dx(form, act, False))
    rows = torch.tensor([2.0 * Mh], dtype=torch.float64, device=gpu_device)

    def run(det):
        loc = [p.bwd('sums') for p in ps]
        for o in loc:
            L.check(o['rc'], 'sums')
        total = loc[0]['work'] + loc[1]['work']
        host = [p.bwd('apply', sums=total, M_total=2 * Mh) for p in ps]
        devc = [p.bwd('apply', sums=total, M_total=Mh, rows_dev=rows) for p in ps]
        for o in host + devc:
            L.check(o['rc'], 'apply')
        return dict(loc=loc, host=host, dev=devc)
    outs = modes.run(run)
    for det in (0, 1):
        o = outs[det]
        tag = f'syncbn {NAME[dtype]} {B.ACT_NAMES[act]} det={det}'
        for i, h in enumerate(halves):
            h64 = B.backward_sums(c.x[h], c.dy[h], *args)
            h32 = B.backward_sums(cpu[0][h], cpu[1][h], *cargs, dt=F32)
            for t in ('dgamma', 'dbeta'):
                k32 = B.k_of(h32[t], h64[t].cpu(), h64['S_' + t].cpu())[0]
                _check_k(o['loc'][i][t], h64[t], h64['S_' + t], F32, 4 * k32 + 2, f'{tag} half {i} {t}')
            _check_k(o['host'][i]['dx'], dx64[h], Sdx[h], dtype, bound_dx, f'{tag} half {i} dx (host count)')
            _same_bits(o['dev'][i]['dx'], o['host'][i]['dx'], f'{tag} half {i}: rows_dev against the host count')


def test_refusals(gpu_device):
    """One assertion per refusal, nothing launched (the outputs keep their canaries: Pass.bwd checks dx)."""
    dev = gpu_device
    lib = L.lib()

    def mk(C_, M=8):
        z = torch.zeros(C_, device=dev)
        x = torch.ones(M, C_, device=dev)
        return Pass(F32, x, x.clone(), x.clone(), z, z + 1, z + 1, z, NONE, al=4)
    # (a width that is not a multiple of 4 cannot even be laid out by Layout's aligned views: hand it in directly)
    p = mk(8)
    p.C = 6
    assert p.bwd('train')['rc'] != 0 and p.fwd(False)[0] != 0 and p.stats()[0] != 0, 'C % 4 != 0'
    p = mk(4100)
    assert p.bwd('train')['rc'] != 0 and p.fwd(False)[0] != 0 and p.stats()[0] != 0, 'C > 4096'
    p = mk(2056)
    was = lib.yv4_get_deterministic()
    try:
        lib.yv4_set_deterministic(1)
        assert p.bwd('train')['rc'] != 0 and p.stats()[0] != 0, 'deterministic mode above 2048 channels per group'
        lib.yv4_set_deterministic(0)
        assert p.bwd('train')['rc'] == 0 and p.stats()[0] == 0
    finally:
        lib.yv4_set_deterministic(was)
    p = mk(8)
    sums = torch.zeros(16, dtype=torch.float64, device=dev)
    assert p.bwd('apply', sums=sums, M_total=7)['rc'] != 0, 'M_total < M'
    assert p.bwd('apply', sums=sums, M_total=8)['rc'] == 0
