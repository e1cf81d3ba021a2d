"""Fixture: what the convolution entry points answer to malformed descriptors (tests/test_conv_desc_host.py,
tools/conv_desc_check.cpp).

For each entry point a valid small descriptor is broken one field at a time (CASES below) and the call is made with FAKE
pointers against a library built from the commit BEFORE the shared descriptor check (csrc/conv_desc.h) went in:
    YV4_LIB_PATH=<that build's libyv4_hip.so> python tests/golden/make_golden_conv_desc.py
Only on a machine WITHOUT a GPU: a call whose descriptor that library accepts goes on to a launch, which fails there and
nowhere else.  Every call runs in a forked child, because that library divides by a zero stride or an empty reduction in
some entries.

One record per (entry, case), one per line of tests/golden/conv_desc_rejects.json:
  desc       the 19 integer fields N .. act2 of the descriptor
  rc         the expected return code of the call: that library's, or for a tightening YV4_E_INVALID
  by         "desc": the descriptor check rejects it; "entry": that library rejected it by a rule the entry keeps for
             itself (its shape rule, 4 GiB addressability: the shared check may get there first, with the same code);
             "none": the descriptor is valid and the call ends at the guard named below
  tightened  that library accepted (or crashed on) a descriptor that made it read or write outside a view, overflow a
             32-bit count or divide by zero; the shared check refuses it
  parent     what that library said
The guard that keeps an accepted call from launching: tile id 99 (forward, scatter, fp8: refused after validation), a
zero-byte workspace (split-K, on a shape that splits).  The weight gradient and the stem have no such guard, so the test
never calls them; their records are checked through check_conv_desc by tools/conv_desc_check.cpp.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIELDS = ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad', 'x_cstride', 'x_coff', 'y_cstride', 'y_coff',
          'r_cstride', 'r_coff', 'act1', 'act2')
P = 0x7f0000001000          # fake, 4 KiB aligned, never dereferenced on the host
LATE = ('tile id', 'workspace')                 # the guards behind the validation, as that library words them
ENTRY_RULES = ('needs Cin 4', 'multiple of 32', '4 GiB', 'K too large', 'scattered grid')


def base(cin=32, cout=64, al=16):
    """N 1, 8x8, 3x3 s1 p1, views with room on both sides of the channels."""
    d = dict(N=1, H=8, W=8, Cin=cin, Ho=8, Wo=8, Cout=cout, KH=3, KW=3, stride=1, pad=1, x_cstride=2 * cin, x_coff=al,
             y_cstride=2 * cout, y_coff=al, r_cstride=2 * cout, r_coff=al, act1=1, act2=2)
    return d


# entry -> (channel alignment, base descriptor, cases this entry accepts BY DESIGN, caller)
def entries(L, lib):
    f, h = L.F32, L.BF16

    def fwd(d):
        return lib.yv4_conv_bn_act_fwd(d, P, P, P, P, P, P, P, P, None)

    def fwd_h16(d):
        return lib.yv4_conv_bn_act_fwd_h16(d, h, h, P, P, P, P, P, P, P, P, None)

    def splitk(d):
        return lib.yv4_conv_bn_act_fwd_splitk(d, P, P, P, P, P, P, P, P, P, 0, None)

    def splitk_h16(d):
        return lib.yv4_conv_bn_act_fwd_h16_splitk(d, h, h, P, P, P, P, P, P, P, P, P, 0, None)

    def scatter(d):
        return lib.yv4_conv_scatter_fwd(d, P, P, P, P, P, 32, 32, 2, 2, 1, 1, None)

    def scatter_h16(d):
        return lib.yv4_conv_scatter_fwd_h16(d, h, P, P, P, P, P, 32, 32, 2, 2, 1, 1, None)

    def f8(d):
        return lib.yv4_conv_bn_act_fwd_f8(d, L.F8E4M3, P, P, P, P, P, P, P, 1.0, 1.0, P, None)

    def wgrad(d):
        return lib.yv4_conv_wgrad(d, P, P, P, None)

    def wgrad_h16(d):
        return lib.yv4_conv_wgrad_h16(d, h, P, P, P, None)

    def stem(d):
        return lib.yv4_conv_stem_fwd(d, P, P, P, P, P, f, None)

    y_free = {'y_cstride_misaligned', 'y_coff_misaligned', 'Cout_misaligned'}
    no_res = {'r_cstride_misaligned', 'r_coff_misaligned', 'r_coff_negative', 'r_view_exceeds'}
    res_free = {'r_cstride_misaligned', 'r_coff_misaligned'}
    acts = {'act1_negative', 'act2_above_swish'}
    stem_d = base(4, 32, 4)
    stem_d.update(x_cstride=8, x_coff=4)
    return {
        'conv': (4, base(), y_free | res_free, fwd),
        'conv h16': (8, base(), y_free | res_free, fwd_h16),
        'conv splitk': (4, base(512), y_free | res_free, splitk),
        'conv h16 splitk': (8, base(512), y_free | res_free, splitk_h16),
        'conv scatter': (4, base(), y_free | no_res | acts | {'Ho_off_by_one'}, scatter),
        'conv scatter h16': (8, base(), {'Cout_misaligned'} | no_res | acts | {'Ho_off_by_one'}, scatter_h16),
        'conv f8': (16, base(), y_free | res_free | {'taps65'}, f8),      # (no tap mask in the fp8 kernel)
        'wgrad': (4, base(), no_res | acts, wgrad),
        'wgrad h16': (8, base(), no_res | acts, wgrad_h16),
        'conv stem': (2, stem_d, y_free | no_res | {'act2_above_swish', 'x_cstride_misaligned'}, stem),
    }


def cases(d, al):
    """name -> the fields to overwrite: one defect each, everything else consistent with it"""
    hal = al // 2
    return {
        'N0': dict(N=0), 'H0': dict(H=0), 'W0': dict(W=0), 'Cin0': dict(Cin=0), 'Cout0': dict(Cout=0),
        'taps65': dict(KH=5, KW=13, pad=6, Ho=16, Wo=8),
        'stride0': dict(stride=0),
        'pad_negative': dict(pad=-1, Ho=4, Wo=4),
        'Cin_misaligned': dict(Cin=d['Cin'] + hal),
        'x_cstride_misaligned': dict(x_cstride=d['x_cstride'] + hal),
        'x_coff_misaligned': dict(x_coff=d['x_coff'] + hal),
        'x_coff_negative': dict(x_coff=-al),
        'x_view_exceeds': dict(x_coff=d['x_cstride'] - d['Cin'] + al),
        'Cout_misaligned': dict(Cout=d['Cout'] + hal),
        'y_cstride_misaligned': dict(y_cstride=d['y_cstride'] + hal),
        'y_coff_misaligned': dict(y_coff=d['y_coff'] + hal),
        'y_coff_negative': dict(y_coff=-al),
        'y_view_exceeds': dict(y_coff=d['y_cstride'] - d['Cout'] + al),
        'r_cstride_misaligned': dict(r_cstride=d['r_cstride'] + hal),
        'r_coff_misaligned': dict(r_coff=d['r_coff'] + hal),
        'r_coff_negative': dict(r_coff=-al),
        'r_view_exceeds': dict(r_coff=d['r_cstride'] - d['Cout'] + al),
        'Ho_off_by_one': dict(Ho=d['Ho'] + 1),
        'act1_negative': dict(act1=-1),
        'act2_above_swish': dict(act2=4),
        'pixels_2^31': dict(N=1 << 25),
        'valid': dict(),
    }


def call_in_child(L, lib, fn, fields):
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        d = L.ConvDesc()
        for k, v in fields.items():
            setattr(d, k, v)
        d.tile = 99
        rc = fn(C.byref(d))
        os.write(w, json.dumps([rc, lib.yv4_last_error().decode()]).encode())
        os._exit(0)
    os.close(w)
    out = b''
    while True:
        chunk = os.read(r, 65536)
        if not chunk:
            break
        out += chunk
    os.close(r)
    _, status = os.waitpid(pid, 0)
    if os.WIFSIGNALED(status) or not out:
        return None, f'killed by signal {os.WTERMSIG(status)}' if os.WIFSIGNALED(status) else 'no answer'
    return tuple(json.loads(out))


def main():
    import torch
    import mmdet_yolov4_amd as pkg
    if torch.cuda.is_available():
        sys.exit('a GPU is visible: this script makes calls that must not be able to launch')
    L = pkg._lib
    lib = L.lib()
    lines = []
    for entry, (al, d0, by_design, fn) in entries(L, lib).items():
        for case, change in cases(d0, al).items():
            fields = dict(d0)
            fields.update(change)
            rc, msg = call_in_child(L, lib, fn, fields)
            unguarded = entry.startswith('wgrad') or entry == 'conv stem'
            if rc is None:
                accepted = True                                   # crashed behind a validation that let it through
            elif unguarded:
                accepted = rc not in (L_INVALID, L_UNSUPPORTED)      # reached a launch, which failed for want of a GPU
            else:
                accepted = any(k in msg for k in LATE)
            want_accept = case == 'valid' or case in by_design
            rec = dict(entry=entry, case=case, desc=[fields[k] for k in FIELDS])
            if accepted and not want_accept:
                rec.update(rc=L_INVALID, by='desc', tightened=True)
            elif accepted:
                rec.update(rc=None if unguarded else rc, by='none', tightened=False)
            else:
                assert not want_accept or case != 'valid', (entry, case, rc, msg)
                rec.update(rc=rc, by='entry' if any(k in msg for k in ENTRY_RULES) else 'desc', tightened=False)
            rec['parent'] = f'rc {rc}: {msg}' if rc is not None else msg
            lines.append(json.dumps(rec))
    path = os.path.join(HERE, 'conv_desc_rejects.json')
    with open(path, 'w') as f:
        f.write('[\n' + ',\n'.join(lines) + '\n]\n')
    print(f'{path}: {len(lines)} records from {L.LIB_PATH}')


L_INVALID, L_UNSUPPORTED = -1, -2        # YV4_E_INVALID, YV4_E_UNSUPPORTED

if __name__ == '__main__':
    main()
