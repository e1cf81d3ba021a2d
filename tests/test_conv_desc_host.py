"""Malformed descriptors at the convolution entry points: the return codes of tests/golden/conv_desc_rejects.json
(recorded from the library as it was before the shared check csrc/conv_desc.h, tests/golden/make_golden_conv_desc.py;
"tightened" marks what that library let through into an out-of-view access, a 32-bit overflow or a division by zero).

The pointers are fake and this test also runs where a GPU is present, so no call may be able to launch even if the check
under test wrongly passes: forward, scatter and fp8 calls carry tile id 99, which the dispatch refuses after validation
and before any launch; split-K calls use a shape that splits and a zero-byte workspace.  The weight gradient and the stem
have no such guard and are not called: tools/conv_desc_check.cpp runs their records through check_conv_desc."""
import ctypes as C
import json
import os

import pytest

import mmdet_yolov4_amd as pkg

L = pkg._lib
P = 0x7f0000001000          # fake, 4 KiB aligned, never dereferenced on the host
FIELDS = ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad', 'x_cstride', 'x_coff', 'y_cstride', 'y_coff',
          'r_cstride', 'r_coff', 'act1', 'act2')
INVALID, UNSUPPORTED = -1, -2
GUARDS = (b'tile', b'workspace')

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_desc_rejects.json')) as _f:
    RECORDS = json.load(_f)


def _callers(lib):
    h = L.BF16
    return {
        'conv': lambda d: lib.yv4_conv_bn_act_fwd(d, P, P, P, P, P, P, P, P, None),
        'conv h16': lambda d: lib.yv4_conv_bn_act_fwd_h16(d, h, h, P, P, P, P, P, P, P, P, None),
        'conv splitk': lambda d: lib.yv4_conv_bn_act_fwd_splitk(d, P, P, P, P, P, P, P, P, P, 0, None),
        'conv h16 splitk': lambda d: lib.yv4_conv_bn_act_fwd_h16_splitk(d, h, h, P, P, P, P, P, P, P, P, P, 0, None),
        'conv scatter': lambda d: lib.yv4_conv_scatter_fwd(d, P, P, P, P, P, 32, 32, 2, 2, 1, 1, None),
        'conv scatter h16': lambda d: lib.yv4_conv_scatter_fwd_h16(d, h, P, P, P, P, P, 32, 32, 2, 2, 1, 1, None),
        'conv f8': lambda d: lib.yv4_conv_bn_act_fwd_f8(d, L.F8E4M3, P, P, P, P, P, P, P, 1.0, 1.0, P, None),
    }


# the words by which a message names the defect of a case
DEFECT = {
    'N0': b'empty', 'H0': b'empty', 'W0': b'empty', 'Cin0': b'empty', 'Cout0': b'empty',
    'taps65': b'taps', 'stride0': b'stride', 'pad_negative': b'pad',
    'Cin_misaligned': b'multiples of', 'x_cstride_misaligned': b'multiples of', 'x_coff_misaligned': b'multiples of',
    'Cout_misaligned': b'multiples of', 'y_cstride_misaligned': b'multiples of', 'y_coff_misaligned': b'multiples of',
    'x_coff_negative': b'input view', 'x_view_exceeds': b'input view',
    'y_coff_negative': b'output view', 'y_view_exceeds': b'output view',
    'r_coff_negative': b'residual view', 'r_view_exceeds': b'residual view',
    'Ho_off_by_one': b'geometry', 'act1_negative': b'activation', 'act2_above_swish': b'activation',
    'pixels_2^31': b'31 bits',
}
# a split-K call whose shape does not split hands over to the plain entry, which reports under its own name
PREFIXES = {'conv splitk': (b'conv splitk:', b'conv:'), 'conv h16 splitk': (b'conv h16 splitk:', b'conv h16:')}

CALLED = [r for r in RECORDS if not r['entry'].startswith('wgrad') and r['entry'] != 'conv stem']


def test_the_table_covers_every_entry_and_case():
    entries = {r['entry'] for r in RECORDS}
    assert entries == set(_callers(None)) | {'wgrad', 'wgrad h16', 'conv stem'}
    for e in entries:
        assert {r['case'] for r in RECORDS if r['entry'] == e} == set(DEFECT) | {'valid', 'r_cstride_misaligned', 'r_coff_misaligned'}, e
    assert all(r['rc'] in (INVALID, UNSUPPORTED) for r in CALLED)
    assert all(r['by'] == 'desc' and r['rc'] == INVALID for r in RECORDS if r['tightened'])


@pytest.mark.parametrize('rec', CALLED, ids=[f"{r['entry']}-{r['case']}".replace(' ', '_') for r in CALLED])
def test_reject(rec):
    lib = L.lib()
    d = L.ConvDesc()
    for k, v in zip(FIELDS, rec['desc']):
        setattr(d, k, v)
    d.tile = 99
    rc = _callers(lib)[rec['entry']](C.byref(d))
    msg = lib.yv4_last_error()
    assert rc == rec['rc'], (rc, msg, rec['parent'])
    if rec['by'] == 'none':          # a valid descriptor: the call got as far as the guard, and no further
        assert any(g in msg for g in GUARDS), msg
        return
    assert not any(g in msg for g in GUARDS), msg
    assert msg.startswith(PREFIXES.get(rec['entry'], (rec['entry'].encode() + b':',))), msg
    if rec['by'] == 'desc':
        assert DEFECT[rec['case']] in msg, msg
