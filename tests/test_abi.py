"""The C-ABI library loads and exports every symbol include/yv4.h declares (no compute)."""
import os
import re

import pytest

import mmdet_yolov4_amd as pkg

import _abi_probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(yv4_[a-z0-9_]+)\s*\(', text))


def test_header_binding_library_agree():
    declared = _declared()
    assert declared, 'no declarations parsed'
    assert declared == set(pkg._lib.SIGNATURES), (declared ^ set(pkg._lib.SIGNATURES))
    lib = pkg._lib.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.yv4_abi_version() == pkg._lib.ABI_VERSION
    assert lib.yv4_arch() == b'gfx950'


def test_struct_layout_matches_header():
    import ctypes
    assert ctypes.sizeof(pkg._lib.ConvDesc) == 23 * 4 and pkg._lib.ConvDesc.flags.offset == 22 * 4     # ABI 7: + flags
    # yv4_loss_level / yv4_loss_desc (gcc sizeof on include/yv4.h: 176 / 1016, slot_anchor at 960, ABI 6's losses at 1008)
    assert ctypes.sizeof(pkg._lib.LossLevel) == 176 and ctypes.sizeof(pkg._lib.LossDesc) == 1016
    assert pkg._lib.LossDesc.slot_anchor.offset == 960 and pkg._lib.LossDesc.losses.offset == 1008
    assert ctypes.sizeof(pkg._lib.LevelDesc) == 8 + 3 * 4 + 4 + 8 * 4 * 4 or ctypes.sizeof(pkg._lib.LevelDesc) == 8 + 3 * 4 + 8 * 4 * 4 + 4


def test_every_struct_and_field_matches_a_c_compiler():
    """All of the ctypes mirror against the header: every struct the header declares is in ``STRUCTS``, with the
    header's members in the header's order (a field missing at the end of a class would pass the offsets), and a C
    compiler's ``sizeof`` of every struct and ``offsetof`` / ``sizeof`` of every field equal ctypes'."""
    import ctypes
    L = pkg._lib
    declared = _abi_probe.header_structs()
    assert set(declared) == set(L.STRUCTS), set(declared) ^ set(L.STRUCTS)
    assert len(L.STRUCTS) == 23 and len(set(L.STRUCTS.values())) == 23
    for cname, cls in L.STRUCTS.items():
        assert issubclass(cls, ctypes.Structure) and [f[0] for f in cls._fields_] == declared[cname], cname
    assert sum(len(cls._fields_) for cls in L.STRUCTS.values()) == 304
    p = _abi_probe.probe()                                      # skips without a C compiler
    assert len(p.sizeof) == 23 and len(p.fields) == 304
    assert _abi_probe.mismatches() == []


#: the header's constants that ``_lib`` deliberately does not mirror: nothing in the Python uses them
NOT_MIRRORED = {'OK', 'E_LAUNCH', 'E_CAPACITY', 'HTILE_128x128', 'HTILE_128x64', 'HTILE_64x64', 'HTILE_PP3x3', 'HTILE_W3x3',
                'HTILE_WIDE', 'HTILE_WS_1x1', 'HTILE_S3x3', 'JPEG_ERR_OVERRUN', 'JPEG_ERR_CODE', 'JPEG_ERR_DC_CATEGORY',
                'JPEG_ERR_INDEX', 'JPEG_ERR_TRAILING', 'JPEG_WG_CHUNKS'}


def test_constants_match_the_header():
    """Every object-like numeric ``#define YV4_*`` equals ``_lib``'s value of the same name, or is in NOT_MIRRORED --
    and is then really absent, so that the list cannot go stale in either direction."""
    L = pkg._lib
    defs = _abi_probe.header_constants()
    assert len(defs) == 84 and NOT_MIRRORED <= set(defs), NOT_MIRRORED - set(defs)
    for name, value in defs.items():
        if name in NOT_MIRRORED:
            assert not hasattr(L, name), f'{name} is mirrored: take it off NOT_MIRRORED'
        else:
            assert getattr(L, name) == value and type(getattr(L, name)) is int, name
    assert set(L.HTILE_NAMES) >= {defs[k] for k in NOT_MIRRORED if k.startswith('HTILE_')}


def test_pinned_tile_shapes_are_the_name_tables_keys():
    """The four ``YV4_*_SHAPE(i)`` macros over their pinned ranges, from the C compiler: exactly the keys of TILE_NAMES /
    HTILE_NAMES beyond the plain tile ids, under the name of the tile they pin."""
    L = pkg._lib
    shapes = _abi_probe.probe().shapes
    assert set(shapes) == set(L.SHAPE_COUNTS) and all(len(shapes[m]) == n for m, n in L.SHAPE_COUNTS.items())
    assert set(shapes['TILE_W3x3']) | set(shapes['TILE_WIDE']) == {t for t in L.TILE_NAMES if t > L.TILE_WIDE}
    assert set(shapes['HTILE_W3x3']) | set(shapes['HTILE_WIDE']) == {t for t in L.HTILE_NAMES if t > 8}
    for macro, names, base in (('TILE_W3x3', L.TILE_NAMES, L.TILE_W3x3), ('TILE_WIDE', L.TILE_NAMES, L.TILE_WIDE),
                               ('HTILE_W3x3', L.HTILE_NAMES, 5), ('HTILE_WIDE', L.HTILE_NAMES, 8)):
        assert all(names[t] == names[base] for t in shapes[macro]), macro


# ---- the binding rule, on stand-in handles ---------------------------------------------------------------------------
class _Fn:
    """An entry point of a stand-in library: accepts ``restype`` / ``argtypes`` as a ctypes function does."""
    restype = argtypes = None

    def __init__(self, value=0):
        self.value = value

    def __call__(self):
        return self.value


def _handle(without=(), abi=8):
    h = type('Handle', (), {})()
    for name in pkg._lib.SIGNATURES:
        if name not in without:
            setattr(h, name, _Fn(abi))
    return h


def _load(monkeypatch, handle):
    """``handle`` bound and in the place of the loaded library, for ``has`` / ``require``."""
    present = pkg._lib._bind(handle)
    monkeypatch.setattr(pkg._lib, '_lib', handle)
    monkeypatch.setattr(pkg._lib, '_has', present)
    return present


def _bound(handle, name):
    return getattr(handle, name).argtypes is pkg._lib.SIGNATURES[name][1]


def test_feature_table_is_well_formed():
    L = pkg._lib
    assert list(L.FEATURES) == ['fp8', 'tta', 'letterbox_batch', 'soft_nms', 'v3_augment', 'loss_ex', 'map_eval', 'map_flat',
                                'flex_flat', 'coco_eval', 'results_append', 'jpeg', 'jpeg_orientation', 'jpeg_entropy',
                                'jpeg_sync', 'jpeg_encode', 'draw', 'draw_ex', 'map_image', 'recall', 'v3_loss']
    owned = [s for ft in L.FEATURES.values() for s in ft.symbols]
    assert len(owned) == len(set(owned)), 'a symbol belongs to two features'
    assert all(ft.symbols and set(ft.symbols) <= set(L.SIGNATURES) for ft in L.FEATURES.values())
    assert {f: ft.requires for f, ft in L.FEATURES.items() if ft.requires} == \
        {'flex_flat': ('map_flat',), 'jpeg_sync': ('jpeg_entropy',), 'draw_ex': ('draw',)}
    assert {f: ft.abi for f, ft in L.FEATURES.items() if ft.abi} == {'v3_loss': 8}
    assert not [n for n in vars(L) if n.endswith('_SYMBOLS') or n.startswith('has_')]


def test_bind_a_complete_library(monkeypatch):
    L = pkg._lib
    h = _handle()
    assert _load(monkeypatch, h) == dict.fromkeys(L.FEATURES, True)
    assert all(_bound(h, n) and getattr(h, n).restype is L.SIGNATURES[n][0] for n in L.SIGNATURES)
    assert all(L.has(f) for f in L.FEATURES)
    for f in L.FEATURES:
        L.require(f)
    with pytest.raises(KeyError):
        L.has('jpeg_entropy_sync')


def test_bind_a_library_without_one_feature(monkeypatch):
    """Without jpeg_entropy's symbols: binding succeeds, the feature and the one that requires it are absent, nothing
    else is, and ``require`` names a missing symbol."""
    L = pkg._lib
    gone = L.FEATURES['jpeg_entropy'].symbols
    h = _handle(without=gone)
    _load(monkeypatch, h)
    assert {f for f in L.FEATURES if not L.has(f)} == {'jpeg_entropy', 'jpeg_sync'}
    assert all(_bound(h, n) for n in L.SIGNATURES if n not in gone) and not any(hasattr(h, n) for n in gone)
    with pytest.raises(RuntimeError, match='yv4_jpeg_entropy_decode_device.*rebuild'):
        L.require('jpeg_sync')
    with pytest.raises(RuntimeError, match="entropy='device' needs .*yv4_jpeg_scan_prepare"):
        L.require('jpeg_entropy', "entropy='device'")
    L.require('jpeg')


def test_bind_refuses_a_library_without_a_core_symbol():
    with pytest.raises(AttributeError, match='yv4_conv_bn_act_fwd'):
        pkg._lib._bind(_handle(without={'yv4_conv_bn_act_fwd'}))


def test_bind_half_a_feature(monkeypatch):
    """One symbol of a two-symbol feature gone: the other is still bound, the feature is absent."""
    L = pkg._lib
    h = _handle(without={'yv4_recall_work'})
    _load(monkeypatch, h)
    assert _bound(h, 'yv4_recall_match') and not L.has('recall')
    assert {f for f in L.FEATURES if not L.has(f)} == {'recall'}
    with pytest.raises(RuntimeError, match='yv4_recall_work') as e:
        L.require('recall')
    assert 'yv4_recall_match' not in str(e.value)


def test_bind_the_previous_abi(monkeypatch):
    """A library that reports ABI 7: the v3_loss symbols are left unbound even where it has them, and ``has`` says so."""
    L = pkg._lib
    h = _handle(abi=7)
    _load(monkeypatch, h)
    assert not any(_bound(h, n) for n in L.FEATURES['v3_loss'].symbols)
    assert all(_bound(h, n) for n in L.SIGNATURES if n not in L.FEATURES['v3_loss'].symbols)
    assert {f for f in L.FEATURES if not L.has(f)} == {'v3_loss'}
    with pytest.raises(RuntimeError, match='yv4_yolov3_loss_bwd / yv4_yolov3_loss_fwd'):
        L.require('v3_loss')
    with pytest.raises(AttributeError):          # ABI 8 without them is no ABI 8
        L._bind(_handle(without={'yv4_yolov3_loss_fwd'}))


def test_argument_validation_without_gpu():
    """Entry points reject bad arguments before touching the device."""
    import ctypes
    lib = pkg._lib.lib()
    d = pkg._lib.ConvDesc()
    assert lib.yv4_conv_bn_act_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None) == -1
    assert b'null' in lib.yv4_last_error()
    assert lib.yv4_mish_fwd(None, None, 16, 0, None) == -1
    assert lib.yv4_mish_fwd(None, None, 0, 0, None) == 0          # empty tensor: nothing to do
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = 2, 8, 8, 32, 8, 8, 64
    d.KH = d.KW = 3; d.stride = 1; d.pad = 1
    assert lib.yv4_conv_flops(ctypes.byref(d)) == 2.0 * 2 * 8 * 8 * 64 * 9 * 32
    assert lib.yv4_conv_pick_tile(ctypes.byref(d)) in (1, 2, 3, 4, 5, 6, 7)


def test_cpu_tensors_are_refused():
    """Everything with a plan or kernel behind it refuses CPU tensors.  (The standalone Mish op is the exception the
    reference makes too: mish.cc:14-22 dispatches on is_cuda -- test_mish_host_loop_matches_the_reference_fixture.)"""
    import pytest
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.batched_nms(torch.zeros(1, 4), torch.zeros(1), torch.zeros(1, dtype=torch.long), dict(iou_threshold=0.5))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.Conv(4, 8, 3).eval()(torch.zeros(1, 4, 8, 8))


def test_binding_argument_types_match_the_header():
    """Every prototype in include/yv4.h against the ctypes signature bound to it: argument count, and per argument
    the C scalar type (int / int64_t / float / double / size_t) or pointer-ness.  A wrong argtype (an int64_t bound
    as c_int, a missing argument) would corrupt the call silently."""
    import ctypes
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    protos = re.findall(r'\b([A-Za-z_][\w\s\*]*?)\b(yv4_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S)
    assert len(protos) >= 50
    scalar = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
              'double': ctypes.c_double, 'size_t': ctypes.c_size_t}

    def is_pointer_type(t):
        return t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int)))

    seen = set()
    for ret, name, args in protos:
        if name not in pkg._lib.SIGNATURES:
            continue
        seen.add(name)
        restype, argtypes = pkg._lib.SIGNATURES[name]
        args = ' '.join(args.split())
        params = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
        assert len(params) == len(argtypes), f'{name}: header has {len(params)} arguments, binding {len(argtypes)}'
        for i, (prm, bound) in enumerate(zip(params, argtypes)):
            if '*' in prm or '[' in prm:
                assert is_pointer_type(bound), f'{name} arg {i} ({prm}): bound as {bound}, header says pointer'
            else:
                ctype = prm.replace('const ', '').split()[0]
                assert ctype in scalar, f'{name} arg {i}: unhandled C type {prm!r}'
                assert bound is scalar[ctype], f'{name} arg {i} ({prm}): bound as {bound}'
        ret = ret.replace('const', '').strip()
        if '*' in ret:
            assert is_pointer_type(restype), name
        elif ret in scalar:
            assert restype is scalar[ret], f'{name}: returns {ret}, bound as {restype}'
    assert seen == set(pkg._lib.SIGNATURES), set(pkg._lib.SIGNATURES) - seen


def test_mish_host_loop_matches_the_reference_fixture(golden):
    """mish.cc:14-33: a CPU tensor runs the op's host loop.  The library's own loop (csrc/elementwise.hip
    yv4_mish_*_host, NOT the oracle) against tests/golden/mish.npz, which the reference's unmodified mish_cpu.cc produced:
    bit for bit in float32 and float64; Half / BFloat16 are refused as the reference's CPU dispatch refuses them."""
    import numpy as np
    import torch
    g = golden('mish')
    x, gr = torch.from_numpy(g['x']), torch.from_numpy(g['g'])
    np.testing.assert_array_equal(pkg.mish_forward(x).numpy(), g['y'])
    np.testing.assert_array_equal(pkg.mish_backward(gr, x).numpy(), g['gin'])
    np.testing.assert_array_equal(pkg.mish_forward(x.double()).numpy(), g['y64'])
    np.testing.assert_array_equal(pkg.mish_backward(gr.double(), x.double()).numpy(), g['gin64'])
    import pytest
    with pytest.raises(RuntimeError, match='not implemented for this dtype'):      # AT_DISPATCH_ALL_TYPES has no Half
        pkg.mish_forward(x.half())
    # the autograd Function on CPU tensors, end to end
    xr = x.clone().requires_grad_(True)
    pkg.MishFunction.apply(xr).backward(gr)
    np.testing.assert_array_equal(xr.grad.numpy(), g['gin'])
