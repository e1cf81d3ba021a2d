"""The JPEG decoder without a GPU: the numpy restatement against libjpeg-turbo's output, and the library's host half
(parse and Huffman decode, ``csrc/jpeg_host.cpp``) against the restatement -- exactly, for every fixture -- and against
damaged input.  ``tests/golden/jpeg.npz`` holds the files and Pillow's decode of them (make_golden_jpeg.py)."""
import ctypes

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
import _jpeg_ref as R

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -4
SMALL = ('9x7_420_grad_q90', '17x33_420_grad_q90_rst2')      # the truncation / byte-flip subjects: 4:2:0, one with RSTn


@pytest.fixture(scope='module')
def jpeg(golden):
    g = golden('jpeg')
    return {k: g[k] for k in g.files}


def _names(jpeg):
    return [str(n) for n in jpeg['names']]


def _lib_parse(buf):
    info = pkg._lib.JpegInfo()
    return pkg._lib.lib().yv4_jpeg_parse(buf, len(buf), ctypes.byref(info)), info


def _lib_decode(buf, capacity=None):
    """-> (status, info, coefficients in a buffer of exactly ``capacity`` elements behind a guard)."""
    st, info = _lib_parse(buf)
    if st != OK:
        return st, info, None
    n = int(info.ncoef) if capacity is None else capacity
    coef = np.full(n + 64, 0x5a5a, np.int16)                # pre-filled: the decoder must zero what it owns ...
    info2 = pkg._lib.JpegInfo()
    st = pkg._lib.lib().yv4_jpeg_entropy_decode(buf, len(buf), ctypes.byref(info2), coef.ctypes.data, n)
    assert bytes(info2) == bytes(info), 'parse and entropy_decode disagree about the header'
    assert (coef[n:] == 0x5a5a).all(), 'the decoder wrote past the capacity it was given'      # ... and nothing else
    return st, info, coef[:n]


def _same_info(info, ref):
    for k in ('width', 'height', 'ncomp', 'restart_interval', 'mcus_x', 'mcus_y', 'ncoef', 'scan_offset'):
        assert getattr(info, k) == ref[k], k
    nc = ref['ncomp']
    for k in ('hs', 'vs', 'tq', 'td', 'ta', 'blocks_w', 'blocks_h'):
        assert list(getattr(info, k))[:nc] == list(ref[k]), k
    np.testing.assert_array_equal(np.ctypeslib.as_array(info.quant).reshape(4, 64), ref['quant'])


def test_restatement_equals_libjpeg_turbo_on_every_fixture(jpeg):
    assert len(_names(jpeg)) >= 72
    for n in _names(jpeg):
        buf = jpeg['jpg_' + n].tobytes()
        np.testing.assert_array_equal(R.decode(buf, 'rgb'), jpeg['rgb_' + n], err_msg=n)
        np.testing.assert_array_equal(R.decode(buf, 'bgr'), jpeg['rgb_' + n][:, :, ::-1], err_msg=n)


def test_fixtures_cover_the_cases(jpeg):
    """Every sampling at every size, restart intervals, optimised tables and quality-100 noise."""
    seen, restarts, names = set(), 0, _names(jpeg)
    for n in names:
        info = R.parse(jpeg['jpg_' + n].tobytes())
        samp = 'gray' if info['ncomp'] == 1 else {(1, 1): '444', (2, 1): '422', (2, 2): '420'}[(info['hs'][0], info['vs'][0])]
        seen.add((info['height'], info['width'], samp))
        restarts += info['restart_interval'] > 0
    for h, w in ((1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (37, 53), (40, 72), (48, 64)):
        for samp in ('444', '422', '420', 'gray'):
            assert (h, w, samp) in seen
    assert restarts >= 3 and sum(n.endswith('q30_opt') for n in names) == 4 and sum(n.endswith('q100') for n in names) == 8


def coarse_table_file(jpeg, mult=20):
    """A quality-100 noise file with the first six entries of its quantisation table raised from 1 to ``mult``: the
    IDCT output leaves 0..255 by more than 384, which is where libjpeg's range-limit table wraps around.  No encoder
    writes such a file, so none of the fixtures reaches that part of the table; this one pins the stated rule."""
    buf = bytearray(jpeg['jpg_48x64_gray_noise_q100'].tobytes())
    dqt = bytes(buf).index(b'\xff\xdb')
    for k in range(6):
        buf[dqt + 5 + k] = mult
    return bytes(buf)


def test_range_limit_rule_wraps_where_a_clamp_does_not(jpeg):
    info, coef = R.entropy_decode(coarse_table_file(jpeg))
    exact = R.reconstruct(info, coef)
    table = R._range_limit
    try:
        R._range_limit = lambda v: np.clip(v + 128, 0, 255).astype(np.uint8)
        clamped = R.reconstruct(info, coef)
    finally:
        R._range_limit = table
    assert not np.array_equal(exact, clamped)
    v = np.arange(-2048, 2048, dtype=np.int32)
    inside = (v >= -512) & (v < 512)          # the table is a clamp of v + 128 exactly for -512 <= v < 512
    np.testing.assert_array_equal(table(v)[inside], np.clip(v + 128, 0, 255)[inside])
    assert table(np.int32(512)) == 0 and table(np.int32(895)) == 0 and table(np.int32(-513)) == 255 and table(np.int32(-1024)) == 128


def test_library_parse_fills_the_info_struct(jpeg):
    for n in _names(jpeg):
        buf = jpeg['jpg_' + n].tobytes()
        st, info = _lib_parse(buf)
        assert st == OK, (n, pkg._lib.lib().yv4_last_error())
        _same_info(info, R.parse(buf))


def test_library_coefficients_equal_the_restatement(jpeg):
    for n in _names(jpeg):
        buf = jpeg['jpg_' + n].tobytes()
        st, info, coef = _lib_decode(buf)
        assert st == OK, (n, pkg._lib.lib().yv4_last_error())
        np.testing.assert_array_equal(coef, R.entropy_decode(buf)[1], err_msg=n)
        info2, coef2 = image_io.jpeg_entropy_decode(buf)      # the Python wrapper of the same calls
        np.testing.assert_array_equal(coef2, coef)


def test_capacity_is_checked_before_anything_is_written(jpeg):
    buf = jpeg['jpg_17x33_420_grad_q90'].tobytes()
    ncoef = int(_lib_parse(buf)[1].ncoef)
    st, _, coef = _lib_decode(buf, capacity=ncoef - 1)
    assert st == CAPACITY and (coef == 0x5a5a).all()
    assert b'coefficients' in pkg._lib.lib().yv4_last_error()


def test_refusal_set_is_unsupported_and_names_the_reason(jpeg):
    L = pkg._lib.lib()
    assert sorted(str(n) for n in jpeg['refused']) == ['cmyk', 'progressive']
    buf = jpeg['jpg_progressive'].tobytes()
    assert _lib_parse(buf)[0] == UNSUPPORTED and b'progressive' in L.yv4_last_error()
    assert _lib_decode(buf)[0] == UNSUPPORTED
    buf = jpeg['jpg_cmyk'].tobytes()
    assert _lib_parse(buf)[0] == UNSUPPORTED and b'4 components' in L.yv4_last_error()
    with pytest.raises(NotImplementedError, match='CMYK'):
        image_io.jpeg_parse(buf)


def _patched(buf, edits):
    b = bytearray(buf)
    for off, val in edits:
        b[off] = val
    return bytes(b)


def test_other_unsupported_and_invalid_headers(jpeg):
    """Hand-made variants of one 4:2:0 file: what the header says decides the code."""
    buf = jpeg['jpg_17x33_420_grad_q90'].tobytes()
    sof = buf.index(b'\xff\xc0')
    dqt = buf.index(b'\xff\xdb')
    assert _lib_parse(_patched(buf, [(sof + 4, 12)]))[0] == UNSUPPORTED            # 12-bit samples
    assert _lib_parse(_patched(buf, [(sof + 1, 0xC9)]))[0] == UNSUPPORTED          # arithmetic coding
    assert _lib_parse(_patched(buf, [(sof + 1, 0xC3)]))[0] == UNSUPPORTED          # lossless
    assert _lib_parse(_patched(buf, [(sof + 11, 0x41)]))[0] == UNSUPPORTED         # luma sampled 4x1
    assert _lib_parse(_patched(buf, [(sof + 14, 0x21)]))[0] == UNSUPPORTED         # chroma sampled 2x1
    assert _lib_parse(_patched(buf, [(dqt + 4, 0x10)]))[0] == UNSUPPORTED          # a 16-bit quantisation table
    assert _lib_parse(_patched(buf, [(sof + 5, 0), (sof + 6, 0)]))[0] == INVALID   # zero height
    assert _lib_parse(_patched(buf, [(sof + 12, 3)]))[0] == INVALID                # a quantisation table that is not there
    assert _lib_parse(_patched(buf, [(sof + 11, 0x02)]))[0] == INVALID             # sampling factor 0
    assert _lib_parse(b'')[0] == INVALID and _lib_parse(b'\xff\xd8')[0] == INVALID and _lib_parse(buf[2:])[0] == INVALID
    # more entropy-coded data than the header's MCUs: the same scan under a frame header one MCU row shorter
    short = _patched(buf, [(sof + 6, 16)])
    assert _lib_parse(short)[0] == OK and _lib_decode(short)[0] == INVALID
    assert b'more entropy-coded data' in pkg._lib.lib().yv4_last_error()
    # a taller frame over the same scan: the data ends early
    tall = _patched(buf, [(sof + 6, 40)])
    assert _lib_decode(tall)[0] == INVALID


def _grid(info):
    """The MCU grid and coefficient count that follow from an info struct's size and sampling."""
    mx = -(-info.width // (8 * info.hs[0]))
    my = -(-info.height // (8 * info.vs[0]))
    bw = [mx * info.hs[i] for i in range(info.ncomp)]
    bh = [my * info.vs[i] for i in range(info.ncomp)]
    return mx, my, bw, bh, 64 * sum(a * b for a, b in zip(bw, bh))


def _check_consistent(buf):
    """One damaged input through parse and decode: an error code or a result, and a result agrees with its header."""
    st, info, coef = _lib_decode(buf)
    assert st in (OK, INVALID, UNSUPPORTED), st
    try:
        ref = R.parse(buf)
        want = OK
    except R.Unsupported:
        want = UNSUPPORTED
    except R.Invalid:
        want = INVALID
    pst, pinfo = _lib_parse(buf)
    assert pst == want, (pst, want, pkg._lib.lib().yv4_last_error())
    if pst == OK:
        _same_info(pinfo, ref)
        mx, my, bw, bh, ncoef = _grid(pinfo)
        assert (pinfo.mcus_x, pinfo.mcus_y, pinfo.ncoef) == (mx, my, ncoef)
        assert list(pinfo.blocks_w)[:pinfo.ncomp] == bw and list(pinfo.blocks_h)[:pinfo.ncomp] == bh
        assert 1 <= pinfo.width <= 65535 and 1 <= pinfo.height <= 65535 and pinfo.ncomp in (1, 3)
        assert 0 < pinfo.scan_offset <= len(buf)
    if st == OK:
        assert coef.size == pinfo.ncoef
    return st


@pytest.mark.parametrize('name', SMALL)
def test_every_prefix_truncation_survives(jpeg, name):
    buf = jpeg['jpg_' + name].tobytes()
    codes = [_check_consistent(buf[:n]) for n in range(len(buf))]
    assert all(c == INVALID for c in codes[:-2])              # only a file that lost no more than its EOI still decodes
    assert codes[-1] == OK and codes[-2] == OK


@pytest.mark.parametrize('name', SMALL)
def test_every_header_byte_flip_survives(jpeg, name):
    buf = jpeg['jpg_' + name].tobytes()
    scan = R.parse(buf)['scan_offset']
    seen = set()
    for off in range(scan):
        for val in (buf[off] ^ 0xFF, (buf[off] + 1) & 0xFF, buf[off] ^ (1 << (off & 7))):
            seen.add(_check_consistent(_patched(buf, [(off, val)])))
    assert seen == {OK, INVALID, UNSUPPORTED}


def test_scan_byte_flips_survive(jpeg):
    """Flips inside the entropy-coded data: any code, never a crash, and a success leaves a whole coefficient set."""
    buf = jpeg['jpg_17x33_420_grad_q90_rst2'].tobytes()
    scan = R.parse(buf)['scan_offset']
    for off in range(scan, len(buf)):
        st, info, coef = _lib_decode(_patched(buf, [(off, buf[off] ^ (1 << (off & 7)))]))
        assert st in (OK, INVALID)


def test_layout_and_reconstruct_validate_without_a_gpu(jpeg):
    """``yv4_jpeg_layout`` is host arithmetic; ``yv4_jpeg_reconstruct`` refuses a table that leaves its buffers before
    any launch (the kernels trust the table)."""
    L = pkg._lib.lib()
    bufs = [jpeg['jpg_' + n].tobytes() for n in ('9x7_420_grad_q90', '48x64_444_noise_q90', '17x33_gray_grad_q90')]
    infos = (pkg._lib.JpegInfo * 3)()
    for i, b in enumerate(bufs):
        assert L.yv4_jpeg_parse(b, len(b), ctypes.byref(infos[i])) == OK
    table = (pkg._lib.JpegImage * 3)()
    totals = (ctypes.c_int64 * 3)()
    assert L.yv4_jpeg_layout(infos, 3, table, totals) == OK
    assert totals[0] == sum(i.ncoef for i in infos)
    assert [t.coef_off for t in table] == [0, infos[0].ncoef, infos[0].ncoef + infos[1].ncoef]
    assert [t.unit_base for t in table] == [0, 1, 1 + (3 * 48 + 31) // 32] and [t.tile_base for t in table] == [0, 3, 15]
    assert [t.out_pitch for t in table] == [21, 192, 99] and all(t.out_off % 256 == 0 for t in table)
    assert totals[2] >= table[2].out_off + 17 * 33 * 3
    fake = ctypes.c_void_p(1 << 20)             # never dereferenced: validation returns first

    def recon(tbl, coef_elems=totals[0], work=totals[1], out=totals[2]):
        return L.yv4_jpeg_reconstruct(tbl, fake, 3, fake, coef_elems, fake, fake, work, fake, out, 0, None)
    assert recon(table, out=totals[2] - 256) == INVALID and b'output buffer' in L.yv4_last_error()
    assert recon(table, work=table[2].plane_off[0]) == INVALID and b'workspace' in L.yv4_last_error()
    assert recon(table, coef_elems=totals[0] - 1) == INVALID and b'coefficients' in L.yv4_last_error()
    for field, val in (('out_pitch', 20), ('width', 65), ('hs', 3), ('coef_off', 32), ('unit_base', 5), ('out_off', -1)):
        bad = (pkg._lib.JpegImage * 3).from_buffer_copy(table)
        setattr(bad[0], field, val)
        assert recon(bad) == INVALID, field
    assert L.yv4_jpeg_reconstruct(table, None, 3, fake, 1, fake, fake, 1, fake, 1, 0, None) == INVALID


def test_registry_builds_load_image_from_file_from_the_reference_dicts():
    """The ``LoadImageFromFile`` entries of configs/yolov4/*.py and configs/yolo/*.py."""
    for cfg in (dict(type='LoadImageFromFile'), dict(type='LoadImageFromFile', im_decode_backend='turbojpeg'),
                dict(type='LoadImageFromFile', to_float32=True),
                dict(type='LoadImageFromFile', to_float32=False, color_type='color', file_client_args=dict(backend='disk'))):
        t = pkg.PIPELINES.build(cfg)
        assert isinstance(t, pkg.LoadImageFromFile) and t.to_float32 == cfg.get('to_float32', False)
        assert t.color_type == 'color' and t.file_client_args == dict(backend='disk')
    with pytest.raises(NotImplementedError):
        pkg.PIPELINES.build(dict(type='LoadImageFromFile', color_type='grayscale'))
    with pytest.raises(NotImplementedError):
        pkg.PIPELINES.build(dict(type='LoadImageFromFile', file_client_args=dict(backend='petrel')))


def test_imdecode_refuses_other_formats_by_name(tmp_path):
    png = b'\x89PNG\r\n\x1a\n' + b'\x00\x00\x00\rIHDR' + bytes(17)
    with pytest.raises(NotImplementedError, match='PNG'):
        pkg.imdecode(png)
    with pytest.raises(NotImplementedError, match='PNG'):
        pkg.imdecode([png, png])
    p = tmp_path / 'x.png'
    p.write_bytes(png)
    with pytest.raises(NotImplementedError, match='PNG'):
        pkg.imread(p)
    with pytest.raises(NotImplementedError, match='GIF'):
        pkg.imdecode(b'GIF89a' + bytes(20))
    with pytest.raises(NotImplementedError, match='WebP'):
        pkg.imdecode(b'RIFF\x00\x00\x00\x00WEBPVP8 ')
    with pytest.raises(NotImplementedError, match='unknown'):
        pkg.imdecode(bytes(32))
    assert image_io.image_format(b'\xff\xd8\xff\xe0') == 'JPEG'
    assert image_io.MAX_DECODE_THREADS == 16
