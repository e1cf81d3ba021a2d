"""The device Huffman decode without a GPU: ``yv4_jpeg_scan_prepare``'s segment table, and the decode core the kernel
runs (``csrc/jpeg_entropy_core.h``) run on the CPU over the same tables (``yv4_jpeg_entropy_decode_segments``) against
the host decoder ``yv4_jpeg_entropy_decode``, the oracle -- every coefficient of every file of ``jpeg.npz`` and
``jpeg_entropy.npz``, and the same status class for every damaged one."""
import ctypes

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -4
L = pkg._lib


@pytest.fixture(scope='module')
def cases(golden):
    """-> (valid: name -> bytes over both fixtures, damaged: name -> (bytes, recorded status), refused: name -> bytes)"""
    a, b = golden('jpeg'), golden('jpeg_entropy')
    valid = {str(n): a['jpg_' + str(n)].tobytes() for n in a['names']}
    valid.update({str(n): b['jpg_' + str(n)].tobytes() for n in b['names']})
    damaged = {str(n): (b['jpg_' + str(n)].tobytes(), int(b['status_' + str(n)])) for n in b['damaged']}
    refused = {str(n): a['jpg_' + str(n)].tobytes() for n in a['refused']}
    return valid, damaged, refused


def _host(buf):
    """The oracle -> (status, info, coefficients)."""
    info = L.JpegInfo()
    st = L.lib().yv4_jpeg_parse(buf, len(buf), ctypes.byref(info))
    if st != OK:
        return st, info, None
    coef = np.empty(int(info.ncoef), np.int16)
    st = L.lib().yv4_jpeg_entropy_decode(buf, len(buf), ctypes.byref(info), coef.ctypes.data, coef.size)
    return st, info, coef


def _segments(buf):
    """prepare + the CPU run of the kernel's core -> (status class, tables or None, coefficients or None)."""
    try:
        t, coef, status = image_io.jpeg_entropy_decode_segments([buf])
    except NotImplementedError:
        return UNSUPPORTED, None, None
    except ValueError:
        return INVALID, None, None
    return (INVALID if status[0] else OK), t, coef


def test_abi_exports_the_entropy_entries():
    names = ('yv4_jpeg_scan_prepare', 'yv4_jpeg_entropy_workgroups', 'yv4_jpeg_entropy_decode_segments',
             'yv4_jpeg_entropy_decode_device', 'yv4_jpeg_entropy_strerror')
    assert set(names) == set(L.FEATURES['jpeg_entropy'].symbols) and set(names) <= set(L.SIGNATURES)
    assert all(hasattr(L.lib(), n) for n in names) and L.has('jpeg_entropy')
    assert L.lib().yv4_abi_version() == 8
    assert (ctypes.sizeof(L.JpegHuff), ctypes.sizeof(L.JpegScan), ctypes.sizeof(L.JpegSegment), ctypes.sizeof(L.JpegWg)) == \
        (1344, 96, 40, 16)
    assert L.JpegScan.nseg.offset == 40 and L.JpegScan.td.offset == 64 and L.JpegSegment.pred.offset == 32
    assert b'restart marker' in L.lib().yv4_jpeg_entropy_strerror(5) and b'unknown' in L.lib().yv4_jpeg_entropy_strerror(6)


def test_fixture_covers_the_cases(cases):
    valid, damaged, refused = cases
    assert len(valid) == 79 + 5 and len(refused) == 2 and sorted(damaged) == ['cut_last', 'cut_mid', 'inserted', 'removed', 'swapped']
    t = image_io.ScanTables([valid['72x80_444_grad_q90_rst1'], valid['72x80_420_grad_q90_rst1'],
                             valid['72x80_444_noise_q100_rst1'], valid['8x8_gray_block_q90']])
    assert [s.nseg for s in t.scans] == [90, 25, 90, 1] and t.nseg == 206
    assert [(w.image, w.first_seg, w.count) for w in t.wgs] == [(0, 0, 64), (0, 64, 26), (1, 0, 25), (2, 0, 64), (2, 64, 26),
                                                                (3, 0, 1)]
    noise = valid['72x80_444_noise_q100_rst1']
    scan = t.infos[2].scan_offset
    assert sum(noise[i] == 0xFF and noise[i + 1] == 0 for i in range(scan, len(noise) - 1)) >= 100      # stuffed pairs
    assert np.abs(_host(noise)[2]).max() >= 512                                                           # 10-bit magnitudes


def test_segment_table_of_every_file(cases):
    """Count, MCU ranges, and the byte ranges: each starts behind the previous one's marker and ends where the next
    marker (fill bytes included) or the scan's end stands."""
    valid = cases[0]
    for name, buf in valid.items():
        t = image_io.ScanTables([buf])
        f, sc = t.infos[0], t.scans[0]
        total, ri = f.mcus_x * f.mcus_y, f.restart_interval
        want = -(-total // ri) if ri else 1
        assert (sc.nseg, t.nseg, sc.seg_base, sc.data_off, sc.data_len, sc.ncoef) == (want, want, 0, 0, len(buf), f.ncoef), name
        assert (sc.ncomp, sc.mcus_x, sc.mcus_y, sc.hs, sc.vs) == (f.ncomp, f.mcus_x, f.mcus_y, f.hs[0], f.vs[0])
        assert 1 <= sc.nhuff <= 6 and all(0 <= sc.td[i] < sc.nhuff and 0 <= sc.ta[i] < sc.nhuff for i in range(f.ncomp))
        assert t.segs[0].begin == f.scan_offset
        for s, g in enumerate(t.segs):
            assert g.first_mcu == s * (ri or total) and g.mcu_count == min(ri or total, total - g.first_mcu), (name, s)
            assert (g.bit_off, g.reserved, list(g.pred)) == (0, 0, [0, 0, 0, 0])
            data = buf[g.begin:g.end]
            assert b'\xff' not in data.replace(b'\xff\x00', b''), (name, s)      # nothing but data and stuffed pairs inside
            if s + 1 < want:
                gap = buf[g.end:t.segs[s + 1].begin]
                assert gap.lstrip(b'\xff') == bytes([0xD0 + (s & 7)]) and gap[:1] == b'\xff', (name, s)
            else:
                assert buf[g.end:g.end + 2] == b'\xff\xd9', name
    t = image_io.ScanTables([valid['72x80_444_grad_q90_rst1_fill']])
    assert t.segs[38].begin - t.segs[37].end == 4


def test_core_on_the_cpu_equals_the_host_decoder_in_every_coefficient(cases):
    valid = cases[0]
    for name, buf in valid.items():
        st, info, want = _host(buf)
        assert st == OK, name
        st, t, got = _segments(buf)
        assert st == OK, (name, pkg._lib.lib().yv4_last_error())
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_a_batch_on_the_cpu_equals_the_single_files(cases):
    valid = cases[0]
    names = list(valid)[::7] + ['72x80_444_grad_q90_rst1', '8x8_gray_block_q90', '72x80_420_grad_q90_rst1']
    t, coef, status = image_io.jpeg_entropy_decode_segments([valid[n] for n in names])
    assert not status.any() and [s.seg_base for s in t.scans] == list(np.cumsum([0] + [s.nseg for s in t.scans])[:-1])
    for n, sc in zip(names, t.scans):
        np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], _host(valid[n])[2], err_msg=n)


def test_damaged_files_fail_in_both_with_the_same_class(cases):
    valid, damaged, _ = cases
    for name, (buf, recorded) in damaged.items():
        assert _host(buf)[0] == recorded == INVALID, name
        assert _segments(buf)[0] == recorded, name
    # where the failure is found: the marker rules in prepare, what only the bits show in the decode
    for name in ('swapped', 'removed', 'cut_mid'):
        with pytest.raises(ValueError, match='restart marker'):
            image_io.ScanTables([damaged[name][0]])
    codes = {}
    for name in ('cut_last', 'inserted'):
        t, coef, status = image_io.jpeg_entropy_decode_segments([valid['8x8_gray_block_q90'], damaged[name][0]])
        assert status[0] == 0
        codes[name] = int(status[1])
    assert codes == dict(cut_last=1, inserted=5)


def test_every_prefix_and_scan_byte_flip_gives_the_host_decoders_class(cases):
    """Two small restart files: every truncation, and one bit of every byte of the scan flipped -- the class of the
    outcome, and on success every coefficient, equal the host decoder's."""
    valid = cases[0]
    seen = set()
    for name in ('17x33_420_grad_q90_rst2', '9x7_420_grad_q90'):
        buf = valid[name]
        scan = _host(buf)[1].scan_offset
        variants = [buf[:n] for n in range(len(buf))]
        for off in range(scan, len(buf)):
            b = bytearray(buf)
            b[off] ^= 1 << (off & 7)
            variants.append(bytes(b))
        for v in variants:
            st, _, want = _host(v)
            got_st, _, got = _segments(v)
            assert got_st == st, (name, len(v))
            seen.add(st)
            if st == OK:
                np.testing.assert_array_equal(got, want)
    assert seen == {OK, INVALID}


def test_refused_files_are_unsupported_in_both(cases):
    for name, buf in cases[2].items():
        assert _host(buf)[0] == UNSUPPORTED and _segments(buf)[0] == UNSUPPORTED, name
        info, scan = L.JpegInfo(), L.JpegScan()
        huff, segs = (L.JpegHuff * 6)(), (L.JpegSegment * 1)()
        assert L.lib().yv4_jpeg_scan_prepare(buf, len(buf), ctypes.byref(info), ctypes.addressof(scan), ctypes.addressof(huff),
                                             ctypes.addressof(segs), 1) == UNSUPPORTED


def test_prepare_checks_its_capacity(cases):
    buf = cases[0]['72x80_420_grad_q90_rst1']
    info, scan = L.JpegInfo(), L.JpegScan()
    huff, segs = (L.JpegHuff * 6)(), (L.JpegSegment * 25)()
    args = (buf, len(buf), ctypes.byref(info), ctypes.addressof(scan), ctypes.addressof(huff), ctypes.addressof(segs))
    assert L.lib().yv4_jpeg_scan_prepare(*args, 24) == CAPACITY and scan.nseg == 25 and segs[0].end == 0
    assert L.lib().yv4_jpeg_scan_prepare(*args, 25) == OK and segs[24].first_mcu == 24


def test_tables_that_leave_the_buffers_are_refused_without_a_gpu(cases):
    """``yv4_jpeg_entropy_decode_device`` validates the host tables before any launch (the kernel trusts the device
    copies): with a bad table it returns before it touches the device or a pointer."""
    valid = cases[0]
    bufs = [valid['72x80_444_grad_q90_rst1'], valid['17x33_gray_grad_q90'], valid['72x80_420_grad_q90_rst1']]
    good = image_io.ScanTables(bufs)
    fake = ctypes.c_void_p(1 << 20)             # never dereferenced: validation returns first

    def call(t, nbytes=good.nbytes, ncoef=good.ncoef, nhuff=good.nhuff, nseg=good.nseg, nwg=good.nwg):
        return L.lib().yv4_jpeg_entropy_decode_device(
            ctypes.addressof(t.scans), ctypes.addressof(t.segs), ctypes.addressof(t.wgs), fake, fake, fake, 3, nseg, nwg,
            fake, nbytes, fake, nhuff, fake, ncoef, fake, None)

    err = L.lib().yv4_last_error
    assert call(good, nbytes=good.nbytes - 8) == INVALID and b'byte buffer' in err()
    assert call(good, ncoef=good.ncoef - 1) == INVALID and b'coefficients' in err()
    assert call(good, nhuff=good.nhuff - 1) == INVALID and b'Huffman tables' in err()
    assert call(good, nseg=good.nseg - 1) == INVALID and call(good, nwg=good.nwg + 1) == INVALID
    for where, field, val in (('scans', 'data_off', -1), ('scans', 'data_len', 1 << 40), ('scans', 'coef_off', 32),
                              ('scans', 'ncoef', 64), ('scans', 'mcus_x', 11), ('scans', 'hs', 3), ('scans', 'nseg', 91),
                              ('scans', 'seg_base', 1), ('scans', 'huff_base', -1), ('scans', 'nhuff', 7),
                              ('segs', 'end', 1 << 20), ('segs', 'begin', -1), ('segs', 'first_mcu', 1),
                              ('segs', 'mcu_count', 2), ('segs', 'mcu_count', 0), ('segs', 'bit_off', 3),
                              ('wgs', 'count', 65), ('wgs', 'count', 63), ('wgs', 'first_seg', 1), ('wgs', 'image', 1)):
        bad = image_io.ScanTables(bufs)
        setattr(getattr(bad, where)[0], field, val)
        assert call(bad) == INVALID, (where, field, val)
    bad = image_io.ScanTables(bufs)
    bad.scans[0].td[0] = 6
    assert call(bad) == INVALID and b'table index' in err()
    bad = image_io.ScanTables(bufs)
    bad.segs[95].pred[1] = 7
    assert call(bad) == INVALID and b'entry state' in err()
    assert L.lib().yv4_jpeg_entropy_decode_device(ctypes.addressof(good.scans), ctypes.addressof(good.segs),
                                                  ctypes.addressof(good.wgs), fake, fake, fake, 3, good.nseg, good.nwg,
                                                  fake, good.nbytes, None, good.nhuff, fake, good.ncoef, fake, None) == INVALID


def test_entropy_setting_and_arguments():
    assert image_io.DEFAULT_ENTROPY == 'host'
    assert pkg.set_default_entropy('device') == 'host' and image_io.DEFAULT_ENTROPY == 'device'
    assert pkg.set_default_entropy('host') == 'device' and image_io.DEFAULT_ENTROPY == 'host'
    with pytest.raises(ValueError, match='entropy'):
        pkg.set_default_entropy('gpu')
    with pytest.raises(ValueError, match='entropy'):
        pkg.LoadImageFromFile(entropy='gpu')
    assert pkg.PIPELINES.build(dict(type='LoadImageFromFile', entropy='device')).entropy == 'device'
    assert pkg.LoadImageFromFile().entropy is None
