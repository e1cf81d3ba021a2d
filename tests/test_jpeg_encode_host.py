"""The JPEG encoder without a GPU: the numpy restatement against libjpeg-turbo's files, the fixture's coverage, the
library's CPU form (the core the kernels run) against both seams, and the table's validation.  Nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io as io

import _jpeg_enc_data as D
import _jpeg_enc_ref as E


@pytest.fixture(scope='module')
def cases(golden):
    return D.load_cases(golden)


def test_restatement_gives_libjpeg_turbos_files(cases):
    names, srcs, jpgs, quals, samps = cases
    for name, src, jpg, q, s in zip(names, srcs, jpgs, quals, samps):
        assert E.encode(src, q, s, 'rgb') == jpg, name


def test_restatement_channel_order(cases):
    names, srcs, jpgs, quals, samps = cases
    k = names.index('37x53_420_grad_q90')
    assert E.encode(np.ascontiguousarray(srcs[k][..., ::-1]), quals[k], samps[k], 'bgr') == jpgs[k]


def test_fixture_covers_the_rules(cases):
    names, srcs, jpgs, quals, samps = cases
    pads, zrl, stuffed, last63, dummy_col, dummy_row, most = set(), 0, 0, 0, 0, 0, 0
    for src, q, s in zip(srcs, quals, samps):
        planes, hs, vs = E.coefficients(src, q, s, 'rgb')
        stats = {}
        E.scan_bytes(planes, hs, vs, stats)
        pads.add(stats['pad'])
        zrl += stats['zrl']
        stuffed += stats['stuffed']
        last63 += stats['last63']
        most = max(most, stats['blocks'])
        h, w = src.shape[:2]
        dummy_col += planes[0].shape[1] > -(-w // 8)
        dummy_row += planes[0].shape[0] > -(-h // 8)
    assert pads == set(range(8))
    assert zrl and stuffed and last63 and dummy_col and dummy_row
    assert set(samps) == {'444', '422', '420', 'gray'} and {1, 30, 50, 75, 90, 95, 100} <= set(quals)
    assert most == 918 and most > pkg._lib.JPEG_ENC_WG_BLOCKS      # more than one workgroup of the bit-offset scan


def test_quality_tables_and_header(cases):
    for q in (1, 5, 30, 49, 50, 51, 75, 95, 100):
        et = io.EncodeTable([(8, 8, 3)], q, '444')
        for t in range(2):
            assert list(et.table[0].quant[t]) == E.quant_table(t, q)
    for shape, s in (((37, 53, 3), '420'), ((37, 53, 3), '422'), ((1, 1, 3), '444'), ((23, 130), 'gray')):
        et = io.EncodeTable([shape], 77, s)
        assert et.header(0) == E.header(shape[1], shape[0], 77, s)
        assert len(et.header(0)) <= pkg._lib.JPEG_ENC_HEADER_MAX


def _host(et, stage, pix, coef, work, out, sizes, rgb=1):
    return pkg._lib.lib().yv4_jpeg_encode_host(et.table, len(et), stage, pix.ctypes.data if pix is not None else None,
                                               pix.size if pix is not None else 0, rgb, coef.ctypes.data, coef.size,
                                               work.ctypes.data if work is not None else None,
                                               work.size if work is not None else 0,
                                               out.ctypes.data if out is not None else None,
                                               out.size if out is not None else 0,
                                               sizes.ctypes.data if sizes is not None else None)


def test_cpu_form_per_case_at_both_seams_behind_guards(cases):
    """Per case, every buffer behind guard bytes and the input at a wider pitch: stage 1's coefficients equal the host
    decoder's for libjpeg-turbo's file; stage 2 FROM THOSE gives the file's scan bytes; header + scan + EOI is the
    file."""
    names, srcs, jpgs, quals, samps = cases
    for name, src, jpg, q, s in zip(names, srcs, jpgs, quals, samps):
        et = io.EncodeTable([src.shape], q, s)
        npix, ncoef, nwork, nout = D.spread(et)
        t = et.table[0]
        pix = D.place_pixels(et, [src], npix)
        coef = np.full(ncoef, GUARD16, np.int16)
        assert _host(et, 1, pix, coef, None, None, None) == 0, pkg._lib.lib().yv4_last_error()
        info, want = io.jpeg_entropy_decode(jpg)
        lo, hi = int(t.coef_off), int(t.coef_off + t.nblocks * 64)
        assert hi - lo == want.size, name
        np.testing.assert_array_equal(coef[lo:hi], want, err_msg=name)
        D.assert_guards(coef.view(np.uint8), [(2 * lo, 2 * (hi - lo))], name + ' coefficients')

        coef2 = np.full(ncoef, GUARD16, np.int16)
        coef2[lo:hi] = want
        work = np.full(nwork // 8 + 1, GUARD64, np.uint64).view(np.uint8)
        out = np.full(nout, D.GUARD_BYTE, np.uint8)
        sizes = np.zeros(1, np.int64)
        assert _host(et, 2, None, coef2, work, out, sizes) == 0, pkg._lib.lib().yv4_last_error()
        head = et.header(0)
        scan = out[t.out_off:t.out_off + int(sizes[0])].tobytes()
        assert scan == jpg[len(head):-2], name
        assert head + scan + b'\xff\xd9' == jpg, name
        D.assert_guards(out, [(int(t.out_off), int(sizes[0]))], name + ' output')
        D.assert_guards(work, [(int(t.work_off), et.work_region_bytes(0))], name + ' workspace')


GUARD16 = np.int16(0x5A5A)
GUARD64 = np.uint64(0x5A5A5A5A5A5A5A5A)


def test_cpu_form_batch_equals_single_calls(cases):
    names, srcs, jpgs, quals, samps = cases
    et, coef, out, sizes = io.jpeg_encode_host(srcs, quals, samps, 'rgb')
    assert et.files(out, sizes) == jpgs
    bgr = [np.ascontiguousarray(a[..., ::-1]) if a.ndim == 3 else a for a in srcs]
    et, coef, out, sizes = io.jpeg_encode_host(bgr, quals, samps, 'bgr')
    assert et.files(out, sizes) == jpgs


def test_layout_refuses_bad_tables_before_anything_runs():
    L = pkg._lib.lib()

    def table(**kw):
        et = io.EncodeTable([(37, 53, 3), (16, 24)], [90, 50], ['420', 'gray'])
        for k, v in kw.items():
            setattr(et.table[1 if k.endswith('1') else 0], k.rstrip('1'), v)
        return et

    def validate(et, pix=None, coef=None, work=None, out=None):
        return L.yv4_jpeg_encode_validate(et.table, len(et), et.pixel_bytes if pix is None else pix,
                                          et.ncoef if coef is None else coef, et.work_bytes if work is None else work,
                                          et.out_bytes if out is None else out)

    assert validate(table()) == 0
    for bad, word in ((dict(quality=0), b'quality'), (dict(quality=101), b'quality'), (dict(src_pitch=3 * 53 - 1), b'pitch'),
                      (dict(src_off=-1), b'pixels'), (dict(coef_off=32), b'coefficients'), (dict(work_off=4), b'work'),
                      (dict(out_cap=100), b'bound'), (dict(wg_base1=0), b'workgroup'), (dict(mcus_x=9), b'grids'),
                      (dict(width=70), b'grids'), (dict(hs=1, vs=2), b'sampling')):
        et = table(**bad)
        assert validate(et) == -1, bad
        assert word in L.yv4_last_error(), (bad, L.yv4_last_error())
        # ... and the CPU form makes the same check before it writes anything
        coef = np.full(et.ncoef, GUARD16, np.int16)
        pix = np.zeros(et.pixel_bytes, np.uint8)
        assert _host(et, 1, pix, coef, None, None, None) == -1
        assert (coef == GUARD16).all()
    good = table()
    for kw, word in ((dict(pix=good.pixel_bytes - 300), b'pixels'), (dict(coef=good.ncoef - 1), b'coefficients'),
                     (dict(work=good.work_bytes - 300), b'work'), (dict(out=good.out_bytes - 300), b'output')):
        assert validate(good, **kw) == -1 and word in L.yv4_last_error(), (kw, L.yv4_last_error())
    # a batch whose stuffing grid would pass 2^24 workgroups is refused, not launched
    big = io.EncodeTable([(60000, 60000, 3)], 90, '444')
    assert L.yv4_jpeg_encode_validate(big.table, 1, 1 << 60, 1 << 60, 1 << 60, 1 << 60) == -1
    assert b'too large' in L.yv4_last_error()
    totals = (C.c_int64 * 6)()
    for field, v, word in (('quality', 0, b'quality'), ('quality', 101, b'quality'), ('width', 0, b'empty'),
                           ('height', 65536, b'65535'), ('hs', 4, b'sampling'), ('channels', 2, b'channels')):
        tab = (pkg._lib.JpegEncImage * 1)()
        tab[0].width, tab[0].height, tab[0].channels, tab[0].hs, tab[0].vs, tab[0].quality = 8, 8, 3, 2, 2, 90
        setattr(tab[0], field, v)
        assert L.yv4_jpeg_encode_layout(tab, 1, totals) == -1 and word in L.yv4_last_error(), (field, L.yv4_last_error())


def test_python_arguments_are_refused_by_name():
    for kw, word in ((dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=90.0), 'quality'),
                     (dict(subsampling='411'), 'subsampling'), (dict(subsampling='gray'), 'gray')):
        with pytest.raises(ValueError, match=word):
            io.EncodeTable([(8, 8, 3)], **kw)
    for shape, word in (((0, 8, 3), 'empty'), ((8, 65536, 3), '65535'), ((8, 8, 4), 'shape')):
        with pytest.raises(ValueError, match=word):
            io.EncodeTable([shape])
    with pytest.raises(NotImplementedError, match='PNG'):
        pkg.imwrite(np.zeros((8, 8, 3), np.uint8), 'a.png')
    with pytest.raises(NotImplementedError, match='JPEG'):
        pkg.imwrite([np.zeros((8, 8, 3), np.uint8)] * 2, ['a.JPG', 'b.tiff'])
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pkg.imencode(np.zeros((8, 8, 3), np.uint8))
