"""EXIF orientation without a GPU: the header parse (``yv4_jpeg_parse`` -> ``JpegInfo.orientation``) against
``tests/golden/jpeg_exif.npz`` (make_golden_jpeg_exif.py: Pillow-written and hand-made APP1 segments, the expected
pixels from ``ImageOps.exif_transpose``), the numpy restatement of the orientation table (``_exif_ref.py``) against the
same pixels, and the host arithmetic of the oriented layout."""
import ctypes

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
import _exif_ref as E


@pytest.fixture(scope='module')
def exif(golden):
    g = golden('jpeg_exif')
    return {k: g[k] for k in g.files}


def _cases(exif):
    return [(str(n), int(o), str(b)) for n, o, b in zip(exif['names'], exif['orientation'], exif['plain'])]


def test_fixture_holds_the_cases_the_kernel_can_get_wrong(exif):
    names = {n for n, _, _ in _cases(exif)}
    for size in ('1x1_444', '1x17_444', '17x1_444', '13x29_420', '48x64_422', '9x20_gray', '70x130_444', '5x300_420'):
        assert {f'{size}_o{o}' for o in range(1, 9)} <= names
    assert {'13x29_420_mm_o6', '13x29_420_second_o8', '13x29_420_badifd', '13x29_420_o9', '13x29_420_long'} <= names


def test_parse_reports_the_orientation_of_every_file(exif):
    for name, o, _ in _cases(exif):
        assert image_io.jpeg_parse(exif['jpg_' + name].tobytes()).orientation == o, name
    for name in ('13x29_420_badifd', '13x29_420_o9', '13x29_420_long'):      # malformed: 0, and never an error
        assert image_io.jpeg_parse(exif['jpg_' + name].tobytes()).orientation == 0


def test_big_endian_header_and_second_segment(exif):
    mm = exif['jpg_13x29_420_mm_o6'].tobytes()
    assert b'Exif\0\0MM\0\x2a' in mm and image_io.jpeg_parse(mm).orientation == 6
    two = exif['jpg_13x29_420_second_o8'].tobytes()
    assert two.count(b'Exif\0\0') == 2 and image_io.jpeg_parse(two).orientation == 8      # the first segment decides


def test_existing_fixture_files_report_no_orientation(golden):
    count = 0
    for fixture in ('jpeg', 'jpeg_entropy'):
        g = golden(fixture)
        for n in g['names']:
            assert image_io.jpeg_parse(g['jpg_' + str(n)].tobytes()).orientation == 0, n
            count += 1
    assert count == 84


def test_every_cut_of_the_app1_segment_parses_to_a_valid_orientation(exif):
    """The segment shortened byte by byte (its length field following): the orientation is the file's or 0, the rest of
    the header is unchanged, and nothing is an error."""
    buf = exif['jpg_13x29_420_mm_o6'].tobytes()
    at = buf.index(b'\xff\xe1')
    seglen = int.from_bytes(buf[at + 2:at + 4], 'big')
    want = image_io.jpeg_parse(buf)
    seen = set()
    for n in range(2, seglen + 1):
        cut = buf[:at + 2] + n.to_bytes(2, 'big') + buf[at + 4:at + 2 + n] + buf[at + 2 + seglen:]
        info = image_io.jpeg_parse(cut)
        assert info.orientation in (0, 6) and (info.width, info.height, info.ncoef) == (want.width, want.height, want.ncoef)
        seen.add(info.orientation)
    assert seen == {0, 6}


def test_numpy_orientation_table_equals_exif_transpose(exif):
    for name, o, base in _cases(exif):
        np.testing.assert_array_equal(E.orient(exif['rgb_' + base], o), exif['rgb_' + name], err_msg=name)


def test_oriented_layout_is_additive_and_swaps_the_pitch(exif):
    """``yv4_jpeg_layout`` ignores the tag; ``yv4_jpeg_layout_oriented(apply=1)`` carries it, lays 5 .. 8 out at pitch
    3 * height and gives such an image no tile of the plain pixel kernel; with apply=0 it is ``yv4_jpeg_layout``."""
    L = pkg._lib.lib()
    names = [f'13x29_420_o{o}' for o in range(1, 9)] + ['13x29_420_o9']
    N = len(names)
    infos = (pkg._lib.JpegInfo * N)(*[image_io.jpeg_parse(exif['jpg_' + n].tobytes()) for n in names])
    plain, same, orient = ((pkg._lib.JpegImage * N)() for _ in range(3))
    totals = [(ctypes.c_int64 * 3)() for _ in range(3)]
    assert L.yv4_jpeg_layout(infos, N, plain, totals[0]) == 0
    assert L.yv4_jpeg_layout_oriented(infos, N, 0, same, totals[1]) == 0
    assert L.yv4_jpeg_layout_oriented(infos, N, 1, orient, totals[2]) == 0
    assert bytes(plain) == bytes(same) and list(totals[0]) == list(totals[1]) == list(totals[2])
    tiles = 0
    for n, (p, q) in enumerate(zip(plain, orient)):
        o = n + 1 if n < 8 else 0
        assert (p.orientation, q.orientation) == (0, o)
        assert p.out_pitch == 3 * 29 and q.out_pitch == 3 * (13 if o >= 5 else 29)
        assert image_io.oriented_size(q) == ((29, 13) if o >= 5 else (13, 29))
        assert (q.out_off, q.coef_off, q.unit_base, q.width, q.height) == (p.out_off, p.coef_off, p.unit_base, 29, 13)
        assert q.tile_base == tiles
        tiles += 0 if o >= 2 else 4      # ceil(29 / 256) * ceil(13 / 4)


def test_load_image_from_file_accepts_both_colour_flags():
    a = pkg.PIPELINES.build(dict(type='LoadImageFromFile'))
    b = pkg.PIPELINES.build(dict(type='LoadImageFromFile', color_type='color_ignore_orientation'))
    c = pkg.PIPELINES.build(dict(type='LoadImageFromFile', apply_orientation=True))
    assert (a.apply_orientation, b.apply_orientation, c.apply_orientation) == (False, False, True)
    with pytest.raises(ValueError):
        pkg.PIPELINES.build(dict(type='LoadImageFromFile', color_type='color_ignore_orientation', apply_orientation=True))
