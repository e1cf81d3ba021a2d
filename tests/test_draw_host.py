"""The drawing rule without a GPU: the numpy restatement on hand-made cases, and the library's per-pixel function on the
CPU (the one the kernel runs) against it, bit for bit."""
import numpy as np
import pytest

from mmdet_yolov4_amd import draw as draw_mod

import _draw_data as D
import _draw_ref as R

BITMAPS = {
    '0': ['.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'],
    '1': ['..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'],
    '|': ['..#..', '..#..', '..#..', '..#..', '..#..', '..#..', '..#..'],
    '.': ['.....', '.....', '.....', '.....', '.....', '.##..', '.##..'],
    '?': ['.###.', '#...#', '....#', '...#.', '..#..', '.....', '..#..'],
}
COLOR = np.array((72, 101, 241), np.uint8)


def test_glyphs_against_bitmaps_written_here():
    for ch, rows in BITMAPS.items():
        want = np.array([[c == '#' for c in r] for r in rows])
        np.testing.assert_array_equal(R.glyph(ord(ch)), want, err_msg=ch)


def test_label_text_rounds_in_float32():
    assert R.label_text('car', 0.87) == b'car|0.87'
    assert R.label_text('car', 1.0) == b'car|1.00'
    assert R.label_text('car', 0.004) == b'car|0.00'
    assert R.label_text('car', 0.005) == b'car|0.01'      # 0.005f * 100 + 0.5 = 1.0000000 in float32
    assert R.label_text('tr\xe4in\n', 0.5) == b'tr??in?|0.50'
    assert len(R.label_text('x' * 50, 0.5)) == 31 + 5


def test_box_clipped_at_each_border():
    # (-10, -7) .. (25, 20) in a 40 x 60 image: the left and top edges lie outside; the 9-row label starts at (-10, -7), so
    # its last two rows are the image's rows 0 and 1, out to column -10 + 1 + 6 * 11 = 57
    img, dets, labels, names, style = D.cases()['clipped_left_top']
    out = R.draw(img, dets, labels, names, **style)
    assert (out[19:21, :26] == COLOR).all()                                     # bottom edge: rows 19, 20 (y2 = 20)
    assert (out[2:19, 24:26] == COLOR).all()                                    # right edge: columns 24, 25 (x2 = 25)
    np.testing.assert_array_equal(out[2:19, 0:24], img[2:19, 0:24])             # the inside
    np.testing.assert_array_equal(out[21:], img[21:])
    np.testing.assert_array_equal(out[2:, 26:], img[2:, 26:])
    np.testing.assert_array_equal(out[:2, 57:], img[:2, 57:])
    lab = out[:2, :57]
    assert ((lab == COLOR).all(2) | (lab == img[:2, :57] // 5).all(2)).all()
    # (30, 18) .. (90, 70): the right and bottom edges lie outside; the label covers rows 18 .. 26 from column 30 on
    img, dets, labels, names, style = D.cases()['clipped_right_bottom']
    out = R.draw(img, dets, labels, names, **style)
    assert (out[27:, 30:32] == COLOR).all()                                     # left edge below the label
    np.testing.assert_array_equal(out[:18], img[:18])
    np.testing.assert_array_equal(out[:, :30], img[:, :30])
    np.testing.assert_array_equal(out[27:, 32:], img[27:, 32:])
    img, dets, labels, names, style = D.cases()['outside']
    np.testing.assert_array_equal(R.draw(img, dets, labels, names, **style), img)


def test_thickness_larger_than_the_box_fills_it():
    # (50, 2) .. (56, 25), thickness 9: seven columns wide, so every pixel of the rectangle is frame; rows 2 .. 10 are label
    img, dets, labels, names, style = D.cases()['thick_box']
    out = R.draw(img, dets, labels, names, **style)
    assert (out[11:26, 50:57] == COLOR).all()
    changed = (out != img).any(2)
    assert not changed[:2].any() and not changed[26:].any() and not changed[:, :50].any() and not changed[11:, 57:].any()


def test_two_overlapping_boxes_the_later_wins():
    # box 0: (5, 5) .. (60, 40); box 1: (20, 8) .. (90, 60), its label over rows 8 .. 16, columns 20 .. 68
    img, dets, labels, names, style = D.cases()['later_wins']
    out = R.draw(img, dets, labels, names, **style)
    only0 = R.draw(img, dets[:1], labels[:1], names, **style)
    green, text = np.array((0, 255, 0), np.uint8), np.array((1, 2, 3), np.uint8)
    assert (out[30, 20:22] == green).all() and (only0[30, 20:22] == img[30, 20:22]).all()     # box 1's left edge inside box 0
    assert (out[30, 59:61] == green).all() and (out[40, 30] == green).all()                     # box 0's edges outside box 1's
    assert (only0[14:17, 59:61] == green).all()                      # box 0's right edge below its own label ...
    lab = out[8:17, 20:69]                                           # ... lies under box 1's label
    assert ((lab == text).all(2) | (lab == img[8:17, 20:69] // 5).all(2)).all()
    assert (out[8, 70] == green).all() and not (only0[8, 70] == green).all()      # box 1's top edge over box 0's label


def test_score_equal_to_the_threshold_is_not_drawn():
    img, dets, labels, names, style = D.cases()['at_threshold']
    out = R.draw(img, dets, labels, names, **style)
    only_second = R.draw(img, dets[1:], labels[1:], names, **style)
    np.testing.assert_array_equal(out, only_second)
    assert (out != img).any()
    np.testing.assert_array_equal(R.draw(img, dets[:1], labels[:1], names, **style), img)


def test_label_pixels():
    img, dets, labels, names, style = D.cases()['scaled_font']
    out = R.draw(img, dets, labels, names, **style)
    text = R.label_text('car', 0.995)
    assert text == b'car|1.00'
    mask = R.text_mask(text, 3)
    region = out[3:3 + 27, 3:3 + mask.shape[1]]
    np.testing.assert_array_equal(region[mask], np.full((mask.sum(), 3), 255, np.uint8))
    np.testing.assert_array_equal(region[~mask], img[3:30, 3:3 + mask.shape[1]][~mask] // 5)


@pytest.mark.parametrize('name', sorted(D.cases()))
def test_library_cpu_form_equals_the_restatement(name):
    img, dets, labels, names, style = D.cases()[name]
    got = draw_mod.draw_boxes_host(img, dets, labels, names, **style)
    np.testing.assert_array_equal(got, R.draw(img, dets, labels, names, **style))


def test_library_cpu_form_on_the_batch_images():
    imgs, dets, labels = D.batch()
    for img, d, lab in zip(imgs, dets, labels):
        np.testing.assert_array_equal(draw_mod.draw_boxes_host(img, d, lab, D.NAMES, score_thr=0.3),
                                      R.draw(img, d, lab, D.NAMES, score_thr=0.3))


def test_a_name_byte_outside_the_glyph_table_reads_as_a_question_mark():
    """The library itself, not only ``name_table``: a table made elsewhere with bytes outside 0x20 .. 0x7E never indexes
    the glyph table outside."""
    import ctypes as C
    from mmdet_yolov4_amd import _lib
    img = D.image(24, 120, 31)
    dets = np.array([[2.0, 2.0, 110.0, 20.0, 0.75]], np.float32)
    labels = np.zeros(1, np.int32)
    names = draw_mod.name_table(['ab?de?g'])
    names[0, 3], names[0, 6] = 0x07, 0xF3
    out = img.copy()
    st = draw_mod._style(1, 0.3, (72, 101, 241), (72, 101, 241), 2, 13)
    table, total = draw_mod._tables([(24, 120, 0, 360)], [1])
    assert _lib.lib().yv4_draw_boxes_host(table, 1, out.ctypes.data, out.size, dets.ctypes.data, labels.ctypes.data, 1,
                                          names.ctypes.data, C.byref(st)) == 0
    np.testing.assert_array_equal(out, R.draw(img, dets, [0], ['ab?de?g']))


def test_arguments():
    assert draw_mod.color_val('red') == (0, 0, 255) and draw_mod.color_val((1, 2, 3)) == (1, 2, 3)
    for bad in ('purple', (1, 2), (0, 0, 256)):
        with pytest.raises(ValueError):
            draw_mod.color_val(bad)
    with pytest.raises(ValueError, match='thickness'):
        draw_mod.draw_boxes_host(np.zeros((4, 4, 3), np.uint8), np.zeros((0, 5)), [], ['a'], thickness=0)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            draw_mod.draw_boxes_into(torch.zeros(48, dtype=torch.uint8), [(4, 4, 0, 12)], [torch.zeros(0, 5)],
                                     [torch.zeros(0)], ['a'])
