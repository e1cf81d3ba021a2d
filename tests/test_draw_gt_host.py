"""Boxes without a score on the CPU: the kernel's per-pixel function (``yv4_draw_boxes_host_ex`` with
``YV4_DRAW_NO_SCORE``) against the numpy restatement (tests/_draw_gt_ref.py), and ``flags = 0`` against the call it
extends."""
import ctypes as C

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import draw as DR

import _draw_data as D
import _draw_gt_data as G
import _draw_gt_ref as GR
import _draw_ref as R


@pytest.mark.parametrize('name', sorted(G.cases()))
def test_host_twin_equals_the_restatement(name):
    img, boxes, labels, names, style = G.cases()[name]
    got = DR.draw_boxes_host(img, boxes, labels, names, **style)
    np.testing.assert_array_equal(got, GR.draw_gt(img, boxes, labels, names, **style))
    # no box is skipped, whatever the threshold
    np.testing.assert_array_equal(DR.draw_boxes_host(img, boxes, labels, names, score_thr=2.0, **style), got)


def test_the_label_is_the_name_alone():
    img = D.image(30, 120, 31)
    box = np.array([[2.0, 2.0, 110.0, 25.0]], np.float32)
    bare = DR.draw_boxes_host(img, box, [2], D.NAMES)
    scored = DR.draw_boxes_host(img, np.concatenate([box, [[0.5]]], 1).astype(np.float32), [2], D.NAMES, score_thr=0.0)
    np.testing.assert_array_equal(scored, R.draw(img, np.concatenate([box, [[0.5]]], 1), [2], D.NAMES, score_thr=0.0))
    width = 1 + 6 * len('car')                                   # the label's columns without '|0.50'
    np.testing.assert_array_equal(bare[2:11, 2:2 + width], scored[2:11, 2:2 + width])
    assert (bare[2:11, 2 + width:2 + width + 30] != scored[2:11, 2 + width:2 + width + 30]).any()


@pytest.mark.parametrize('name', sorted(D.cases()))
def test_flags_zero_is_the_call_it_extends(name):
    img, dets, labels, names, style = D.cases()[name]
    lib = pkg._lib.lib()
    st = DR._style(len(names), style.get('score_thr', 0.3), style.get('bbox_color', (72, 101, 241)),
                   style.get('text_color', (72, 101, 241)), style.get('thickness', 2), style.get('font_size', 13))
    d = np.ascontiguousarray(dets, np.float32)
    lab = np.ascontiguousarray(labels, np.int32)
    table, total = DR._tables([(img.shape[0], img.shape[1], 0, 3 * img.shape[1])], [len(d)])
    nt = DR.name_table(names)
    a, b = img.copy(), img.copy()
    assert lib.yv4_draw_boxes_host(table, 1, a.ctypes.data, a.size, d.ctypes.data, lab.ctypes.data, total, nt.ctypes.data,
                                   C.byref(st)) == 0
    assert lib.yv4_draw_boxes_host_ex(table, 1, b.ctypes.data, b.size, d.ctypes.data, lab.ctypes.data, total, nt.ctypes.data,
                                      C.byref(st), 0) == 0
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, R.draw(img, dets, labels, names, **style))
    # an unknown flag is refused and nothing is drawn
    c = img.copy()
    assert lib.yv4_draw_boxes_host_ex(table, 1, c.ctypes.data, c.size, d.ctypes.data, lab.ctypes.data, total, nt.ctypes.data,
                                      C.byref(st), 2) == -1
    np.testing.assert_array_equal(c, img)


def test_mixed_box_widths_are_refused():
    with pytest.raises(ValueError, match='all'):
        DR._box_width([np.zeros((1, 4), np.float32), np.zeros((1, 5), np.float32)])
    with pytest.raises(ValueError, match='all'):
        DR.draw_boxes_host(D.image(8, 8, 1), np.zeros((1, 6), np.float32), [0], D.NAMES)
