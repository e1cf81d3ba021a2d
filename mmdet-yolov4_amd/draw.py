"""Detections drawn onto images on the GPU: ``draw_boxes`` (``yv4_draw_boxes``, one launch per batch, one lane per pixel).

The rule is the package's own and is stated in ``include/yv4.h`` ("drawing detections"); ``tests/_draw_ref.py`` restates
it in numpy and the kernel equals it bit for bit.  The reference renders through matplotlib with anti-aliased text in a
system font, which cannot be reproduced: parity with its pictures is not claimed.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import DrawImage, DrawStyle, check
from .ops import stream_ptr

#: mmcv's colour names (``mmcv.visualization.color.Color``), B G R
COLORS = dict(red=(0, 0, 255), green=(0, 255, 0), blue=(255, 0, 0), cyan=(255, 255, 0), yellow=(0, 255, 255),
              magenta=(255, 0, 255), white=(255, 255, 255), black=(0, 0, 0))


def color_val(color):
    """A B G R tuple of ints in 0 .. 255, or one of mmcv's colour names -> the tuple (``mmcv.color_val``)."""
    if isinstance(color, str):
        if color not in COLORS:
            raise ValueError(f'colour {color!r} is not one of {sorted(COLORS)}')
        return COLORS[color]
    vals = tuple(int(c) for c in color)
    if len(vals) != 3 or any(not 0 <= c <= 255 for c in vals):
        raise ValueError(f'colour {color!r} is not three channels in 0 .. 255')
    return vals


def name_table(class_names):
    """The class names as the kernel reads them: ``(len + 1, DRAW_NAME_BYTES)`` uint8, a row's first byte its length and
    the characters behind it (bytes outside 0x20 .. 0x7E as ``?``, at most 31); the last row, ``?``, is the name of a label
    outside the classes."""
    rows = np.zeros((len(class_names) + 1, _lib.DRAW_NAME_BYTES), np.uint8)
    for k, name in enumerate(list(class_names) + ['?']):
        raw = name.encode('utf-8', 'replace') if isinstance(name, str) else bytes(name)
        raw = bytes(b if 0x20 <= b <= 0x7E else ord('?') for b in raw[:_lib.DRAW_NAME_BYTES - 1])
        rows[k, 0] = len(raw)
        rows[k, 1:1 + len(raw)] = np.frombuffer(raw, np.uint8)
    return rows


def _style(num_classes, score_thr, bbox_color, text_color, thickness, font_size):
    st = DrawStyle()
    st.bbox_color[:] = color_val(bbox_color)
    st.text_color[:] = color_val(text_color)
    if int(thickness) < 1 or int(font_size) < 1:
        raise ValueError(f'thickness {thickness!r} and font_size {font_size!r} must be at least 1')
    st.thickness, st.font_size, st.num_classes, st.score_thr = int(thickness), int(font_size), num_classes, float(score_thr)
    return st


def _tables(places, counts):
    """``DrawImage`` array over images placed at ``(height, width, byte offset, pitch)`` with ``counts`` boxes each."""
    table = (DrawImage * len(places))()
    base = 0
    for t, (h, w, off, pitch), k in zip(table, places, counts):
        t.height, t.width, t.pix_off, t.pitch, t.box_base, t.nbox = int(h), int(w), int(off), int(pitch), base, int(k)
        base += int(k)
    total = C.c_int64()
    check(_lib.lib().yv4_draw_layout(table, len(table), C.byref(total)), 'yv4_draw_layout')
    return table, base


def draw_boxes_into(pixels, places, dets, labels, class_names, score_thr=0.3, bbox_color=(72, 101, 241),
                    text_color=(72, 101, 241), thickness=2, font_size=13):
    """Draws in place into the flat ``torch.uint8`` device buffer ``pixels``: image n lies at ``places[n]`` = ``(height,
    width, byte offset, row pitch)`` and takes ``dets[n]`` ((k, 5) float32 device tensor: x1, y1, x2, y2, score) with
    ``labels[n]`` ((k,) integer device tensor).  One launch for the batch; nothing is read back."""
    if not torch.cuda.is_available() or pixels.device.type != 'cuda':
        raise RuntimeError('draw_boxes runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
    if not _lib.has_draw():
        raise RuntimeError('yv4_draw_boxes is not exported by the loaded libyv4_hip.so: rebuild it')
    if pixels.dtype != torch.uint8 or not pixels.is_contiguous():
        raise ValueError('pixels must be a contiguous torch.uint8 tensor')
    dev = pixels.device
    st = _style(len(class_names), score_thr, bbox_color, text_color, thickness, font_size)
    table, total = _tables(places, [int(d.shape[0]) for d in dets])
    with torch.cuda.device(dev):
        names = name_table(class_names)
        stage = torch.empty(C.sizeof(table) + 256 + names.size, dtype=torch.uint8, pin_memory=True)
        noff = (C.sizeof(table) + 255) // 256 * 256
        C.memmove(stage.data_ptr(), table, C.sizeof(table))
        stage[noff:noff + names.size] = torch.from_numpy(names.reshape(-1))
        up = stage.to(dev, non_blocking=True)
        if total:
            d = torch.cat([x.to(dev, torch.float32).reshape(-1, 5) for x in dets]).contiguous()
            lab = torch.cat([x.to(dev).reshape(-1) for x in labels]).to(torch.int32).contiguous()
        else:
            d = lab = None
        check(_lib.lib().yv4_draw_boxes(table, up.data_ptr(), len(table), pixels.data_ptr(), pixels.numel(),
                                        d.data_ptr() if total else None, lab.data_ptr() if total else None, total,
                                        up.data_ptr() + noff, C.byref(st), stream_ptr()), 'yv4_draw_boxes')
    return pixels


def draw_boxes(imgs, dets, labels, class_names, **style):
    """``imgs``: a list of contiguous (h, w, 3) ``torch.uint8`` device tensors -> drawn COPIES, as views of one flat buffer
    (``draw_boxes_into`` on the copy)."""
    offs, end = [], 0
    for a in imgs:
        if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
            raise ValueError(f'an image to draw on is a (h, w, 3) torch.uint8 tensor, not {tuple(a.shape)} {a.dtype}')
        offs.append(end)
        end += (a.numel() + 255) // 256 * 256
    flat = torch.empty(end, dtype=torch.uint8, device=imgs[0].device)
    views = [flat[o:o + a.numel()].view(a.shape) for o, a in zip(offs, imgs)]
    for v, a in zip(views, imgs):
        v.copy_(a)
    draw_boxes_into(flat, [(a.shape[0], a.shape[1], o, 3 * a.shape[1]) for o, a in zip(offs, imgs)], dets, labels,
                    class_names, **style)
    return views


def draw_boxes_host(img, dets, labels, class_names, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241),
                    thickness=2, font_size=13):
    """The kernel's per-pixel function on the CPU (``yv4_draw_boxes_host``) over one numpy image -> the drawn copy.  For
    tests; ``draw_boxes`` never takes this path."""
    out = np.array(img, np.uint8, copy=True, order='C')
    d = np.ascontiguousarray(np.asarray(dets, np.float32).reshape(-1, 5))
    lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
    st = _style(len(class_names), score_thr, bbox_color, text_color, thickness, font_size)
    table, total = _tables([(out.shape[0], out.shape[1], 0, 3 * out.shape[1])], [d.shape[0]])
    names = name_table(class_names)
    check(_lib.lib().yv4_draw_boxes_host(table, 1, out.ctypes.data, out.size, d.ctypes.data if total else None,
                                         lab.ctypes.data if total else None, total, names.ctypes.data, C.byref(st)),
          'yv4_draw_boxes_host')
    return out
