"""Detections drawn onto images on the GPU: ``draw_boxes`` (``yv4_draw_boxes_ex``, one launch per batch, one lane per pixel).

The rule is the package's own and is stated in ``include/yv4.h`` ("drawing detections"); ``tests/_draw_ref.py`` restates
it in numpy and the kernel equals it bit for bit.  The reference renders through matplotlib with anti-aliased text in a
system font, which cannot be reproduced: parity with its pictures is not claimed.

Boxes without a score -- ``(k, 4)`` instead of ``(k, 5)``, as ground truth is drawn (``imshow_det_bboxes`` writes
``|score`` only when a box has a fifth column) -- get the class name alone and are never skipped by ``score_thr``
(``YV4_DRAW_NO_SCORE``; ``tests/_draw_gt_ref.py``).  ``imshow_gt_det_bboxes`` draws an image's ground truth and then its
detections over it.
"""
import ctypes as C
import os

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


def _box_width(dets):
    """4 or 5: the columns of every box table of a call (4: no scores, ``YV4_DRAW_NO_SCORE``)."""
    widths = {int(d.shape[-1]) if d.ndim == 2 else 5 for d in dets}
    if len(widths) > 1 or not widths <= {4, 5}:
        raise ValueError(f'the box tables of one draw call are all (k, 5) or all (k, 4), got widths {sorted(widths)}')
    return widths.pop() if widths else 5


def draw_boxes_into(pixels, places, dets, labels, class_names, score_thr=0.3, bbox_color=(72, 101, 241),
                    text_color=(72, 101, 241), thickness=2, font_size=13):
    """Draws in place into the flat ``torch.uint8`` device buffer ``pixels``: image n lies at ``places[n]`` = ``(height,
    width, byte offset, row pitch)`` and takes ``dets[n]`` ((k, 5) float32 device tensor: x1, y1, x2, y2, score -- or
    (k, 4) in every image: boxes without a score, labelled by the class name alone and never skipped) with ``labels[n]``
    ((k,) integer device tensor).  One launch for the batch; nothing is read back."""
    if not torch.cuda.is_available() or pixels.device.type != 'cuda':
        raise RuntimeError('draw_boxes runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
    width = _box_width(dets)
    _lib.require('draw_ex')
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
            d = torch.cat([x.to(dev, torch.float32).reshape(-1, width) for x in dets])
            if width == 4:                                   # the rows stay five floats wide: the fifth is not read
                d = torch.nn.functional.pad(d, (0, 1))
            d = d.contiguous()
            lab = torch.cat([x.to(dev).reshape(-1) for x in labels]).to(torch.int32).contiguous()
        else:
            d = lab = None
        check(_lib.lib().yv4_draw_boxes_ex(
            table, up.data_ptr(), len(table), pixels.data_ptr(), pixels.numel(), d.data_ptr() if total else None,
            lab.data_ptr() if total else None, total, up.data_ptr() + noff, C.byref(st),
            _lib.DRAW_NO_SCORE if width == 4 else 0, stream_ptr()), 'yv4_draw_boxes_ex')
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
    """The kernel's per-pixel function on the CPU (``yv4_draw_boxes_host_ex``) over one numpy image -> the drawn copy;
    ``dets`` (k, 5), or (k, 4) for boxes without a score.  For tests; ``draw_boxes`` never takes this path."""
    out = np.array(img, np.uint8, copy=True, order='C')
    dets = np.asarray(dets, np.float32)
    width = _box_width([dets])
    _lib.require('draw_ex')
    d = dets.reshape(-1, width)
    if width == 4:
        d = np.concatenate([d, np.zeros((d.shape[0], 1), np.float32)], 1)
    d = np.ascontiguousarray(d)
    lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
    st = _style(len(class_names), score_thr, bbox_color, text_color, thickness, font_size)
    table, total = _tables([(out.shape[0], out.shape[1], 0, 3 * out.shape[1])], [d.shape[0]])
    names = name_table(class_names)
    check(_lib.lib().yv4_draw_boxes_host_ex(
        table, 1, out.ctypes.data, out.size, d.ctypes.data if total else None, lab.ctypes.data if total else None,
        total, names.ctypes.data, C.byref(st), _lib.DRAW_NO_SCORE if width == 4 else 0), 'yv4_draw_boxes_host_ex')
    return out


def result_boxes(result, device=None):
    """One image's detections as ``(dets (k, 5) float32, labels (k,) int64)``: the per-class list of (n, 5) arrays
    (``np.vstack`` and the class of every row, as ``imshow_gt_det_bboxes`` forms them), or ``(dets, labels)`` tensors,
    which pass through.  A ``(bbox, segm)`` tuple carries masks, which are not built.  With ``device`` the pair is put
    there."""
    if isinstance(result, tuple) and len(result) == 2 and isinstance(result[0], torch.Tensor):
        d, lab = result
    elif isinstance(result, tuple):
        raise NotImplementedError('a (bbox, segm) result carries masks, which are not built')
    else:
        rows = [np.asarray(r, np.float32).reshape(-1, 5) for r in result]
        d = torch.from_numpy(np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32))
        lab = torch.from_numpy(np.concatenate([np.full(r.shape[0], k, np.int64) for k, r in enumerate(rows)])
                               if rows else np.zeros(0, np.int64))
    d, lab = d.reshape(-1, 5), lab.reshape(-1)
    return (d.to(device, torch.float32), lab.to(device)) if device is not None else (d, lab)


def gt_boxes(annotation, device=None):
    """An annotation's ground truth as ``(boxes (k, 4) float32, labels (k,) int64)`` tensors: the keys ``gt_bboxes`` /
    ``gt_labels`` of a loaded sample, as the reference reads them, or ``bboxes`` / ``labels`` of ``get_ann_info``."""
    if annotation.get('gt_masks', None) is not None:
        raise NotImplementedError('imshow_gt_det_bboxes: gt_masks are not built')
    keys = ('gt_bboxes', 'gt_labels') if 'gt_bboxes' in annotation else ('bboxes', 'labels')
    assert keys[0] in annotation and keys[1] in annotation, 'the annotation holds neither gt_bboxes / gt_labels nor bboxes / labels'
    b, lab = annotation[keys[0]], annotation[keys[1]]
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b, np.float32).reshape(-1, 4))
    lab = lab if isinstance(lab, torch.Tensor) else torch.from_numpy(np.asarray(lab, np.int64).reshape(-1))
    b, lab = b.reshape(-1, 4), lab.reshape(-1)
    return (b.to(device, torch.float32), lab.to(device)) if device is not None else (b, lab)


def draw_gt_det_into(pixels, places, annotations, results, class_names, score_thr=0, gt_bbox_color=(255, 102, 61),
                     gt_text_color=(255, 102, 61), det_bbox_color=(72, 101, 241), det_text_color=(72, 101, 241), thickness=2,
                     font_size=13):
    """The batch behind ``imshow_gt_det_bboxes``: two launches over the images lying in ``pixels`` at ``places`` (as
    ``draw_boxes_into`` takes them) -- every image's ground truth (no score), then its detections over it."""
    dev = pixels.device
    gts = [gt_boxes(a, dev) for a in annotations]
    dets = [result_boxes(r, dev) for r in results]
    draw_boxes_into(pixels, places, [g[0] for g in gts], [g[1] for g in gts], class_names, score_thr=0,
                    bbox_color=gt_bbox_color, text_color=gt_text_color, thickness=thickness, font_size=font_size)
    draw_boxes_into(pixels, places, [d[0] for d in dets], [d[1] for d in dets], class_names, score_thr=score_thr,
                    bbox_color=det_bbox_color, text_color=det_text_color, thickness=thickness, font_size=font_size)
    return pixels


def imshow_gt_det_bboxes(img, annotation, result, class_names, score_thr=0, gt_bbox_color=(255, 102, 61),
                         gt_text_color=(255, 102, 61), det_bbox_color=(72, 101, 241), det_text_color=(72, 101, 241), thickness=2,
                         font_size=13, show=False, out_file=None):
    """``mmdet.core.visualization.imshow_gt_det_bboxes`` on the GPU, by the package's own drawing rule: the ground
    truth of ``annotation`` (``gt_bboxes`` / ``gt_labels``, or ``bboxes`` / ``labels``) first, labelled by the class name
    alone, then the detections of ``result`` (the per-class list, a ``(bbox, segm)`` tuple without masks being refused)
    with a score above ``score_thr`` over it.  ``img``: a JPEG file name, a (h, w, 3) BGR uint8 array or a device
    tensor.  Returns the drawn device tensor, and with ``out_file`` also writes it as a JPEG.  There is no display:
    ``show=True`` raises, and so do masks."""
    from . import image_io
    if show:
        raise NotImplementedError('imshow_gt_det_bboxes(show=True): there is no display window; pass out_file=')
    if not isinstance(result, (tuple, list)):
        raise TypeError(f'imshow_gt_det_bboxes: the result is a per-class list or a (bbox, segm) tuple, not {type(result)}')
    if isinstance(result, tuple) and not isinstance(result[0], torch.Tensor):
        if result[1] is not None:
            raise NotImplementedError('imshow_gt_det_bboxes: a (bbox, segm) result carries masks, which are not built')
        result = result[0]
    if out_file is not None:
        image_io.check_jpeg_paths([out_file], 'imshow_gt_det_bboxes')
    if not torch.cuda.is_available():
        raise RuntimeError('imshow_gt_det_bboxes runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
    if isinstance(img, (str, os.PathLike)):
        img = image_io.imread(img)
    elif isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('imshow_gt_det_bboxes: the image is not a file name or a (h, w, 3) uint8 array or tensor')
    out = img.contiguous().clone()
    draw_gt_det_into(out.view(-1), [(out.shape[0], out.shape[1], 0, 3 * out.shape[1])], [annotation], [result],
                     list(class_names), score_thr, gt_bbox_color, gt_text_color, det_bbox_color, det_text_color, thickness,
                     font_size)
    if out_file is not None:
        image_io.imwrite(out, out_file)
    return out
