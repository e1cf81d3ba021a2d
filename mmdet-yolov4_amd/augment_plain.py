"""The plain train pipeline of the reference's dataset base configs (``configs/_base_/datasets/voc0712.py``,
``coco_detection.py``) as one launch per batch: ``LoadImageFromFile -> LoadAnnotations -> Resize(img_scale,
keep_ratio=True[, multiscale_mode]) -> RandomFlip -> Normalize -> Pad(size_divisor) -> DefaultFormatBundle -> Collect``.

Pixels: the existing ``yv4_letterbox_u8_batch`` (csrc/preprocess.hip), one slot per output image with its drawn scale
and flip code; the launch writes the collate's zero padding to the batch maximum too.  The image is 8-bit here
(``LoadImageFromFile`` without ``to_float32``), so the resize is OpenCV's 8-bit fixed-point bilinear, which is what the
kernel restates.  Draws: from a ``RandomState`` in the reference's order -- ``Resize``'s scale, then ``RandomFlip``'s
choice -- with ``augment_v3``'s calls.  Boxes: on the host in float32, as ``Resize._resize_bboxes`` and
``RandomFlip.bbox_flip`` compute them.  The output is the dict ``FusedV3TrainPipeline`` returns.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import FLIP_CODES, FLIP_NONE, check
from .augment import rescale_size
from .augment_v3 import (_NOOPS, draw_flip, draw_resize_scale, parse_geometry_transform, resize_flip_boxes,
                         upload_boxes)
from .ops import stream_ptr

_ORDER = ('Resize', 'RandomFlip', 'Normalize', 'Pad')


class PlainTrainPipeline:

    def __init__(self, img_scale=(1333, 800), multiscale_mode='range', flip_ratio=0.5, flip_direction='horizontal',
                 mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, size_divisor=32, device=None):
        self.img_scale = [tuple(s) for s in (img_scale if isinstance(img_scale, list) or
                                             isinstance(img_scale[0], (tuple, list)) else [img_scale])]
        if multiscale_mode not in ('range', 'value'):
            raise NotImplementedError(f'Resize: multiscale_mode={multiscale_mode!r} is not built')
        if multiscale_mode == 'range' and len(self.img_scale) not in (1, 2):
            raise ValueError("Resize: multiscale_mode='range' takes two scales")
        self.multiscale_mode = multiscale_mode
        if not isinstance(flip_ratio, float) or not 0 <= flip_ratio <= 1:
            raise NotImplementedError('RandomFlip: flip_ratio must be one float in [0, 1]')
        if flip_direction not in FLIP_CODES:
            raise NotImplementedError(f'RandomFlip: direction={flip_direction!r} is not built')
        self.flip_ratio, self.flip_direction = flip_ratio, flip_direction
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        self.to_rgb = bool(to_rgb)
        self.size_divisor = int(size_divisor)
        self.device = device

    @classmethod
    def from_config(cls, pipeline, device=None, **over):
        kw = dict(device=device)
        seen = []
        for t in pipeline:
            typ = t['type']
            if typ == 'LoadImageFromFile':
                if t.get('to_float32', False):
                    raise NotImplementedError('LoadImageFromFile: to_float32=True is not built for the plain pipeline '
                                              '(its Resize is the 8-bit one)')
                continue
            if typ in _NOOPS:
                if typ == 'LoadAnnotations' and (t.get('with_mask') or t.get('with_seg')):
                    raise NotImplementedError('LoadAnnotations: with_mask / with_seg are not built')
                continue
            if not parse_geometry_transform(t, kw):
                raise NotImplementedError(f'train pipeline transform {typ!r} is not built')
            seen.append(typ)
        if tuple(seen) != _ORDER:
            raise NotImplementedError(f'train pipeline order {seen} is not built: the plain pipeline is exactly '
                                      f'{list(_ORDER)}')
        kw.update(over)
        return cls(**kw)

    # ---- random draws (host) -----------------------------------------------------------------------------------------
    def draw_params(self, rng, h, w):
        """One sample's parameters from ``rng`` in the reference's order: ``Resize._random_scale``
        (transforms.py:101-203), then ``RandomFlip`` (:430-452)."""
        scale = draw_resize_scale(rng, self.img_scale, self.multiscale_mode)
        p = dict(scale=(int(scale[0]), int(scale[1])))
        p['rh'], p['rw'] = rescale_size(h, w, scale)
        p['flip'] = draw_flip(rng, self.flip_ratio, self.flip_direction)
        return p

    def pad_shape(self, p):
        d = self.size_divisor
        return -(-p['rh'] // d) * d, -(-p['rw'] // d) * d

    def transform_boxes(self, p, h, w, boxes, labels):
        """-> (boxes float32 (k, 4), labels, scale_factor float32 (4,))."""
        boxes = np.array(boxes, dtype=np.float32).reshape(-1, 4)
        boxes, scale_factor = resize_flip_boxes(boxes, h, w, p['rh'], p['rw'], p['flip'])
        return boxes, np.asarray(labels).reshape(-1), scale_factor

    # ---- device ------------------------------------------------------------------------------------------------------
    def __call__(self, samples, rng=None, params=None):
        """``samples``: list of (image uint8 (h, w, 3) cuda tensor -- a view with a row pitch is read where it lies --,
        boxes float32 (k, 4), labels int (k,)).  ``params``: list of parameter dicts (default: drawn from ``rng``, a
        ``numpy.random.RandomState``).  -> dict(img, gt_bboxes, gt_labels, img_metas, params)."""
        N = len(samples)
        if N == 0:
            raise ValueError('empty batch')
        _lib.require('letterbox_batch', 'PlainTrainPipeline')
        for s in samples:
            img = s[0]
            if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 \
                    or not img.is_cuda:
                raise TypeError('source images must be uint8 (h, w, 3) tensors on the GPU (there is no CPU fallback)')
            if img.device != samples[0][0].device:
                raise ValueError('all source images must live on one device')
            if img.stride(2) != 1 or img.stride(1) != 3 or (img.shape[0] > 1 and img.stride(0) < 3 * img.shape[1]):
                raise ValueError('source images must be dense along w and c')
        if params is None:
            rng = rng if rng is not None else np.random.RandomState()
            params = [self.draw_params(rng, int(s[0].shape[0]), int(s[0].shape[1])) for s in samples]
        if len(params) != N:
            raise ValueError('one parameter dict per sample')
        boxes, labels, metas = [], [], []
        for s, p in zip(samples, params):
            h, w = int(s[0].shape[0]), int(s[0].shape[1])
            b = np.asarray(s[1].cpu() if isinstance(s[1], torch.Tensor) else s[1], dtype=np.float32)
            l = np.asarray(s[2].cpu() if isinstance(s[2], torch.Tensor) else s[2]).reshape(-1)
            if b.size == 0:
                b = b.reshape(0, 4)
            if b.ndim != 2 or b.shape[1] != 4 or l.size != b.shape[0]:
                raise ValueError(f'boxes must be (k, 4) with k labels, got {b.shape} and {l.shape}')
            ob, ol, sf = self.transform_boxes(p, h, w, b, l)
            boxes.append(ob)
            labels.append(ol.astype(np.int64))
            metas.append(dict(ori_shape=(h, w, 3), img_shape=(p['rh'], p['rw'], 3), pad_shape=self.pad_shape(p) + (3,),
                              scale_factor=sf, flip=p['flip'] is not None, flip_direction=p['flip'],
                              img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)))
        dev = samples[0][0].device
        Hmax, Wmax = max(m['pad_shape'][0] for m in metas), max(m['pad_shape'][1] for m in metas)
        total = N * 3 * Hmax * Wmax
        with torch.cuda.device(dev):
            tstage = torch.empty(N * C.sizeof(_lib.LetterboxSlot), dtype=torch.uint8, pin_memory=True)
            table = (_lib.LetterboxSlot * N).from_address(tstage.data_ptr())
            for n, (s, p, m) in enumerate(zip(samples, params, metas)):
                img, t = s[0], table[n]
                h, w = int(img.shape[0]), int(img.shape[1])
                t.src, t.src_h, t.src_w = img.data_ptr(), h, w
                t.src_pitch = int(img.stride(0)) if h > 1 else 3 * w
                t.inv_sx, t.inv_sy = 1.0 / (p['rw'] / w), 1.0 / (p['rh'] / h)
                t.dst_off = n * 3 * Hmax * Wmax
                t.new_h, t.new_w, t.pad_h, t.pad_w = p['rh'], p['rw'], m['pad_shape'][0], m['pad_shape'][1]
                t.H, t.W = Hmax, Wmax
                t.flip = FLIP_NONE if p['flip'] is None else FLIP_CODES[p['flip']]
            table_dev = tstage.to(dev, non_blocking=True)
            img = torch.empty((N, 3, Hmax, Wmax), dtype=torch.float32, device=dev)
            # Pad follows Normalize here: the border is 0.0, as the collate's padding is
            check(_lib.lib().yv4_letterbox_u8_batch(
                table, table_dev.data_ptr(), N, img.data_ptr(), total, self.mean.ctypes.data_as(C.c_void_p),
                self.std.ctypes.data_as(C.c_void_p), int(self.to_rgb), 0, 0, stream_ptr()), 'yv4_letterbox_u8_batch')
        gt_bboxes, gt_labels = upload_boxes(boxes, labels, dev)
        return dict(img=img, gt_bboxes=gt_bboxes, gt_labels=gt_labels, img_metas=metas, params=params)
