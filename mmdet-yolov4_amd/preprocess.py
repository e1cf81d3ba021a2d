"""Test-time input pipeline on the GPU: ``Resize(keep_ratio=True) -> Pad(size_divisor) -> Normalize ->
ImageToTensor -> collate`` for a list of 8-bit HWC images, one ``yv4_letterbox_u8`` launch per image, straight
into the NCHW fp32 batch ``SingleStageDetector.simple_test`` takes, plus the ``img_metas`` the reference's pipeline
would have produced (``ori_shape``, ``img_shape``, ``pad_shape``, ``scale_factor``, ``flip``).

Test-time augmentation (``MultiScaleFlipAug(img_scale=[...], flip=True, flip_direction=...)``,
``mmdet/datasets/pipelines/test_time_aug.py:95-106``): one batch per augmentation, in the reference's order -- per
scale the unflipped image, then one per flip direction -- the flip applied to the resized image by
``yv4_letterbox_u8_flip`` (``RandomFlip`` between ``Resize`` and ``Normalize`` / ``Pad``).

Mirrors the ``test_pipeline`` block of ``configs/yolov4/yolov4l_coco_mosaic.py:70-84`` (transform classes of
``mmdet/datasets/pipelines/transforms.py`` and the batch padding of mmcv's ``collate``).  **Parity unpinned**: the
arithmetic of those transforms is mmcv's and OpenCV's, third party and absent from the build image; the kernel is
tested bit for bit against ``oracle/preprocess_oracle.py``, a restatement of their published algorithms.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import stream_ptr


def rescale_size(h, w, scale):
    """mmcv ``rescale_size`` with a (long, short) tuple: the largest factor keeping both edges inside."""
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(h * float(factor) + 0.5), int(w * float(factor) + 0.5)


class FusedTestPipeline:
    """``FusedTestPipeline(img_scale=(640, 640), size_divisor=32, mean=..., std=..., to_rgb=True)(images)`` ->
    ``(batch (N, 3, H, W) fp32 on the GPU, img_metas)``.  ``images``: (h, w, 3) uint8 numpy arrays, which are uploaded,
    or ``torch.uint8`` tensors already on the pipeline's device (``image_io.imread``), which are not; mixed freely.
    ``pad_before_normalize``: the order of ``Pad`` and
    ``Normalize`` in the config (the YOLOv4 configs pad first, so the border carries ``(0 - mean) / std``)."""

    def __init__(self, img_scale=(640, 640), size_divisor=32, mean=(114, 114, 114), std=(255, 255, 255), to_rgb=True,
                 pad_val=0, pad_before_normalize=True, device=None, flip=False, flip_direction='horizontal'):
        """``img_scale``: one (long, short) tuple or a list of them; ``flip`` / ``flip_direction`` as
        ``MultiScaleFlipAug``.  More than one augmentation makes ``__call__`` return one batch per augmentation."""
        scales = [tuple(x) for x in img_scale] if isinstance(img_scale, list) else [tuple(img_scale)]
        dirs = flip_direction if isinstance(flip_direction, list) else [flip_direction]
        for d in dirs:
            if d not in _lib.FLIP_CODES:
                raise ValueError(f'flip_direction {d!r} is not one of {sorted(_lib.FLIP_CODES)}')
        # MultiScaleFlipAug order (test_time_aug.py:95-106)
        self.augs = [(sc, None) for sc in scales] if not flip else [(sc, d) for sc in scales for d in [None] + dirs]
        self.img_scale, self.size_divisor = scales[0], int(size_divisor)
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        self.to_rgb, self.pad_val, self.pad_first = bool(to_rgb), int(pad_val), bool(pad_before_normalize)
        self.device = device

    @classmethod
    def from_config(cls, pipeline, device=None):
        """Build from a reference ``test_pipeline`` list (``cfg.data.test.pipeline``): ``LoadImageFromFile`` and
        ``Collect`` / ``ImageToTensor`` / ``RandomFlip`` carry no arithmetic of their own and are accepted; the geometry
        comes from ``MultiScaleFlipAug(img_scale, flip, flip_direction)`` + ``Resize(keep_ratio=True)``,
        ``Pad(size_divisor)`` and ``Normalize(mean, std, to_rgb)``, and their order decides whether the border is
        normalised.  A flip needs ``RandomFlip`` after ``Resize`` and before ``Pad`` (the v3 configs' order)."""
        kw, seen = dict(device=device), []

        def walk(items):
            for t in items:
                typ = t['type']
                if typ == 'MultiScaleFlipAug':
                    if t.get('img_scale') is None:
                        raise NotImplementedError('MultiScaleFlipAug(scale_factor=...) is not built')
                    scale = t['img_scale']
                    kw['img_scale'] = [tuple(x) for x in scale] if isinstance(scale, list) else tuple(scale)
                    if t.get('flip', False):
                        kw['flip'] = True
                        kw['flip_direction'] = t.get('flip_direction', 'horizontal')
                    walk(t['transforms'])
                elif typ == 'Resize':
                    if not t.get('keep_ratio', False):
                        raise NotImplementedError('Resize(keep_ratio=False) is not built')
                    if 'img_scale' in t and t['img_scale'] is not None:
                        kw['img_scale'] = tuple(t['img_scale'])
                    seen.append(typ)
                elif typ == 'Pad':
                    if t.get('size', None) is not None:
                        raise NotImplementedError('Pad(size=...) is not built')
                    kw['size_divisor'] = t['size_divisor']
                    kw['pad_val'] = t.get('pad_val', 0)
                    seen.append(typ)
                elif typ == 'Normalize':
                    kw.update(mean=t['mean'], std=t['std'], to_rgb=t.get('to_rgb', True))
                    seen.append(typ)
                elif typ == 'RandomFlip':
                    seen.append(typ)
                elif typ in ('LoadImageFromFile', 'ImageToTensor', 'Collect', 'DefaultFormatBundle'):
                    continue
                else:
                    raise NotImplementedError(f'test pipeline transform {typ!r} is not built')
        walk(pipeline)
        if kw.get('flip') and 'RandomFlip' not in seen:
            # the reference only warns and then labels unflipped images as flipped (test_time_aug.py:78-81)
            raise NotImplementedError('MultiScaleFlipAug(flip=True) without a RandomFlip transform is not built')
        if 'Resize' not in seen or 'Normalize' not in seen or 'img_scale' not in kw:
            raise ValueError('the test pipeline needs MultiScaleFlipAug / Resize and Normalize')
        if 'Pad' not in seen:
            kw['size_divisor'] = 1
        else:
            kw['pad_before_normalize'] = seen.index('Pad') < seen.index('Normalize')
        if kw.get('flip'):
            if seen.index('RandomFlip') < seen.index('Resize') or ('Pad' in seen and seen.index('RandomFlip') > seen.index('Pad')):
                raise NotImplementedError('RandomFlip is built between Resize and Pad only')
        return cls(**kw)

    @property
    def num_augs(self):
        return len(self.augs)

    def __call__(self, images):
        """-> ``(batch, img_metas)``; with more than one augmentation ``([batch per augmentation],
        [img_metas per augmentation])`` in MultiScaleFlipAug order, each meta with ``flip`` and ``flip_direction``."""
        if len(self.augs) == 1:
            return self._run(images, self.augs[0][0], None, False)
        out = [self._run(images, sc, d, True) for sc, d in self.augs]
        return [b for b, _ in out], [m for _, m in out]

    def _run(self, images, img_scale, direction, tta):
        if not torch.cuda.is_available():
            raise RuntimeError('FusedTestPipeline runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
        dev = torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        geo = []
        for img in images:
            if isinstance(img, torch.Tensor):      # decoded on the device already (image_io.imread): no upload
                if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                    raise ValueError('FusedTestPipeline takes (h, w, 3) uint8 images')
                if img.device.type != dev.type or (dev.index is not None and img.device.index != dev.index):
                    raise ValueError(f'FusedTestPipeline on {dev} takes uint8 tensors of that device, not of {img.device}')
            elif img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError('FusedTestPipeline takes (h, w, 3) uint8 images')
            h, w = img.shape[:2]
            nh, nw = rescale_size(h, w, img_scale)
            d = self.size_divisor
            geo.append((h, w, nh, nw, int(math.ceil(nh / d)) * d, int(math.ceil(nw / d)) * d))
        H = max(g[4] for g in geo)
        W = max(g[5] for g in geo)
        # collate pads every image of the batch to the largest padded shape with zeros (after Normalize)
        batch = torch.zeros((len(images), 3, H, W), dtype=torch.float32, device=dev)
        metas = []
        L = _lib.lib()
        mean_p = self.mean.ctypes.data_as(C.c_void_p)
        std_p = self.std.ctypes.data_as(C.c_void_p)
        keep = []
        flip = 0 if direction is None else _lib.FLIP_CODES[direction]

        def letterbox(src, h, w, dst, hp, wp, plane, nh, nw):
            args = (src.data_ptr(), h, w, 3 * w, dst.data_ptr(), hp, wp, plane, nh, nw, mean_p, std_p, int(self.to_rgb),
                    self.pad_val, int(self.pad_first))
            if flip:
                check(L.yv4_letterbox_u8_flip(*args, flip, stream_ptr()), 'yv4_letterbox_u8_flip')
            else:
                check(L.yv4_letterbox_u8(*args, stream_ptr()), 'yv4_letterbox_u8')
        for i, (img, (h, w, nh, nw, hp, wp)) in enumerate(zip(images, geo)):
            if isinstance(img, torch.Tensor):
                src = img.contiguous()
            else:
                src = torch.from_numpy(np.ascontiguousarray(img)).to(dev, non_blocking=True)
            keep.append(src)
            slot = batch[i]
            if (hp, wp) == (H, W):
                letterbox(src, h, w, slot, hp, wp, H * W, nh, nw)
            else:       # a smaller image of a ragged batch: produce it densely, then place it in its zero-padded slot
                tmp = torch.empty((3, hp, wp), dtype=torch.float32, device=dev)
                letterbox(src, h, w, tmp, hp, wp, hp * wp, nh, nw)
                slot[:, :hp, :wp] = tmp
            meta = dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(hp, wp, 3),
                        scale_factor=np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32), flip=bool(flip),
                        img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
            if tta:
                meta['flip_direction'] = direction
            metas.append(meta)
        return batch, metas
