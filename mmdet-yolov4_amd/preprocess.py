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
    ``Normalize`` in the config (the YOLOv4 configs pad first, so the border carries ``(0 - mean) / std``).

    ``batched=True``: the whole call -- every augmentation of every image, the batch's zero padding included -- is ONE
    ``yv4_letterbox_u8_batch`` launch into one ``torch.empty`` allocation, of which the returned batches are views.  numpy
    inputs are packed into one pinned buffer and go up in one copy; device tensors, views with a row pitch among them
    (``decode_into(placement=...)``), are read where they lie; the slot table is staged pinned and uploaded once.  Every
    element equals the default per-image path's, bit for bit."""

    def __init__(self, img_scale=(640, 640), size_divisor=32, mean=(114, 114, 114), std=(255, 255, 255), to_rgb=True,
                 pad_val=0, pad_before_normalize=True, device=None, flip=False, flip_direction='horizontal', batched=False):
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
        self.device, self.batched = device, bool(batched)

    @classmethod
    def from_config(cls, pipeline, device=None, batched=False):
        """Build from a reference ``test_pipeline`` list (``cfg.data.test.pipeline``): ``LoadImageFromFile`` and
        ``Collect`` / ``ImageToTensor`` / ``RandomFlip`` carry no arithmetic of their own and are accepted; the geometry
        comes from ``MultiScaleFlipAug(img_scale, flip, flip_direction)`` + ``Resize(keep_ratio=True)``,
        ``Pad(size_divisor)`` and ``Normalize(mean, std, to_rgb)``, and their order decides whether the border is
        normalised.  A flip needs ``RandomFlip`` after ``Resize`` and before ``Pad`` (the v3 configs' order)."""
        kw, seen = dict(device=device, batched=batched), []

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
        if self.batched:
            out = self._run_batched(images)
            return out[0] if len(self.augs) == 1 else ([b for b, _ in out], [m for _, m in out])
        if len(self.augs) == 1:
            return self._run(images, self.augs[0][0], None, False)
        out = [self._run(images, sc, d, True) for sc, d in self.augs]
        return [b for b, _ in out], [m for _, m in out]

    def _dev(self):
        if not torch.cuda.is_available():
            raise RuntimeError('FusedTestPipeline runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
        return torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())

    @staticmethod
    def _check(img, dev):
        if isinstance(img, torch.Tensor):      # decoded on the device already (image_io.imread): no upload
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError('FusedTestPipeline takes (h, w, 3) uint8 images')
            if img.device.type != dev.type or (dev.index is not None and img.device.index != dev.index):
                raise ValueError(f'FusedTestPipeline on {dev} takes uint8 tensors of that device, not of {img.device}')
        elif img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError('FusedTestPipeline takes (h, w, 3) uint8 images')

    def _geometry(self, h, w, img_scale):
        nh, nw = rescale_size(h, w, img_scale)
        d = self.size_divisor
        return h, w, nh, nw, int(math.ceil(nh / d)) * d, int(math.ceil(nw / d)) * d

    def _meta(self, g, flip, direction, tta):
        h, w, nh, nw, hp, wp = g
        meta = dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(hp, wp, 3),
                    scale_factor=np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32), flip=bool(flip),
                    img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
        if tta:
            meta['flip_direction'] = direction
        return meta

    def _run(self, images, img_scale, direction, tta):
        dev = self._dev()
        geo = []
        for img in images:
            self._check(img, dev)
            geo.append(self._geometry(img.shape[0], img.shape[1], img_scale))
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
            metas.append(self._meta((h, w, nh, nw, hp, wp), flip, direction, tta))
        return batch, metas

    def _run_batched(self, images):
        """-> ``[(batch, img_metas) per augmentation]``: one slot per (augmentation, image), one launch."""
        _lib.require('letterbox_batch', 'FusedTestPipeline(batched=True)')
        dev = self._dev()
        images = list(images)
        if not images:
            raise ValueError('FusedTestPipeline: an empty batch')
        for img in images:
            self._check(img, dev)
        N, tta = len(images), len(self.augs) > 1
        # the host images back to back in one pinned buffer; a device image where it lies, if its rows are dense pixels
        host = [i for i, img in enumerate(images) if not isinstance(img, torch.Tensor)]
        offs = np.concatenate([[0], np.cumsum([images[i].size for i in host], dtype=np.int64)])
        src = [None] * N
        with torch.cuda.device(dev):
            keep = []
            if host:
                stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
                flat = stage.numpy()
                for k, i in enumerate(host):
                    flat[offs[k]:offs[k + 1]].reshape(images[i].shape)[...] = images[i]
                up = stage.to(dev, non_blocking=True)
                keep.append(up)
                for k, i in enumerate(host):
                    src[i] = (up.data_ptr() + int(offs[k]), 3 * images[i].shape[1])
            for i, img in enumerate(images):
                if isinstance(img, torch.Tensor):
                    if img.stride(2) != 1 or img.stride(1) != 3 or (img.shape[0] > 1 and img.stride(0) < 3 * img.shape[1]):
                        img = img.contiguous()
                        keep.append(img)
                    src[i] = (img.data_ptr(), img.stride(0) if img.shape[0] > 1 else 3 * img.shape[1])
            # the canvases of the augmentations back to back, each begun on a 16-byte boundary
            geos, bases, total = [], [], 0
            for sc, _ in self.augs:
                geo = [self._geometry(img.shape[0], img.shape[1], sc) for img in images]
                H, W = max(g[4] for g in geo), max(g[5] for g in geo)
                geos.append((geo, H, W))
                bases.append(total)
                total += (N * 3 * H * W + 3) // 4 * 4
            S = N * len(self.augs)
            tstage = torch.empty(S * C.sizeof(_lib.LetterboxSlot), dtype=torch.uint8, pin_memory=True)
            table = (_lib.LetterboxSlot * S).from_address(tstage.data_ptr())
            for a, ((sc, direction), (geo, H, W)) in enumerate(zip(self.augs, geos)):
                flip = 0 if direction is None else _lib.FLIP_CODES[direction]
                for i, (h, w, nh, nw, hp, wp) in enumerate(geo):
                    t = table[a * N + i]
                    t.src, t.src_h, t.src_w, t.src_pitch = src[i][0], h, w, src[i][1]
                    t.inv_sx, t.inv_sy = 1.0 / (nw / w), 1.0 / (nh / h)
                    t.dst_off = bases[a] + i * 3 * H * W
                    t.new_h, t.new_w, t.pad_h, t.pad_w, t.H, t.W, t.flip = nh, nw, hp, wp, H, W, flip
            table_dev = tstage.to(dev, non_blocking=True)
            out = torch.empty(total, dtype=torch.float32, device=dev)
            check(_lib.lib().yv4_letterbox_u8_batch(
                table, table_dev.data_ptr(), S, out.data_ptr(), total, self.mean.ctypes.data_as(C.c_void_p),
                self.std.ctypes.data_as(C.c_void_p), int(self.to_rgb), self.pad_val, int(self.pad_first), stream_ptr()),
                'yv4_letterbox_u8_batch')
        res = []
        for (sc, direction), (geo, H, W), base in zip(self.augs, geos, bases):
            flip = 0 if direction is None else _lib.FLIP_CODES[direction]
            res.append((out[base:base + N * 3 * H * W].view(N, 3, H, W), [self._meta(g, flip, direction, tta) for g in geo]))
        return res
