"""The train-side input pipeline of the YOLOv3 mstrain recipe as one launch per batch (``csrc/augment_v3.hip``).

``FusedV3TrainPipeline.from_config(cfg.data.train.pipeline)`` reads the reference's ``train_pipeline`` block
(configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78): ``PhotoMetricDistortion -> Expand -> MinIoURandomCrop ->
Resize(img_scale=[(320, 320), (608, 608)], keep_ratio=True) -> RandomFlip -> Normalize -> Pad(size_divisor=32)``; loading
and format transforms carry no arithmetic and are accepted.  Calling it with decoded 8-bit BGR images that already live
on the device (plus their host-side boxes and labels) returns what the reference's collate hands the detector: ``img``
(N, 3, Hmax, Wmax) fp32 -- every image at its own drawn scale, zero-padded to the batch maximum -- ``gt_bboxes`` /
``gt_labels`` lists of device tensors and ``img_metas``.

What stays on the host: the random draws, made from a ``numpy.random.RandomState`` in the reference's order with the
reference's calls, so that ``RandomState(s)`` gives the parameters the reference's chain gives after ``np.random.seed(s)``
(MinIoURandomCrop's acceptance loop included: its draws depend on the boxes), and the box chain, in numpy float32 as the
reference computes it -- a few dozen boxes per image.  One descriptor table, one launch and one upload of the
concatenated boxes and labels per batch.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import FLIP_CODES, FLIP_NONE, V3AugImage, check
from .augment import FusedTrainPipeline, rescale_size
from .ops import stream_ptr

_NOOPS = ('LoadAnnotations', 'DefaultFormatBundle', 'Collect')
_ORDER = ('PhotoMetricDistortion', 'Expand', 'MinIoURandomCrop', 'Resize', 'RandomFlip', 'Normalize', 'Pad')


def _only(t, allowed):
    """Refuse every option of transform dict ``t`` this pipeline does not know."""
    for k in t:
        if k != 'type' and k not in allowed:
            raise NotImplementedError(f"{t['type']}: option {k!r} is not built")


def _patch_iou(patch, boxes):
    """IoU of one integer patch with (k, 4) float32 boxes in float32: intersection / max(area_p + area_b - intersection,
    1e-6), the arithmetic of the reference's numpy ``bbox_overlaps`` (core/evaluation/bbox_overlaps.py) for one row."""
    p = patch.astype(np.float32)
    area_p = (p[2] - p[0]) * (p[3] - p[1])
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    iw = np.maximum(np.minimum(p[2], boxes[:, 2]) - np.maximum(p[0], boxes[:, 0]), np.float32(0))
    ih = np.maximum(np.minimum(p[3], boxes[:, 3]) - np.maximum(p[1], boxes[:, 1]), np.float32(0))
    inter = iw * ih
    return inter / np.maximum(area_p + area_b - inter, np.float32(1e-6))


def _centres_in(boxes, patch):
    c = (boxes[:, :2] + boxes[:, 2:]) / 2
    return (c[:, 0] > patch[0]) & (c[:, 1] > patch[1]) & (c[:, 0] < patch[2]) & (c[:, 1] < patch[3])


def draw_resize_scale(rng, img_scale, multiscale_mode):
    """``Resize._random_scale`` without ``ratio_range`` (transforms.py:101-203): one scale as it is, ``'range'`` through
    ``random_sample`` (long edge, then short edge), ``'value'`` through ``random_select``.  ``img_scale``: a list of
    (long, short) tuples.  Shared with ``augment_plain.PlainTrainPipeline``."""
    if len(img_scale) == 1:
        scale = img_scale[0]
    elif multiscale_mode == 'range':
        longs, shorts = [max(s) for s in img_scale], [min(s) for s in img_scale]
        long_edge = rng.randint(min(longs), max(longs) + 1)
        short_edge = rng.randint(min(shorts), max(shorts) + 1)
        scale = (long_edge, short_edge)
    else:
        scale = img_scale[rng.randint(len(img_scale))]
    return scale


def draw_flip(rng, flip_ratio, flip_direction):
    """``RandomFlip.__call__``'s draw for one direction (transforms.py:430-452): the direction, or ``None``."""
    single = flip_ratio / 1
    cur = rng.choice([flip_direction, None], p=[single, 1 - flip_ratio])
    return None if cur is None else str(cur)


def resize_flip_boxes(boxes, h, w, rh, rw, flip):
    """``Resize._resize_bboxes`` (transforms.py:236-244: scale by the float32 ``scale_factor``, clip to the resized image)
    and ``RandomFlip.bbox_flip`` (:384-416) for float32 (k, 4) boxes of an (h, w) image resized to (rh, rw) -> (boxes, scale_factor)."""
    scale_factor = np.array([rw / w, rh / h, rw / w, rh / h], dtype=np.float32)
    boxes = boxes * scale_factor
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, rw)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, rh)
    if flip is not None:
        f = boxes.copy()
        if flip in ('horizontal', 'diagonal'):
            f[:, 0], f[:, 2] = rw - boxes[:, 2], rw - boxes[:, 0]
        if flip in ('vertical', 'diagonal'):
            f[:, 1], f[:, 3] = rh - boxes[:, 3], rh - boxes[:, 1]
        boxes = f
    return boxes, scale_factor


def upload_boxes(boxes, labels, dev):
    """The boxes and labels of a whole batch in one upload -- (T, 4) float32 followed by (T,) int64 -- split per image
    again: ``(gt_bboxes, gt_labels)``, lists of device tensors."""
    counts = [len(b) for b in boxes]
    T = sum(counts)
    blob = np.concatenate(boxes, 0).tobytes() + np.concatenate(labels, 0).tobytes()
    if T:
        d_blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
        d_boxes, d_labels = d_blob[:16 * T].view(torch.float32).view(T, 4), d_blob[16 * T:].view(torch.int64)
    else:
        d_boxes = torch.empty((0, 4), dtype=torch.float32, device=dev)
        d_labels = torch.empty((0,), dtype=torch.int64, device=dev)
    return list(torch.split(d_boxes, counts)), list(torch.split(d_labels, counts))


def parse_geometry_transform(t, kw):
    """The options of one ``Resize`` / ``RandomFlip`` / ``Normalize`` / ``Pad`` block into the keyword dict ``kw``, every
    option outside the built set refused by name; ``False`` for any other transform.  Shared with
    ``augment_plain.PlainTrainPipeline``."""
    typ = t['type']
    if typ == 'Resize':
        _only(t, ('img_scale', 'multiscale_mode', 'ratio_range', 'keep_ratio', 'bbox_clip_border', 'backend',
                  'override'))
        if t.get('ratio_range') is not None:
            raise NotImplementedError('Resize: ratio_range is not built')
        if not t.get('keep_ratio', True):
            raise NotImplementedError('Resize: keep_ratio=False is not built')
        if not t.get('bbox_clip_border', True):
            raise NotImplementedError('Resize: bbox_clip_border=False is not built')
        if t.get('backend', 'cv2') != 'cv2' or t.get('override', False):
            raise NotImplementedError('Resize: backend / override are not built')
        if t.get('img_scale') is None:
            raise NotImplementedError('Resize: img_scale=None is not built')
        kw.update(img_scale=t['img_scale'], multiscale_mode=t.get('multiscale_mode', 'range'))
    elif typ == 'RandomFlip':
        _only(t, ('flip_ratio', 'direction'))
        if isinstance(t.get('direction', 'horizontal'), (list, tuple)):
            raise NotImplementedError('RandomFlip: direction lists are not built')
        if not isinstance(t.get('flip_ratio'), float):
            raise NotImplementedError('RandomFlip: flip_ratio must be one float')
        kw.update(flip_ratio=t['flip_ratio'], flip_direction=t.get('direction', 'horizontal'))
    elif typ == 'Normalize':
        _only(t, ('mean', 'std', 'to_rgb'))
        kw.update(mean=t['mean'], std=t['std'], to_rgb=t.get('to_rgb', True))
    elif typ == 'Pad':
        _only(t, ('size', 'size_divisor', 'pad_val'))
        if t.get('size') is not None:
            raise NotImplementedError('Pad: size= is not built (size_divisor only)')
        if t.get('size_divisor') is None or t.get('pad_val', 0) != 0:
            raise NotImplementedError('Pad: size_divisor with pad_val=0 is the only form built')
        kw['size_divisor'] = t['size_divisor']
    else:
        return False
    return True


class FusedV3TrainPipeline:

    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18,
                 expand_mean=(0, 0, 0), expand_to_rgb=True, expand_ratio_range=(1, 4), expand_prob=0.5,
                 min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3, img_scale=((320, 320), (608, 608)),
                 multiscale_mode='range', flip_ratio=0.5, flip_direction='horizontal', mean=(0, 0, 0),
                 std=(255, 255, 255), to_rgb=True, size_divisor=32, device=None):
        self.brightness_delta = brightness_delta
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range
        self.hue_delta = hue_delta
        expand_mean = list(expand_mean)
        self.expand_fill = np.asarray(expand_mean[::-1] if expand_to_rgb else expand_mean, dtype=np.float32)
        self.expand_min, self.expand_max = expand_ratio_range
        self.expand_prob = expand_prob
        self.min_ious = tuple(min_ious)
        self.sample_mode = (1, *self.min_ious, 0)
        self.min_crop_size = min_crop_size
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
                if not t.get('to_float32', False):
                    raise NotImplementedError('LoadImageFromFile: to_float32=True is required (PhotoMetricDistortion '
                                              'asserts a float32 image)')
                continue
            if typ in _NOOPS:
                if typ == 'LoadAnnotations' and (t.get('with_mask') or t.get('with_seg')):
                    raise NotImplementedError('LoadAnnotations: with_mask / with_seg are not built')
                continue
            seen.append(typ)
            if typ == 'PhotoMetricDistortion':
                _only(t, ('brightness_delta', 'contrast_range', 'saturation_range', 'hue_delta'))
                kw.update({k: t[k] for k in t if k != 'type'})
            elif typ == 'Expand':
                _only(t, ('mean', 'to_rgb', 'ratio_range', 'prob', 'seg_ignore_label'))
                if t.get('seg_ignore_label') is not None:
                    raise NotImplementedError('Expand: seg_ignore_label is not built')
                kw.update(expand_mean=t.get('mean', (0, 0, 0)), expand_to_rgb=t.get('to_rgb', True),
                          expand_ratio_range=t.get('ratio_range', (1, 4)), expand_prob=t.get('prob', 0.5))
            elif typ == 'MinIoURandomCrop':
                _only(t, ('min_ious', 'min_crop_size', 'bbox_clip_border'))
                if not t.get('bbox_clip_border', True):
                    raise NotImplementedError('MinIoURandomCrop: bbox_clip_border=False is not built')
                kw.update(min_ious=t.get('min_ious', (0.1, 0.3, 0.5, 0.7, 0.9)), min_crop_size=t.get('min_crop_size', 0.3))
            elif parse_geometry_transform(t, kw):
                pass
            else:
                raise NotImplementedError(f'train pipeline transform {typ!r} is not built')
        if tuple(seen) != _ORDER:
            raise NotImplementedError(f'train pipeline order {seen} is not built: the kernel fuses exactly {list(_ORDER)}')
        kw.update(over)
        return cls(**kw)

    # ---- random draws (host) -----------------------------------------------------------------------------------------
    def draw_params(self, rng, h, w, boxes):
        """One sample's parameters from ``rng`` (a ``numpy.random.RandomState``), consumed in the reference's order with
        its calls: PhotoMetricDistortion (transforms.py:950-991), Expand (:1047-1067), MinIoURandomCrop (:1157-1229),
        Resize.random_sample / random_select (:101-143), RandomFlip (:430-450).  ``boxes``: this image's (k, 4) boxes --
        the crop's acceptance loop depends on them (after Expand's shift)."""
        boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        p = dict(brightness=None, contrast=None, contrast_first=False, saturation=None, hue=None, perm=None,
                 expand=None, crop=None, flip=None)
        if rng.randint(2):
            p['brightness'] = rng.uniform(-self.brightness_delta, self.brightness_delta)
        mode = rng.randint(2)
        p['contrast_first'] = bool(mode == 1)
        if mode == 1 and rng.randint(2):
            p['contrast'] = rng.uniform(self.contrast_lower, self.contrast_upper)
        if rng.randint(2):
            p['saturation'] = rng.uniform(self.saturation_lower, self.saturation_upper)
        if rng.randint(2):
            p['hue'] = rng.uniform(-self.hue_delta, self.hue_delta)
        if mode == 0 and rng.randint(2):
            p['contrast'] = rng.uniform(self.contrast_lower, self.contrast_upper)
        if rng.randint(2):
            p['perm'] = tuple(int(c) for c in rng.permutation(3))
        # Expand
        H, W = h, w
        if not rng.uniform(0, 1) > self.expand_prob:
            ratio = rng.uniform(self.expand_min, self.expand_max)
            H, W = int(h * ratio), int(w * ratio)
            left = int(rng.uniform(0, w * ratio - w))
            top = int(rng.uniform(0, h * ratio - h))
            p['expand'] = (H, W, left, top)
            boxes = boxes + np.tile((left, top), 2).astype(np.float32)
        # MinIoURandomCrop
        p['crop_redraws'] = -1
        while p['crop'] is None:
            p['crop_redraws'] += 1
            mode = rng.choice(self.sample_mode)
            p['crop_mode'] = float(mode)
            if mode == 1:
                break
            for _ in range(50):
                new_w = rng.uniform(self.min_crop_size * W, W)
                new_h = rng.uniform(self.min_crop_size * H, H)
                if new_h / new_w < 0.5 or new_h / new_w > 2:
                    continue
                left = rng.uniform(W - new_w)              # one argument: low = W - new_w, high = 1.0 (as the reference)
                top = rng.uniform(H - new_h)
                patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)))
                if patch[2] == patch[0] or patch[3] == patch[1]:
                    continue
                if len(boxes):
                    if _patch_iou(patch, boxes).min() < mode:
                        continue
                    if not _centres_in(boxes, patch).any():
                        continue
                p['crop'] = tuple(int(v) for v in patch)
                break
        ch, cw = H, W
        if p['crop'] is not None:
            x1, y1, x2, y2 = p['crop']
            ch, cw = min(y2, H) - y1, min(x2, W) - x1
        # Resize
        scale = draw_resize_scale(rng, self.img_scale, self.multiscale_mode)
        p['scale'] = (int(scale[0]), int(scale[1]))
        p['rh'], p['rw'] = rescale_size(ch, cw, scale)
        # RandomFlip
        p['flip'] = draw_flip(rng, self.flip_ratio, self.flip_direction)
        return p

    # ---- boxes (host, numpy float32 as the reference) ---------------------------------------------------------------
    def geometry(self, p, h, w):
        """(canvas h, w, left, top), (crop x1, y1, w, h) of parameters ``p`` for an (h, w) source."""
        H, W, left, top = p['expand'] if p['expand'] is not None else (h, w, 0, 0)
        if p['crop'] is not None:
            x1, y1, x2, y2 = p['crop']
            crop = (x1, y1, min(x2, W) - x1, min(y2, H) - y1)
        else:
            crop = (0, 0, W, H)
        return (H, W, left, top), crop

    def transform_boxes(self, p, h, w, boxes, labels):
        """The reference's box chain for parameters ``p``: Expand's shift, MinIoURandomCrop's centre-in-patch mask + clip
        + shift, Resize's scale + clip, the flip.  -> (boxes float32 (k', 4), labels, scale_factor float32 (4,))."""
        boxes = np.array(boxes, dtype=np.float32).reshape(-1, 4)
        labels = np.asarray(labels).reshape(-1)
        (H, W, left, top), (cx, cy, cw, ch) = self.geometry(p, h, w)
        if p['expand'] is not None:
            boxes = boxes + np.tile((left, top), 2).astype(np.float32)
        if p['crop'] is not None and len(boxes):
            patch = np.array(p['crop'])
            mask = _centres_in(boxes, patch)
            boxes, labels = boxes[mask], labels[mask]
            pf = patch.astype(np.float32)
            boxes[:, 2:] = np.minimum(boxes[:, 2:], pf[2:])
            boxes[:, :2] = np.maximum(boxes[:, :2], pf[:2])
            boxes -= np.tile(pf[:2], 2)
        boxes, scale_factor = resize_flip_boxes(boxes, ch, cw, p['rh'], p['rw'], p['flip'])
        return boxes, labels, scale_factor

    def pad_shape(self, p):
        d = self.size_divisor
        return -(-p['rh'] // d) * d, -(-p['rw'] // d) * d

    def describe(self, img, p):
        """One output image's descriptor -> filled ``V3AugImage``.  ``img``: uint8 (h, w, 3) device tensor (BGR)."""
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise TypeError('source images must be uint8 (h, w, 3) tensors on the GPU')
        if not img.is_cuda:
            raise TypeError('source images must be uint8 (h, w, 3) tensors on the GPU (there is no CPU fallback)')
        if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * img.shape[1]:
            raise ValueError('source images must be dense along w and c')
        h, w = int(img.shape[0]), int(img.shape[1])
        (H, W, left, top), (cx, cy, cw, ch) = self.geometry(p, h, w)
        if not (0 <= left and left + w <= W and 0 <= top and top + h <= H and 0 <= cx and 0 <= cy and cw > 0 and ch > 0
                and cx + cw <= W and cy + ch <= H and p['rh'] > 0 and p['rw'] > 0):
            raise ValueError(f'parameters do not fit an ({h}, {w}) source: expand {p["expand"]}, crop {p["crop"]}')
        g = V3AugImage()
        g.src, g.sh, g.sw, g.pitch = img.data_ptr(), h, w, int(img.stride(0))
        if p['brightness'] is not None:
            g.bright_on, g.bright_delta = 1, p['brightness']
        if p['contrast'] is not None:
            g.contrast_mode = _lib.V3AUG_CONTRAST_FIRST if p['contrast_first'] else _lib.V3AUG_CONTRAST_LAST
            g.contrast_alpha = p['contrast']
        if p['saturation'] is not None:
            g.sat_on, g.sat_alpha = 1, p['saturation']
        if p['hue'] is not None:
            g.hue_on, g.hue_delta = 1, p['hue']
        if p['perm'] is not None:
            if sorted(p['perm']) != [0, 1, 2]:
                raise ValueError(f'not a channel permutation: {p["perm"]}')
            g.perm_on = 1
            g.perm[0], g.perm[1], g.perm[2] = (int(c) for c in p['perm'])
        g.eh, g.ew, g.etop, g.eleft = H, W, top, left
        g.fill[0], g.fill[1], g.fill[2] = (float(v) for v in self.expand_fill)
        g.cx, g.cy, g.cw, g.ch = cx, cy, cw, ch
        g.rh, g.rw = p['rh'], p['rw']
        g.ph, g.pw = self.pad_shape(p)
        g.flip = FLIP_NONE if p['flip'] is None else FLIP_CODES[p['flip']]
        return g

    # ---- device ------------------------------------------------------------------------------------------------------
    def __call__(self, samples, rng=None, params=None):
        """``samples``: list of (image uint8 (h, w, 3) cuda tensor, boxes float32 (k, 4) numpy array in that image's pixel
        coordinates, labels int (k,)).  ``params``: list of parameter dicts (default: drawn from ``rng``, a
        ``numpy.random.RandomState``).  -> dict(img, gt_bboxes, gt_labels, img_metas, params)."""
        N = len(samples)
        if N == 0:
            raise ValueError('empty batch')
        hb = []
        for s in samples:
            b = np.asarray(s[1].cpu() if isinstance(s[1], torch.Tensor) else s[1], dtype=np.float32)
            l = np.asarray(s[2].cpu() if isinstance(s[2], torch.Tensor) else s[2])
            if b.size == 0:
                b = b.reshape(0, 4)
            if b.ndim != 2 or b.shape[1] != 4 or l.size != b.shape[0]:
                raise ValueError(f'boxes must be (k, 4) with k labels, got {b.shape} and {l.shape}')
            if not isinstance(s[0], torch.Tensor) or s[0].dim() != 3:
                raise TypeError('source images must be uint8 (h, w, 3) tensors on the GPU')
            hb.append((b, l.reshape(-1)))
        if params is None:
            rng = rng if rng is not None else np.random.RandomState()
            params = [self.draw_params(rng, int(s[0].shape[0]), int(s[0].shape[1]), b) for s, (b, _) in zip(samples, hb)]
        if len(params) != N:
            raise ValueError('one parameter dict per sample')
        table = (V3AugImage * N)()
        boxes, labels, metas = [], [], []
        for n, (s, (b, l), p) in enumerate(zip(samples, hb, params)):
            table[n] = self.describe(s[0], p)
            if s[0].device != samples[0][0].device:
                raise ValueError('all source images must live on one device')
            h, w = int(s[0].shape[0]), int(s[0].shape[1])
            ob, ol, sf = self.transform_boxes(p, h, w, b, l)
            boxes.append(ob)
            labels.append(ol.astype(np.int64))
            metas.append(dict(ori_shape=(h, w, 3), img_shape=(p['rh'], p['rw'], 3), pad_shape=self.pad_shape(p) + (3,),
                              scale_factor=sf, flip=p['flip'] is not None, flip_direction=p['flip'],
                              img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)))
        dev = samples[0][0].device
        Hmax, Wmax = max(m['pad_shape'][0] for m in metas), max(m['pad_shape'][1] for m in metas)
        d_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        img = torch.empty((N, 3, Hmax, Wmax), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(_lib.lib().yv4_v3_augment_u8(d_table.data_ptr(), N, img.data_ptr(), Hmax, Wmax,
                                               self.mean.ctypes.data_as(C.c_void_p), self.std.ctypes.data_as(C.c_void_p),
                                               int(self.to_rgb), stream_ptr()), 'yv4_v3_augment_u8')
        gt_bboxes, gt_labels = upload_boxes(boxes, labels, dev)
        return dict(img=img, gt_bboxes=gt_bboxes, gt_labels=gt_labels, img_metas=metas, params=params)


def build_train_pipeline(pipeline, **kw):
    """The fused train pipeline of a reference ``train_pipeline`` block: ``FusedTrainPipeline`` for the mosaic recipes,
    ``FusedV3TrainPipeline`` for the YOLOv3 mstrain recipe, ``PlainTrainPipeline`` for the plain ``Resize -> RandomFlip ->
    Normalize -> Pad`` block of the dataset base configs."""
    types = [t['type'] for t in pipeline]
    if 'MosaicPipeline' in types:
        return FusedTrainPipeline.from_config(pipeline, **kw)
    if 'PhotoMetricDistortion' in types:
        return FusedV3TrainPipeline.from_config(pipeline, **kw)
    if 'Resize' in types:
        from .augment_plain import PlainTrainPipeline
        return PlainTrainPipeline.from_config(pipeline, **kw)
    raise NotImplementedError(f'no fused train pipeline for {types}: neither MosaicPipeline nor PhotoMetricDistortion nor '
                              'a plain Resize block')
