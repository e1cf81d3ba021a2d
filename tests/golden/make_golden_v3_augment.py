"""Golden vectors of the YOLOv3 mstrain train pipeline (configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78), made by
running the REFERENCE's own transform classes in the build container, in the config's order, under ``np.random.seed(s)``:

  PhotoMetricDistortion -> Expand -> MinIoURandomCrop -> Resize(keep_ratio=True, two-scale range) -> RandomFlip ->
  Normalize -> Pad(size_divisor=32)

with the reference's real ``mmdet/core/evaluation/bbox_overlaps.py`` (pure numpy) behind MinIoURandomCrop.

THE ``mmcv.*`` PIXEL FUNCTIONS ARE STAND-INS: mmcv and OpenCV are absent from the build image, so ``mmcv.bgr2hsv``,
``hsv2bgr``, ``imrescale``, ``imflip``, ``imnormalize`` and ``impad_to_multiple`` are bound to the numpy float32
restatement tests/_v3_aug_ref.py.  What this fixture pins is therefore the reference's control flow, draw order, box
arithmetic, fill, channel permutation and hue wrap rules -- NOT OpenCV's bits ("parity unpinned").

The draws are OBSERVED, not recomputed: the ``random`` module object transforms.py imported is replaced by a proxy that
forwards to ``numpy.random`` and logs every call next to the stand-ins' own calls; brightness / contrast / saturation /
hue are told apart by their position relative to the colour conversions, the crop patch is the last trial's four draws,
scale and flip are read from the results dict.

Seeds are picked greedily so that the cases together hit every branch listed in BRANCHES (asserted before writing).  The
sources are small (<= 64 x 80) and the scale range is scaled down to [(32, 32), (64, 64)] to keep the file small.
Output: tests/golden/v3_augment.npz (data only).
    python tests/golden/make_golden_v3_augment.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import _v3_aug_ref as R  # noqa: E402
from oracle import build_ref  # noqa: E402

CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32,
           img_scale=[(32, 32), (64, 64)], expand_ratio_range=(1, 2), min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9),
           min_crop_size=0.3, flip_ratio=0.5)
BRANCHES = R.BRANCHES
FLIP_CODES = {None: 0, 'horizontal': 1, 'vertical': 2, 'diagonal': 3}
LOG = []


class RandomProxy:
    """Forwards to numpy.random (the global legacy RandomState) and logs (name, args, value)."""

    def __getattr__(self, name):
        fn = getattr(np.random, name)

        def call(*a, **k):
            v = fn(*a, **k)
            LOG.append((name, a, v))
            return v
        return call


def import_transforms():
    _ref_import.install_shim(build_ref.load_ext())
    sys.modules['cv2'] = types.ModuleType('cv2')                       # absent; nothing below calls it
    core = sys.modules['mmdet.core']
    core.PolygonMasks = type('PolygonMasks', (), {})
    _ref_import._pkg('mmdet.core.evaluation', os.path.join(_ref_import.REF, 'mmdet', 'core', 'evaluation'))
    importlib.import_module('mmdet.core.evaluation.bbox_overlaps')     # the reference's real file (pure numpy)
    ds = os.path.join(_ref_import.REF, 'mmdet', 'datasets')
    _ref_import._pkg('mmdet.datasets', ds)
    _ref_import._pkg('mmdet.datasets.pipelines', os.path.join(ds, 'pipelines'))
    _ref_import._mod('mmdet.datasets.builder', PIPELINES=_ref_import._Registry('pipeline'))
    _ref_import._mod('mmdet.datasets.pipelines.compose', Compose=object)
    mmcv = sys.modules['mmcv']
    mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(s, t) for s in seq)

    def logged(name, fn):
        def call(*a, **k):
            out = fn(*a, **k)
            LOG.append((name, a, out))
            return out
        return call
    for name in ('bgr2hsv', 'hsv2bgr', 'imrescale', 'imflip', 'imnormalize', 'impad_to_multiple'):
        setattr(mmcv, name, logged(name, getattr(R, name)))             # STAND-INS: tests/_v3_aug_ref.py
    T = importlib.import_module('mmdet.datasets.pipelines.transforms')
    T.random = RandomProxy()
    return T


def sources():
    rng = np.random.RandomState(7)
    out = []
    for (h, w, k) in ((60, 80, 4), (64, 48, 3), (48, 64, 0)):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[:8, :12] = rng.randint(0, 256, (8, 12, 1))                 # grey patch: d == 0, s == 0
        img[-6:, -10:] = 0                                              # black patch: v == 0, v < 0 under a negative brightness
        img[10:16, 20:30, 1] = 0                                        # magenta-ish: hue near 300
        img[20:26, 5:15, :2] //= 8                                      # red-ish: hue near 0 / 360
        img[30:36, 34:44] = rng.randint(0, 12, (6, 10, 3))              # dark, coloured: v < 0 with s != 0 under a negative brightness
        xy = rng.rand(k, 2) * [w * 0.6, h * 0.6]
        wh = rng.rand(k, 2) * [w * 0.4, h * 0.4] + 4
        boxes = np.concatenate([xy, np.minimum(xy + wh, [w, h])], 1).astype(np.float32)
        out.append((img, boxes, rng.randint(0, 80, k).astype(np.int64)))
    return out


def run(T, src, boxes, labels, seed):
    """The reference's chain on one sample -> (results, observed draws, branches hit)."""
    del LOG[:]
    np.random.seed(seed)
    chain = [T.PhotoMetricDistortion(), T.Expand(mean=CFG['mean'], to_rgb=CFG['to_rgb'], ratio_range=CFG['expand_ratio_range']),
             T.MinIoURandomCrop(min_ious=CFG['min_ious'], min_crop_size=CFG['min_crop_size']),
             T.Resize(img_scale=CFG['img_scale'], keep_ratio=True), T.RandomFlip(flip_ratio=CFG['flip_ratio']),
             T.Normalize(mean=CFG['mean'], std=CFG['std'], to_rgb=CFG['to_rgb']), T.Pad(size_divisor=CFG['size_divisor'])]
    res = dict(img=src.astype(np.float32), gt_bboxes=boxes.copy(), gt_labels=labels.copy(), img_fields=['img'],
               bbox_fields=['gt_bboxes'], ori_shape=src.shape, img_shape=src.shape)
    marks = {}
    for t in chain:
        marks[type(t).__name__] = len(LOG)
        res = t(res)
        if type(t).__name__ == 'Expand':
            canvas = res['img'].shape[:2]
    names = [type(t).__name__ for t in chain]

    def section(name):
        i = names.index(name)
        return LOG[marks[name]:marks[names[i + 1]] if i + 1 < len(names) else len(LOG)]
    # ---- PhotoMetricDistortion: position relative to the two colour conversions tells the uniforms apart
    d = dict(brightness=None, contrast=None, contrast_first=False, saturation=None, hue=None, perm=None)
    stage = 0
    for name, a, v in section('PhotoMetricDistortion'):
        if name == 'bgr2hsv':
            stage, hsv0 = 1, v.copy()
        elif name == 'hsv2bgr':
            stage = 2
        elif name == 'permutation':
            d['perm'] = tuple(int(c) for c in v)
        elif name == 'uniform':
            if stage == 0 and a[0] < 0:
                d['brightness'] = v
            elif stage == 0:
                d['contrast'], d['contrast_first'] = v, True
            elif stage == 1 and a[0] < 0:
                d['hue'] = v
            elif stage == 1:
                d['saturation'] = v
            else:
                d['contrast'] = v
    # ---- Expand: uniform(0, 1), then ratio, left, top
    ex = [v for name, a, v in section('Expand') if name == 'uniform']
    d['expand'] = None if len(ex) == 1 else (int(canvas[0]), int(canvas[1]), int(ex[2]), int(ex[3]))
    assert len(ex) in (1, 4)
    # ---- MinIoURandomCrop: one `choice` per mode draw; an accepted patch is the last trial's four uniforms
    cr = section('MinIoURandomCrop')
    modes = [float(v) for name, a, v in cr if name == 'choice']
    d['crop_redraws'], d['crop_mode'] = len(modes) - 1, modes[-1]
    if modes[-1] == 1:
        d['crop'] = None
    else:
        new_w, new_h, left, top = [v for name, a, v in cr if name == 'uniform'][-4:]
        d['crop'] = (int(left), int(top), int(left + new_w), int(top + new_h))
    d['scale'] = tuple(int(s) for s in res['scale'])
    d['rh'], d['rw'] = (int(s) for s in res['img_shape'][:2])
    d['flip'] = res['flip_direction']
    # ---- branches
    h0 = hsv0[..., 0]
    hit = {('brightness_on' if d['brightness'] is not None else 'brightness_off'),
           ('contrast_off' if d['contrast'] is None else 'contrast_first' if d['contrast_first'] else 'contrast_last'),
           ('saturation_on' if d['saturation'] is not None else 'saturation_off'),
           ('hue_on' if d['hue'] is not None else 'hue_off'), ('perm_on' if d['perm'] is not None else 'perm_off'),
           ('expand_on' if d['expand'] is not None else 'expand_off'),
           ('crop_mode1' if d['crop'] is None else 'crop_taken'), ('flip_on' if d['flip'] is not None else 'flip_off')}
    if d['hue'] is not None:
        hh = h0 + np.float32(d['hue'])
        hit |= {'wrap_hi'} if (hh > 360).any() else set()
        hit |= {'wrap_lo'} if (hh < 0).any() else set()
    hit |= {'s_zero'} if (hsv0[..., 1] == 0).any() else set()
    hit |= {'v_nonpos'} if (hsv0[..., 2] < 0).any() else set()
    hit |= {'crop_drops_boxes'} if d['crop'] is not None and len(res['gt_bboxes']) < len(boxes) else set()
    hit |= {'crop_exhausted'} if d['crop_redraws'] > 0 else set()
    hit |= {'no_gt'} if len(boxes) == 0 else set()
    lo, hi = min(min(s) for s in CFG['img_scale']), max(max(s) for s in CFG['img_scale'])
    hit |= {'scale_lo'} if lo in d['scale'] else set()
    hit |= {'scale_hi'} if hi in d['scale'] else set()
    return res, d, hit


def pack_draws(d):
    nan = float('nan')
    f = np.array([nan if d[k] is None else d[k] for k in ('brightness', 'contrast', 'saturation', 'hue')] + [d['crop_mode']],
                 dtype=np.float64)
    i = np.array([int(d['contrast_first'])] + list(d['perm'] or (-1, -1, -1)) + list(d['expand'] or (-1, -1, -1, -1)) +
                 list(d['crop'] or (-1, -1, -1, -1)) + [d['crop_redraws'], d['scale'][0], d['scale'][1], d['rh'], d['rw'],
                                                      FLIP_CODES[d['flip']]], dtype=np.int64)
    return f, i


def main():
    if not _ref_import.available():
        print('reference not present: nothing to do')
        return
    T = import_transforms()
    srcs = sources()
    cands = {}
    for si, (img, boxes, labels) in enumerate(srcs):
        for seed in range(400):
            cands[(si, seed)] = run(T, img, boxes, labels, seed)[2]
    need, chosen = set(BRANCHES), []
    while need:                                                         # greedy cover, ties to the lower (source, seed)
        best = max(sorted(cands), key=lambda k: len(cands[k] & need))
        assert cands[best] & need, f'no candidate hits {sorted(need)}'
        chosen.append(best)
        need -= cands[best]
    for si in range(len(srcs)):                                         # every source at least once
        if not any(c[0] == si for c in chosen):
            chosen.append((si, 0))
    data = {'cfg/mean': np.array(CFG['mean'], np.float64), 'cfg/std': np.array(CFG['std'], np.float64),
            'cfg/to_rgb': np.array(CFG['to_rgb']), 'cfg/size_divisor': np.array(CFG['size_divisor']),
            'cfg/img_scale': np.array(CFG['img_scale'], np.int64),
            'cfg/expand_ratio_range': np.array(CFG['expand_ratio_range'], np.int64),
            'cfg/min_ious': np.array(CFG['min_ious'], np.float64), 'cfg/min_crop_size': np.array(CFG['min_crop_size']),
            'cfg/flip_ratio': np.array(CFG['flip_ratio']), 'num_cases': np.array(len(chosen)),
            'num_sources': np.array(len(srcs))}
    for si, (img, boxes, labels) in enumerate(srcs):
        data[f'src{si}/img'], data[f'src{si}/boxes'], data[f'src{si}/labels'] = img, boxes, labels
    covered = set()
    for ci, (si, seed) in enumerate(chosen):
        res, d, hit = run(T, *srcs[si], seed)
        covered |= hit
        f, i = pack_draws(d)
        data[f'case{ci}/source'], data[f'case{ci}/seed'] = np.array(si), np.array(seed)
        data[f'case{ci}/draws_f'], data[f'case{ci}/draws_i'] = f, i
        data[f'case{ci}/img'] = np.ascontiguousarray(res['img'].transpose(2, 0, 1))
        data[f'case{ci}/boxes'], data[f'case{ci}/labels'] = res['gt_bboxes'], res['gt_labels']
        data[f'case{ci}/ori_shape'] = np.array(res['ori_shape'], np.int64)
        data[f'case{ci}/img_shape'] = np.array(res['img_shape'], np.int64)
        data[f'case{ci}/pad_shape'] = np.array(res['pad_shape'], np.int64)
        data[f'case{ci}/scale_factor'] = res['scale_factor']
        data[f'case{ci}/flip'] = np.array(bool(res['flip']))
        assert res['img'].dtype == np.float32 and res['gt_bboxes'].dtype == np.float32
        print(f'case{ci}: source {si} seed {seed} -> img {res["img"].shape} boxes {len(res["gt_bboxes"])} {sorted(hit)}')
    assert covered >= set(BRANCHES), sorted(set(BRANCHES) - covered)
    out = os.path.join(HERE, 'v3_augment.npz')
    np.savez_compressed(out, **data)
    print('wrote v3_augment.npz', os.path.getsize(out) // 1024, 'KB,', len(chosen), 'cases')


if __name__ == '__main__':
    main()
