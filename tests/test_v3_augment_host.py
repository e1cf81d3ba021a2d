"""The YOLOv3 mstrain train pipeline without a GPU (mmdet_yolov4_amd/augment_v3.py): the reference's config block is
read, unsupported options are refused, the host draws + box chain reproduce what the reference's own classes gave under
``np.random.seed`` (tests/golden/v3_augment.npz, tests/golden/make_golden_v3_augment.py), the numpy restatement
(tests/_v3_aug_ref.py) reproduces the fixture's images, and the new C-ABI symbol is declared, bound and exported.
tests/test_gpu_v3_augment.py runs the kernel."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd.augment_v3 import FusedV3TrainPipeline, build_train_pipeline

import _v3_aug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMG_NORM = dict(mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True)
V3_TRAIN_PIPELINE = [     # configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78, unchanged
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion'),
    dict(type='Expand', mean=IMG_NORM['mean'], to_rgb=IMG_NORM['to_rgb'], ratio_range=(1, 2)),
    dict(type='MinIoURandomCrop', min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9), min_crop_size=0.3),
    dict(type='Resize', img_scale=[(320, 320), (608, 608)], keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', **IMG_NORM),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
MOSAIC_PIPELINE = [       # configs/yolov4/yolov4l_coco_mosaic.py:22-69
    dict(type='MosaicPipeline',
         individual_pipeline=[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                              dict(type='Resize', img_scale=(640, 640), keep_ratio=True)], pad_val=114),
    dict(type='Albu', bbox_params=dict(type='BboxParams', format='pascal_voc', min_area=4, min_visibility=0.2,
                                       label_fields=['gt_labels']),
         transforms=[dict(type='PadIfNeeded', min_height=1920, min_width=1920, border_mode=0, value=(114, 114, 114)),
                     dict(type='RandomCrop', width=1280, height=1280), dict(type='RandomScale', scale_limit=0.5),
                     dict(type='CenterCrop', width=640, height=640), dict(type='HorizontalFlip', p=0.5)]),
    dict(type='HueSaturationValueJitter', hue_ratio=0.015, saturation_ratio=0.7, value_ratio=0.4),
    dict(type='GtBBoxesFilter', min_size=2, max_aspect_ratio=20),
    dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
    dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def _with(typ, **kw):
    p = copy.deepcopy(V3_TRAIN_PIPELINE)
    for t in p:
        if t['type'] == typ:
            t.update(kw)
    return p


def test_from_config_reads_the_reference_block():
    p = FusedV3TrainPipeline.from_config(V3_TRAIN_PIPELINE)
    assert (p.brightness_delta, p.contrast_lower, p.contrast_upper, p.hue_delta) == (32, 0.5, 1.5, 18)
    assert (p.saturation_lower, p.saturation_upper) == (0.5, 1.5)
    assert (p.expand_min, p.expand_max, p.expand_prob) == (1, 2, 0.5) and p.expand_fill.tolist() == [0, 0, 0]
    assert p.sample_mode == (1, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0) and p.min_crop_size == 0.3
    assert p.img_scale == [(320, 320), (608, 608)] and p.multiscale_mode == 'range'
    assert (p.flip_ratio, p.flip_direction) == (0.5, 'horizontal')
    assert p.mean.tolist() == [0, 0, 0] and p.std.tolist() == [255, 255, 255] and p.to_rgb and p.size_divisor == 32
    # the other accepted forms of Resize and RandomFlip
    q = FusedV3TrainPipeline.from_config(_with('Resize', img_scale=[(320, 320), (416, 416), (608, 608)],
                                               multiscale_mode='value'))
    assert q.multiscale_mode == 'value' and len(q.img_scale) == 3
    assert FusedV3TrainPipeline.from_config(_with('Resize', img_scale=(608, 608))).img_scale == [(608, 608)]
    assert FusedV3TrainPipeline.from_config(_with('RandomFlip', direction='diagonal')).flip_direction == 'diagonal'
    # Expand's fill is mean[::-1] under to_rgb
    e = FusedV3TrainPipeline.from_config(_with('Expand', mean=[1, 2, 3]))
    assert e.expand_fill.tolist() == [3, 2, 1]
    assert FusedV3TrainPipeline.from_config(_with('Expand', mean=[1, 2, 3], to_rgb=False)).expand_fill.tolist() == [1, 2, 3]


@pytest.mark.parametrize('bad, words', [
    (_with('Resize', ratio_range=(0.8, 1.2)), ('Resize', 'ratio_range')),
    (_with('Resize', keep_ratio=False), ('Resize', 'keep_ratio')),
    (_with('Resize', bbox_clip_border=False), ('Resize', 'bbox_clip_border')),
    (_with('Pad', size=(608, 608), size_divisor=None), ('Pad', 'size')),
    (_with('RandomFlip', direction=['horizontal', 'vertical']), ('RandomFlip', 'direction')),
    (_with('RandomFlip', flip_ratio=[0.3, 0.3]), ('RandomFlip', 'flip_ratio')),
    (_with('MinIoURandomCrop', bbox_clip_border=False), ('MinIoURandomCrop', 'bbox_clip_border')),
    (_with('LoadImageFromFile', to_float32=False), ('LoadImageFromFile', 'to_float32')),
    ([dict(type='LoadImageFromFile')] + V3_TRAIN_PIPELINE[1:], ('LoadImageFromFile', 'to_float32')),
    (_with('PhotoMetricDistortion', gamma=2), ('PhotoMetricDistortion', 'gamma')),
    (V3_TRAIN_PIPELINE[:-2] + [dict(type='CutOut', n_holes=3)] + V3_TRAIN_PIPELINE[-2:], ('CutOut',)),
    (V3_TRAIN_PIPELINE[:3] + V3_TRAIN_PIPELINE[4:], ('order',)),
])
def test_unsupported_options_are_refused_by_name(bad, words):
    with pytest.raises(NotImplementedError) as e:
        FusedV3TrainPipeline.from_config(bad)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_build_train_pipeline_dispatches_both_recipes():
    assert isinstance(build_train_pipeline(V3_TRAIN_PIPELINE), FusedV3TrainPipeline)
    assert isinstance(build_train_pipeline(MOSAIC_PIPELINE), pkg.FusedTrainPipeline)
    assert pkg.build_train_pipeline is build_train_pipeline and pkg.FusedV3TrainPipeline is FusedV3TrainPipeline
    with pytest.raises(NotImplementedError):
        build_train_pipeline([dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(608, 608))])


def test_fixture_covers_every_branch(golden):
    """Re-asserted from the recorded draws, so that a later seed change cannot silently drop a branch."""
    g = golden('v3_augment')
    scales = [tuple(int(v) for v in s) for s in g['cfg/img_scale']]
    hit = set()
    for case in R.fixture_cases(g):
        hit |= R.branches(case, scales)
    assert hit >= set(R.BRANCHES), sorted(set(R.BRANCHES) - hit)


def test_draws_and_box_chain_reproduce_the_reference_exactly(golden):
    """draw_params(RandomState(seed)) gives the draws observed in the reference's chain after np.random.seed(seed), and
    the host box chain gives its boxes, labels and metas -- every value exactly."""
    g = golden('v3_augment')
    pipe = FusedV3TrainPipeline(**R.fixture_kwargs(g))
    cases = R.fixture_cases(g)
    assert len(cases) >= 3
    for c in cases:
        h, w = c['src'].shape[:2]
        p = pipe.draw_params(np.random.RandomState(c['seed']), h, w, c['boxes'])
        want = c['p']
        for k in ('brightness', 'contrast', 'saturation', 'hue', 'perm', 'expand', 'crop', 'crop_mode', 'crop_redraws',
                  'scale', 'rh', 'rw', 'flip'):
            assert p[k] == want[k], (c['seed'], k, p[k], want[k])
        if want['contrast'] is not None:
            assert p['contrast_first'] == want['contrast_first']
        boxes, labels, sf = pipe.transform_boxes(p, h, w, c['boxes'], c['labels'])
        assert boxes.dtype == np.float32
        np.testing.assert_array_equal(boxes, c['out_boxes'])
        np.testing.assert_array_equal(labels, c['out_labels'])
        np.testing.assert_array_equal(sf, c['scale_factor'])
        assert sf.dtype == np.float32
        assert (h, w, 3) == c['ori_shape'] and (p['rh'], p['rw'], 3) == c['img_shape']
        assert pipe.pad_shape(p) + (3,) == c['pad_shape'] and (p['flip'] is not None) == c['flip']


def test_restatement_reproduces_the_fixture_images(golden):
    g = golden('v3_augment')
    kw = R.fixture_kwargs(g)
    pipe = FusedV3TrainPipeline(**kw)
    for c in R.fixture_cases(g):
        got = R.pipeline(c['src'], c['p'], kw['mean'], kw['std'], kw['to_rgb'], kw['size_divisor'], pipe.expand_fill)
        assert got.dtype == np.float32 and got.shape == c['img'].shape == (3,) + c['pad_shape'][:2]
        np.testing.assert_array_equal(got, c['img'])
        rh, rw = c['img_shape'][:2]
        assert not got[:, rh:].any() and not got[:, :, rw:].any()        # Pad writes zeros


def test_symbol_is_declared_bound_and_exported_within_abi_8():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    assert re.search(r'#define\s+YV4_ABI_VERSION\s+8\b', text) and pkg._lib.ABI_VERSION == 8
    assert re.search(r'\bint\s+yv4_v3_augment_u8\s*\(', text) and 'yv4_v3aug_image' in text
    for name, val in (('YV4_V3AUG_CONTRAST_NONE', 0), ('YV4_V3AUG_CONTRAST_FIRST', 1), ('YV4_V3AUG_CONTRAST_LAST', 2)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(val) + r'\b', text), name
    assert (pkg._lib.V3AUG_CONTRAST_NONE, pkg._lib.V3AUG_CONTRAST_FIRST, pkg._lib.V3AUG_CONTRAST_LAST) == (0, 1, 2)
    assert 'yv4_v3_augment_u8' in pkg._lib.SIGNATURES
    lib = pkg._lib.lib()
    assert lib.yv4_abi_version() == 8 and hasattr(lib, 'yv4_v3_augment_u8') and pkg._lib.has('v3_augment')
    # struct layout of the header: 8 + 8 * 4 + 4 * 4 + 3 * 4 + 4 * 4 + 3 * 4 + 10 * 4 bytes
    assert ctypes.sizeof(pkg._lib.V3AugImage) == 136
    assert pkg._lib.V3AugImage.perm.offset == 56 and pkg._lib.V3AugImage.fill.offset == 84
    assert pkg._lib.V3AugImage.cx.offset == 96 and pkg._lib.V3AugImage.flip.offset == 128


def test_entry_point_validates_before_touching_the_device():
    lib = pkg._lib.lib()
    mean = (ctypes.c_float * 3)(0, 0, 0)
    std = (ctypes.c_float * 3)(255, 255, 255)
    one = ctypes.c_void_p(8)                                            # never dereferenced: every call below is refused
    assert lib.yv4_v3_augment_u8(None, 1, one, 32, 32, mean, std, 1, None) == -1
    assert b'null' in lib.yv4_last_error()
    assert lib.yv4_v3_augment_u8(one, 1, None, 32, 32, mean, std, 1, None) == -1
    assert lib.yv4_v3_augment_u8(one, 1, one, 32, 32, None, std, 1, None) == -1
    assert lib.yv4_v3_augment_u8(one, 0, one, 32, 32, mean, std, 1, None) == -1
    assert lib.yv4_v3_augment_u8(one, 1, one, 0, 32, mean, std, 1, None) == -1
    assert lib.yv4_v3_augment_u8(one, 1, one, 32, -4, mean, std, 1, None) == -1
    std[1] = 0
    assert lib.yv4_v3_augment_u8(one, 1, one, 32, 32, mean, std, 1, None) == -1
    assert b'std' in lib.yv4_last_error()
