"""YOLOv3 test-time augmentation without a GPU: the pipeline's augmentation list from the reference's config block,
the C-ABI symbols and their argument validation, and a CPU restatement of the merge that reproduces the reference's
aug_test results from its per-augmentation outputs (tests/golden/v3_tta.npz, tests/golden/make_golden_v3_tta.py).
tests/test_gpu_tta.py runs the kernels."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from oracle import yolov3_oracle as V3
from oracle import yolov4_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('yv4_letterbox_u8_flip', 'yv4_topk_slots_work', 'yv4_topk_slots', 'yv4_tta_merge')
IMG_NORM = dict(mean=[0, 0, 0], std=[255.0, 255.0, 255.0], to_rgb=True)


def v3_test_pipeline(img_scale, flip, flip_direction='horizontal'):
    """test_pipeline of configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:79-93 with TTA switched on."""
    return [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=img_scale, flip=flip, flip_direction=flip_direction,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Normalize', **IMG_NORM), dict(type='Pad', size_divisor=32),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


def test_pipeline_builds_augmentations_in_reference_order():
    pipe = pkg.FusedTestPipeline.from_config(v3_test_pipeline([(608, 608), (416, 416)], True, ['horizontal', 'vertical']))
    # test_time_aug.py:95-106: per scale the unflipped image, then one per direction
    assert pipe.augs == [((608, 608), None), ((608, 608), 'horizontal'), ((608, 608), 'vertical'),
                         ((416, 416), None), ((416, 416), 'horizontal'), ((416, 416), 'vertical')]
    assert pipe.num_augs == 6 and not pipe.pad_first and pipe.to_rgb and pipe.size_divisor == 32
    pipe = pkg.FusedTestPipeline.from_config(v3_test_pipeline((320, 320), True, 'diagonal'))
    assert pipe.augs == [((320, 320), None), ((320, 320), 'diagonal')]
    pipe = pkg.FusedTestPipeline.from_config(v3_test_pipeline([(608, 608), (320, 320)], False))
    assert pipe.augs == [((608, 608), None), ((320, 320), None)]
    # one augmentation: the pipeline of before
    pipe = pkg.FusedTestPipeline.from_config(v3_test_pipeline((608, 608), False))
    assert pipe.num_augs == 1 and pipe.img_scale == (608, 608)
    with pytest.raises(ValueError):
        pkg.FusedTestPipeline.from_config(v3_test_pipeline((608, 608), True, 'sideways'))
    bad = v3_test_pipeline((608, 608), True)
    bad[1]['transforms'] = [dict(type='RandomFlip')] + [t for t in bad[1]['transforms'] if t['type'] != 'RandomFlip']
    with pytest.raises(NotImplementedError):             # a flip of the source image is not the configs' order
        pkg.FusedTestPipeline.from_config(bad)


def test_yolov3_config_with_flip_builds_detector_and_pipeline():
    cfg = pkg.Config(dict(
        model=dict(type='YOLOV3',
                   backbone=dict(type='Darknet', depth=53, out_indices=(3, 4, 5)),
                   neck=dict(type='YOLOV3Neck', num_scales=3, in_channels=[1024, 512, 256], out_channels=[512, 256, 128]),
                   bbox_head=dict(type='YOLOV3Head', num_classes=80, in_channels=[512, 256, 128],
                                  out_channels=[1024, 512, 256]),
                   test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, conf_thr=0.005,
                                 nms=dict(type='nms', iou_threshold=0.45), max_per_img=100)),
        data=dict(test=dict(pipeline=v3_test_pipeline([(608, 608), (416, 416)], True)))))
    det = pkg.build_detector(cfg.model)
    assert hasattr(det, 'compile_tta') and hasattr(det.bbox_head, 'aug_test_preds')
    pipe = pkg.FusedTestPipeline.from_config(cfg.data.test.pipeline)
    assert [d for _, d in pipe.augs] == [None, 'horizontal', None, 'horizontal']


def test_tta_symbols_declared_bound_exported():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    for name, val in (('YV4_FLIP_NONE', 0), ('YV4_FLIP_HORIZONTAL', 1), ('YV4_FLIP_VERTICAL', 2),
                      ('YV4_FLIP_DIAGONAL', 3), ('YV4_TTA_MAX_AUGS', 16)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(val) + r'\b', text), name
    lib = pkg._lib.lib()
    for name in SYMS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in pkg._lib.SIGNATURES and name in pkg._lib.FEATURES['tta'].symbols
        assert getattr(lib, name).argtypes == pkg._lib.SIGNATURES[name][1]
    assert pkg._lib.has('tta')
    assert pkg._lib.ABI_VERSION == 8 and lib.yv4_abi_version() == 8
    # yv4_tta_aug: 4 pointers, int64 total, int32 S, int32 flip
    assert ctypes.sizeof(pkg._lib.TtaAug) == 48 and pkg._lib.TtaAug.flip.offset == 44


def test_tta_argument_validation_without_gpu():
    lib = pkg._lib.lib()
    fake = ctypes.c_void_p(4096)            # never dereferenced: validation returns first
    mean = (ctypes.c_float * 3)(0, 0, 0)
    std = (ctypes.c_float * 3)(255, 255, 255)
    args = (fake, 10, 10, 30, fake, 32, 32, 32 * 32, 10, 10, mean, std, 1, 0, 0)
    assert lib.yv4_letterbox_u8_flip(*args, 4, None) == -1
    assert b'flip' in lib.yv4_last_error()
    assert lib.yv4_letterbox_u8_flip(*args, -1, None) == -1
    assert lib.yv4_letterbox_u8_flip(None, *args[1:], 1, None) == -1
    sizes = (ctypes.c_int32 * 3)(36, 144, 576)
    assert lib.yv4_topk_slots_work(3, sizes, 40) == 0                  # every cut level sorts in LDS
    big = (ctypes.c_int32 * 2)(100, 20000)
    assert lib.yv4_topk_slots_work(2, big, 10000) > 0                  # a 10 000-box top-k: the radix path's work
    assert lib.yv4_topk_slots(None, 1, 756, 3, sizes, 40, fake, None, fake, 116, None) == -1
    assert lib.yv4_topk_slots(fake, 0, 756, 3, sizes, 40, fake, None, fake, 116, None) == -1           # N
    assert lib.yv4_topk_slots(fake, 1, 700, 3, sizes, 40, fake, None, fake, 116, None) == -1           # sizes != total
    assert lib.yv4_topk_slots(fake, 1, 756, 3, sizes, 40, fake, None, fake, 117, None) == -1           # S
    assert b'S = 117' in lib.yv4_last_error()
    assert lib.yv4_topk_slots(fake, 1, 756, 3, sizes, 40, None, None, fake, 116, None) == -1           # keys needed
    assert lib.yv4_topk_slots(fake, 1, 20100, 2, big, 10000, fake, None, fake, 10100, None) == -1      # work needed
    aug = (pkg._lib.TtaAug * 2)()
    for a in aug:
        a.boxes = a.conf = a.cls = a.slots = 4096
        a.total, a.S, a.flip = 756, 116, 0
    merge = lib.yv4_tta_merge
    assert merge(aug, 0, 1, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1                   # no augmentation
    assert merge(aug, 17, 1, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1                  # > YV4_TTA_MAX_AUGS
    assert merge(aug, 2, 0, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1                   # N
    assert merge(aug, 2, 1, 0, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1                   # C
    assert merge(aug, 2, 1, 6, 0.05, None, fake, fake, 1392, fake, fake, None) == -1                   # meta
    aug[1].flip = 4
    assert merge(aug, 2, 1, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1
    assert b'flip' in lib.yv4_last_error()
    aug[1].flip, aug[1].S = 0, 757                                                                     # S > total
    assert merge(aug, 2, 1, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1
    aug[1].S, aug[1].total, aug[0].total = 1 << 30, 1 << 30, 1 << 30                                   # 32-bit index
    aug[0].S = 1 << 30
    assert merge(aug, 2, 1, 6, 0.05, fake, fake, fake, 1392, fake, fake, None) == -1
    assert b'32-bit' in lib.yv4_last_error()


# ---- the merge restated on the CPU, against the reference's own aug_test ------------------------------------------
def _case(g, name):
    return json.loads(str(g['cases']))[name]


def _map_back(bboxes, img_shape, sf, direction):
    """core/bbox/transforms.py:5-55 bbox_flip + bbox_mapping_back, fp32 torch ops in the reference's order."""
    b = bboxes.clone()
    if direction in ('horizontal', 'diagonal'):
        b[:, 0] = img_shape[1] - bboxes[:, 2]
        b[:, 2] = img_shape[1] - bboxes[:, 0]
    if direction in ('vertical', 'diagonal'):
        b[:, 1] = img_shape[0] - bboxes[:, 3]
        b[:, 3] = img_shape[0] - bboxes[:, 1]
    return b / b.new_tensor(sf)


def cpu_aug_merge(bboxes, scores, confs, img_shapes, sfs, dirs, cfg, rescale):
    """dense_test_mixins.py:38-100 after get_bboxes: map back, concatenate, multiclass_nms(score_factors=conf),
    rescale=False -> * augmentation 0's scale_factor, bbox2result."""
    mapped = [_map_back(torch.from_numpy(b), s, f, d) for b, s, f, d in zip(bboxes, img_shapes, sfs, dirs)]
    det, lab = O.multiclass_nms(torch.cat(mapped), torch.from_numpy(np.concatenate(scores)), cfg['score_thr'],
                                cfg['nms'], cfg['max_per_img'], score_factors=torch.from_numpy(np.concatenate(confs)))
    if not rescale:
        det = det.clone()
        det[:, :4] *= det.new_tensor(sfs[0])
    return pkg.bbox2result(det, lab, scores[0].shape[1] - 1)


@pytest.mark.parametrize('name', ['scales_hflip', 'vflip_dflip', 'split', 'empty'])
def test_cpu_merge_reproduces_reference_aug_test(golden, name):
    g = golden('v3_tta')
    case = _case(g, name)
    A = case['num_augs']
    per = [[g[f'{name}/{k}{a}'] for a in range(A)] for k in ('bboxes', 'scores', 'conf')]
    shapes = [tuple(int(v) for v in g[f'{name}/img_shape{a}']) for a in range(A)]
    sfs = [g[f'{name}/scale_factor{a}'] for a in range(A)]
    if name == 'split':
        assert sum(int((s[:, :-1] > case['test_cfg']['score_thr']).sum()) for s in per[1]) >= 10000
    for rescale, tag in ((True, ''), (False, '_norescale')):
        got = cpu_aug_merge(*per, shapes, sfs, case['flips'], case['test_cfg'], rescale)
        for c in range(6):
            want = g[f'{name}/result{tag}_{c}']
            assert got[c].shape == want.shape, (name, tag, c)
            np.testing.assert_array_equal(got[c], want)                  # labels (per-class lists), boxes and scores


@pytest.mark.parametrize('name', ['scales_hflip', 'vflip_dflip', 'split'])
def test_oracle_restates_get_bboxes_without_nms(golden, name):
    """yolo_head.py:208-391 with with_nms=False from the reference's pred maps: the slot order (levels concatenated,
    a cut level by descending objectness, ties to the lower index), conf and scores bit for bit."""
    g = golden('v3_tta')
    case = _case(g, name)
    nms_pre = case['test_cfg']['nms_pre']
    for a in range(case['num_augs']):
        preds = [torch.from_numpy(g[f'{name}/pred{a}_{i}']) for i in range(3)]
        bs, cs, ss = [], [], []
        for boxes, conf, cls in V3.decode_maps_v3(preds, 6):
            b, c, s = boxes[0], conf[0], cls[0]
            if 0 < nms_pre < c.shape[0]:
                sel = torch.from_numpy(np.lexsort((np.arange(c.shape[0]), -c.numpy().astype(np.float64)))[:nms_pre].copy())
                b, c, s = b[sel], c[sel], s[sel]
            bs.append(b), cs.append(c), ss.append(s)
        np.testing.assert_array_equal(torch.cat(cs).numpy(), g[f'{name}/conf{a}'])
        np.testing.assert_array_equal(torch.cat(ss).numpy(), g[f'{name}/scores{a}'][:, :-1])
        assert not g[f'{name}/scores{a}'][:, -1].any()
        np.testing.assert_allclose(torch.cat(bs).numpy(), g[f'{name}/bboxes{a}'], rtol=1e-5, atol=1e-4)
