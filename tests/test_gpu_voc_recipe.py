"""A VOC block with the wrappers of ``configs/_base_/datasets/voc0712.py`` through ``tools/train.py`` and ``tools/test.py``
as children, on the generated VOC tree of tests/golden/custom_sets: ``RepeatDataset(times=3, VOCDataset(ann_file=[2007,
2012], img_prefix=[...]))`` with the plain ``Resize -> RandomFlip -> Normalize -> Pad`` train block, validation on
``VOCDataset`` (2007: the 11-point AP) with ``evaluation=dict(interval=1, metric='mAP')``, a toy three-level YOLOv4."""
import glob
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

from mmdet_yolov4_amd.registry import Config
from _custom_sets_data import jpgs_of, write_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _run(args):
    p = subprocess.Popen([sys.executable] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    try:
        out, _ = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        p.kill()
        raise
    assert p.returncode == 0, out[-4000:]
    return out


def test_voc0712_wrappers_train_and_test_as_children(tmp_path, golden, gpu_device):
    root = write_tree(str(tmp_path / 'sets'), jpgs_of(golden('custom_sets')))
    v07, v12 = os.path.join(root, 'VOC2007/'), os.path.join(root, 'VOC2012/')
    train_pipeline = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                      dict(type='Resize', img_scale=(100, 64), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
                      dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
                      dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
    test_pipeline = [dict(type='LoadImageFromFile'),
                     dict(type='MultiScaleFlipAug', img_scale=(100, 64), flip=False,
                          transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                      dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32),
                                      dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    val = dict(type='VOCDataset', ann_file=v07 + 'ImageSets/Main/trainval.txt', img_prefix=v07, pipeline=test_pipeline)
    cfg = dict(
        model=dict(type='SingleStageDetector',
                   backbone=dict(type='DarknetCSP', scale=[['conv', 'bottleneck', 'csp', 'csp', 'csp', 'sppv4'],
                                                           [None, 1, 1, 1, 1, 1], [4, 8, 16, 32, 64, 64]],
                                 out_indices=[3, 4, 5]),
                   neck=dict(type='YOLOV4Neck', in_channels=[32, 64, 64], out_channels=[32, 64, 128], csp_repetition=1),
                   bbox_head=dict(type='YOLOCSPHead', num_classes=20, in_channels=[32, 64, 128]), train_cfg=None,
                   test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=100)),
        data=dict(samples_per_gpu=2, workers_per_gpu=2,
                  train=dict(type='RepeatDataset', times=3,
                             dataset=dict(type='VOCDataset', ann_file=[v07 + 'ImageSets/Main/trainval.txt',
                                                                       v12 + 'ImageSets/Main/trainval.txt'],
                                          img_prefix=[v07, v12], pipeline=train_pipeline)),
                  val=val, test=val),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005),
        optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
        lr_config=dict(policy='step', step=[1]), checkpoint_config=dict(interval=1),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]), evaluation=dict(interval=1, metric='mAP'),
        runner=dict(type='EpochBasedRunner', max_epochs=1), workflow=[('train', 1)], load_from=None, resume_from=None,
        log_level='INFO')
    cfg_path = str(tmp_path / 'voc_toy.py')
    Config(cfg).dump(cfg_path)
    out_dir = str(tmp_path / 'out')
    _run([os.path.join(ROOT, 'tools', 'train.py'), cfg_path, '--work-dir', out_dir, '--seed', '0', '--deterministic'])
    files = glob.glob(os.path.join(out_dir, '*.log.json'))
    assert len(files) == 1 and os.path.isfile(os.path.join(out_dir, 'epoch_1.pth'))
    with open(files[0]) as f:
        lines = [json.loads(ln) for ln in f][1:]
    train = [ln for ln in lines if ln['mode'] == 'train']
    # six images survive the filters (three a year; two landscape, four portrait or square), three passes: 12 + 6 samples in
    # batches of 2 from one group each
    assert len(train) == 6 + 3 and all(np.isfinite(ln['loss']) for ln in train)
    val_line = [ln for ln in lines if ln['mode'] == 'val']
    assert len(val_line) == 1 and {'AP50', 'mAP'} <= set(val_line[0])
    out = _run([os.path.join(ROOT, 'tools', 'test.py'), cfg_path, os.path.join(out_dir, 'epoch_1.pth'), '--eval', 'mAP'])
    printed = [ln for ln in out.splitlines() if ln.startswith('OrderedDict(')]
    assert len(printed) == 1
    got = eval(printed[0], dict(OrderedDict=OrderedDict, nan=float('nan')))
    assert {k: round(float(v), 5) for k, v in got.items()} == {k: val_line[0][k] for k in ('AP50', 'mAP')}
