"""The training loader on the GPU: ``build_train_loader`` over ``tests/golden/coco_train_set.json`` with the fixture's
image files (``coco_train_set.npz``, written into a directory here) against the same batches composed by hand with
``imread`` and the fused pipeline; determinism, ``prefetch``, the entropy modes, ranks, EXIF orientation, refused files,
and one epoch of ``Runner`` + ``train_step`` from files."""
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd.optim import build_optimizer
from conftest import GOLDEN, arch_from, state_dict_from

pytestmark = pytest.mark.gpu

CLASSES = ('cat', 'dog')

# the mosaic recipe (configs/yolov4/yolov4l_coco_mosaic.py) scaled down: 64-pixel tiles, a 192 canvas, a 128 crop, 64 out
MOSAIC = [
    dict(type='MosaicPipeline',
         individual_pipeline=[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                              dict(type='Resize', img_scale=(64, 64), keep_ratio=True)], pad_val=114),
    dict(type='Albu', update_pad_shape=True, skip_img_without_anno=False,
         bbox_params=dict(type='BboxParams', format='pascal_voc', label_fields=['gt_labels'], min_area=4,
                          min_visibility=0.2, filter_lost_elements=True),
         transforms=[dict(type='PadIfNeeded', min_height=192, min_width=192, border_mode=0, value=[114, 114, 114],
                          always_apply=True),
                     dict(type='RandomCrop', width=128, height=128, always_apply=True),
                     dict(type='RandomScale', scale_limit=0.5, interpolation=1, always_apply=True),
                     dict(type='CenterCrop', width=64, height=64, always_apply=True),
                     dict(type='HorizontalFlip', p=0.5)]),
    dict(type='HueSaturationValueJitter', hue_ratio=0.015, saturation_ratio=0.7, value_ratio=0.4),
    dict(type='GtBBoxesFilter', min_size=2, max_aspect_ratio=20),
    dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
    dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]

# the YOLOv3 mstrain recipe (configs/yolo/yolov3_d53_mstrain-608_273e_coco.py) at 64 .. 96 pixels
V3 = [
    dict(type='LoadImageFromFile', to_float32=True), dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion'),
    dict(type='Expand', mean=[0, 0, 0], to_rgb=True, ratio_range=(1, 2)),
    dict(type='MinIoURandomCrop', min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9), min_crop_size=0.3),
    dict(type='Resize', img_scale=[(64, 64), (96, 96)], keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


@pytest.fixture(scope='module')
def files(golden):
    g = golden('coco_train_set')
    return {k[4:]: g[k].tobytes() for k in g.files if k.startswith('jpg_')}


def _write_set(root, files, replace=None):
    """The annotation file and its images under ``root``; ``replace``: {image id: key of another fixture file}."""
    os.makedirs(os.path.join(root, 'img'), exist_ok=True)
    with open(os.path.join(GOLDEN, 'coco_train_set.json')) as f:
        d = json.load(f)
    with open(os.path.join(root, 'ann.json'), 'w') as f:
        json.dump(d, f)
    for im in d['images']:
        key = (replace or {}).get(im['id'], str(im['id']))
        with open(os.path.join(root, 'img', im['file_name']), 'wb') as f:
            f.write(files[key])
    return root


@pytest.fixture(scope='module')
def data_root(tmp_path_factory, files):
    return _write_set(str(tmp_path_factory.mktemp('coco_set')), files)


def _cfg(root, pipeline):
    return dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', classes=CLASSES,
                pipeline=pipeline)


def _epoch(loader):
    """One epoch -> [(img bytes, boxes, labels, draws)]: everything a comparison needs, on the host."""
    out = []
    for data in loader:
        assert set(data) == {'img', 'img_metas', 'gt_bboxes', 'gt_labels'}
        assert data['img'].dtype == torch.float32 and data['img'].is_cuda and data['img'].shape[1] == 3
        out.append((data['img'].cpu().numpy(), [b.cpu().numpy() for b in data['gt_bboxes']],
                    [l.cpu().numpy() for l in data['gt_labels']], loader.draws, data['img_metas']))
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for (ia, ba, la, da, _), (ib, bb, lb, db, _) in zip(a, b):
        assert da['indices'] == db['indices'] and da['sources'] == db['sources']
        assert ia.shape == ib.shape and ia.tobytes() == ib.tobytes()
        for x, y in zip(ba + la, bb + lb):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.fixture(scope='module')
def mosaic_epoch(data_root, gpu_device):
    """Seed 3, batch 3, ``entropy='host'``, no prefetch: computed once, compared by several tests."""
    loader = pkg.build_train_loader(_cfg(data_root, MOSAIC), 3, seed=3, device=gpu_device)
    return loader, _epoch(loader)


def _by_hand(loader, epoch, gpu_device, mosaic):
    """Every batch of ``epoch`` again from its recorded draws: ``imread`` of the source files, the dataset's boxes, the
    fused pipeline with the recorded parameters."""
    ds = loader.dataset
    for img, boxes, labels, draws, _ in epoch:
        samples = []
        for group in draws['sources']:
            paths = [os.path.join(ds.img_prefix, ds.data_infos[j]['filename']) for j in group]
            imgs = pkg.imread(paths, device=gpu_device, orientation=True)
            anns = [ds.get_ann_info(j) for j in group]
            triples = [(im, a['bboxes'], a['labels']) for im, a in zip(imgs, anns)]
            samples.append(tuple(triples) if mosaic else triples[0])
        want = loader.pipeline(samples, params=draws['params'])
        assert img.tobytes() == want['img'].cpu().numpy().tobytes()
        for n in range(len(samples)):
            np.testing.assert_array_equal(boxes[n], want['gt_bboxes'][n].cpu().numpy())
            np.testing.assert_array_equal(labels[n], want['gt_labels'][n].cpu().numpy())
            assert labels[n].dtype == np.int64 and boxes[n].dtype == np.float32


def test_mosaic_batches_equal_the_composition_by_hand(mosaic_epoch, gpu_device):
    loader, epoch = mosaic_epoch
    assert isinstance(loader.pipeline, pkg.FusedTrainPipeline) and len(loader) == len(epoch) == 1 + 3
    assert loader.sampler.samples_per_gpu == 3 and loader.dataset is not None and hasattr(loader.sampler, 'set_epoch')
    for img, boxes, _, draws, metas in epoch:
        assert img.shape == (3, 3, 64, 64) and len(metas) == 3
        assert all(len(g) == 4 and g[0] == i for g, i in zip(draws['sources'], draws['indices']))
        flag = loader.dataset.flag
        assert all((flag[g] == flag[g[0]]).all() for g in draws['sources'])      # partners from the sample's group
    assert sum(len(b) for _, boxes, _, _, _ in epoch for b in boxes) > 0
    _by_hand(loader, epoch, gpu_device, mosaic=True)


def test_v3_batches_equal_the_composition_by_hand(data_root, gpu_device):
    loader = pkg.build_train_loader(_cfg(data_root, V3), 2, seed=1, device=gpu_device)
    assert isinstance(loader.pipeline, pkg.FusedV3TrainPipeline)
    epoch = _epoch(loader)
    assert len(epoch) == len(loader) == 2 + 5
    assert all(d['sources'] == [[i] for i in d['indices']] for _, _, _, d, _ in epoch)
    assert all('pad_shape' in m and 'filename' in m for _, _, _, _, metas in epoch for m in metas)
    _by_hand(loader, epoch, gpu_device, mosaic=False)


def test_same_seed_same_batches_and_the_epoch_changes_them(data_root, mosaic_epoch, gpu_device):
    loader, epoch = mosaic_epoch
    again = pkg.build_train_loader(_cfg(data_root, MOSAIC), 3, seed=3, device=gpu_device)
    _assert_same(epoch, _epoch(again))
    assert again.sampler.epoch == 1                                    # an iteration is an epoch
    second = _epoch(again)
    assert [d['indices'] for *_, d, _ in second] != [d['indices'] for *_, d, _ in epoch]
    again.set_epoch(0)
    _assert_same(epoch, _epoch(again))
    other = pkg.build_train_loader(_cfg(data_root, MOSAIC), 3, seed=4, device=gpu_device)
    assert [d['sources'] for *_, d, _ in _epoch(other)] != [d['sources'] for *_, d, _ in epoch]


@pytest.mark.parametrize('entropy,prefetch', [('host', 1), ('device', 0), ('device', 1), ('device_sync', 0), ('device_sync', 1)])
def test_prefetch_and_entropy_modes_give_the_same_batches(data_root, mosaic_epoch, gpu_device, entropy, prefetch):
    loader = pkg.build_train_loader(_cfg(data_root, MOSAIC), 3, seed=3, device=gpu_device, entropy=entropy,
                                    prefetch=prefetch)
    _assert_same(mosaic_epoch[1], _epoch(loader))
    loader.close()


def test_ranks_take_disjoint_slices_of_one_order(data_root, gpu_device):
    from mmdet_yolov4_amd.datasets import DistributedGroupSampler
    loaders = [pkg.build_train_loader(_cfg(data_root, V3), 2, seed=5, rank=r, world=2, device=gpu_device) for r in (0, 1)]
    assert all(isinstance(ld.sampler, DistributedGroupSampler) for ld in loaders)
    got = [[d['indices'] for *_, d, _ in _epoch(ld)] for ld in loaders]
    flat = [sum(g, []) for g in got]
    # the sampler's order over both ranks: group 0 (3 images) padded to 4, group 1 (9) to 12; rank r takes the r-th half
    both = [list(DistributedGroupSampler(loaders[0].dataset, 2, 2, r, seed=5)) for r in (0, 1)]
    assert flat == both and len(flat[0]) == len(flat[1]) == 2 + 6
    counts = Counter(flat[0] + flat[1])
    assert set(counts) == set(range(12)) and sum(counts.values()) == 16
    assert sum(c - 1 for c in counts.values()) == 4                      # disjoint but for the padding's four repeats


def test_tagged_file_arrives_rotated_unless_ignored(tmp_path, files, gpu_device):
    root = _write_set(str(tmp_path), files, replace={2: 'tagged_2'})
    path = os.path.join(root, 'img', '000002.jpg')
    rotated = pkg.imread(path, device=gpu_device, orientation=True)
    plain = pkg.imread(path, device=gpu_device)
    assert tuple(rotated.shape) == (64, 48, 3) and tuple(plain.shape) == (48, 64, 3)
    assert torch.equal(rotated, plain.flip(0).transpose(0, 1))          # orientation 6: O[y, x] = D[h-1-x, y]
    seen = {}
    for color_type in ('color', 'color_ignore_orientation'):
        pipeline = [dict(V3[0], color_type=color_type)] + V3[1:]
        loader = pkg.build_train_loader(_cfg(root, pipeline), 2, seed=2, device=gpu_device)
        assert loader.orientation == (color_type == 'color')
        for data in loader:
            for n, j in enumerate(loader.draws['indices']):
                if loader.dataset.data_infos[j]['id'] == 2:
                    seen[color_type] = data['img_metas'][n]['ori_shape']
    assert seen == {'color': (64, 48, 3), 'color_ignore_orientation': (48, 64, 3)}


def test_refused_file_raises_by_name_or_is_resampled(tmp_path, files, gpu_device, caplog):
    root = _write_set(str(tmp_path), files, replace={10: 'progressive_10'})
    loader = pkg.build_train_loader(_cfg(root, V3), 2, seed=0, device=gpu_device)
    with pytest.raises(NotImplementedError, match=r'000010\.jpg.*progressive'):
        _epoch(loader)
    for prefetch in (0, 1):
        loader = pkg.build_train_loader(_cfg(root, V3), 2, seed=0, device=gpu_device, prefetch=prefetch,
                                        on_unsupported='resample')
        bad = [i for i, d in enumerate(loader.dataset.data_infos) if d['id'] == 10][0]
        with caplog.at_level('WARNING'):
            caplog.clear()
            first, second = _epoch(loader), _epoch(loader)
        assert loader.resampled >= 2 and len(first) == len(second) == len(loader)
        assert sum('000010.jpg' in r.getMessage() for r in caplog.records) == 1      # logged once per file
        for epoch in (first, second):
            hit = [(i, g[0]) for *_, d, _ in epoch for i, g in zip(d['indices'], d['sources']) if i == bad]
            assert hit and all(o != bad and loader.dataset.flag[o] == loader.dataset.flag[bad] for _, o in hit)
        loader.close()
    # a damaged scan is a ValueError in either mode
    with open(os.path.join(root, 'img', '000013.jpg'), 'wb') as f:
        f.write(files['13'][:-40])
    loader = pkg.build_train_loader(_cfg(root, V3), 2, seed=0, device=gpu_device, on_unsupported='resample')
    with pytest.raises(ValueError, match='000013'):
        _epoch(loader)


def test_one_epoch_of_runner_and_train_step_from_files(golden, data_root, gpu_device):
    g = golden('train_v4')
    stages, reps, chans = arch_from(g)
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[stages, reps, chans], out_indices=[3, 4, 5]),
        neck=dict(type='YOLOV4Neck', in_channels=[32, 64, 64], out_channels=[32, 64, 128], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=[32, 64, 128]), train_cfg=None,
        test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=300)))
    det.load_state_dict(state_dict_from(g), strict=True)
    det.to(gpu_device)
    opt = build_optimizer(det, dict(type='SGD', lr=0.01, momentum=0.937, weight_decay=0.0005, nesterov=True,
                                    paramwise_cfg=dict(bias_decay_mult=0., norm_decay_mult=0.)))
    loader = pkg.build_train_loader(_cfg(data_root, MOSAIC), 3, seed=0, device=gpu_device, prefetch=1)
    runner = H.Runner(det, opt, max_epochs=1)
    runner.register_hook_from_cfg(dict(type='DistSamplerSeedHook'))
    runner.register_hook(H.Fp16GradAccumulateOptimizerHook(accumulation=1, grad_clip=dict(max_norm=35, norm_type=2),
                                                           loss_scale='dynamic'), 'ABOVE_NORMAL')
    losses = []

    class Rec(H.Hook):
        def after_train_iter(self, r):
            losses.append(float(r.outputs['log_vars']['loss']))
    runner.register_hook(Rec(), 'LOWEST')
    runner.run(loader)
    assert len(losses) == len(loader) == 4 and all(np.isfinite(losses))
    assert runner.epoch == 1 and loader.sampler.epoch == 1
    loader.close()
