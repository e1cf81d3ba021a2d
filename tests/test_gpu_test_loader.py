"""The test loader on the GPU: ``build_test_loader`` over ``tests/golden/coco_train_set.json`` with the fixture's image
files (``coco_train_set.npz``, written into a directory here) against the same batches composed by hand --
``imread(orientation=True)``, then the per-image ``FusedTestPipeline``; the entropy modes, ``prefetch``, ranks, EXIF
orientation, refused and damaged files, and the loader under ``single_gpu_test``, ``EvalHook`` and a TTA ``forward_test``."""
import json
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import dist
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd.coco_eval import flatten_results
from conftest import GOLDEN

import _eval_hook_data as DATA

pytestmark = pytest.mark.gpu

CLASSES = ('cat', 'dog', 'bird')
NORM = dict(mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True)
# the test_pipeline block of configs/yolov4/yolov4l_coco_mosaic.py at 64 pixels
TEST = [dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=(64, 64), flip=False,
             transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32),
                         dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                         dict(type='Collect', keys=['img'])])]
# the test_pipeline block of configs/yolo/yolov3_d53_mstrain-608_273e_coco.py with two scales and the flip turned on
TTA = [dict(type='LoadImageFromFile'),
       dict(type='MultiScaleFlipAug', img_scale=[(64, 64), (96, 64)], flip=True,
            transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                        dict(type='Normalize', mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True),
                        dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                        dict(type='Collect', keys=['img'])])]


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
    return _write_set(str(tmp_path_factory.mktemp('coco_test_set')), files)


def _cfg(root, pipeline=TEST, **kw):
    return dict(dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', classes=CLASSES,
                     pipeline=pipeline), **kw)


class ByHand:
    """The loader composed by hand: per batch ``imread(orientation=...)`` of the files (``stand_in``: {dataset index:
    array} in place of a file), then the per-image pipeline, nested per augmentation as the test collate does."""

    def __init__(self, dataset, indices, batch, dev, pipeline=TEST, orientation=True, stand_in=None):
        self.dataset, self.indices, self.batch, self.dev = dataset, list(indices), batch, dev
        self.pipe = pkg.FusedTestPipeline.from_config(pipeline, device=dev)
        self.orientation, self.stand_in = orientation, stand_in or {}
        assert not self.pipe.batched

    def __len__(self):
        return -(-len(self.indices) // self.batch)

    def __iter__(self):
        ds = self.dataset
        for lo in range(0, len(self.indices), self.batch):
            idx = self.indices[lo:lo + self.batch]
            paths = [os.path.join(ds.img_prefix, ds.data_infos[j]['filename']) for j in idx]
            imgs = [self.stand_in[j] if j in self.stand_in else
                    pkg.imread(p, device=self.dev, orientation=self.orientation) for j, p in zip(idx, paths)]
            batch, metas = self.pipe(imgs)
            if not isinstance(batch, list):
                batch, metas = [batch], [metas]
            for per_aug in metas:
                for m, j, p in zip(per_aug, idx, paths):
                    m['ori_filename'], m['filename'] = ds.data_infos[j]['filename'], p
            yield dict(img=batch, img_metas=metas)


def _host(loader):
    """One pass -> [([bytes of the batch per augmentation], [shape per augmentation], metas)], on the host."""
    out = []
    for data in loader:
        assert set(data) == {'img', 'img_metas'} and len(data['img']) == len(data['img_metas'])
        assert all(b.dtype == torch.float32 and b.is_cuda and b.shape[1] == 3 for b in data['img'])
        out.append(([b.cpu().numpy().tobytes() for b in data['img']], [tuple(b.shape) for b in data['img']],
                    data['img_metas']))
    return out


def _same_meta(a, b):
    assert set(a) == set(b) and {'filename', 'ori_filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor',
                                 'flip'} <= set(a)
    for k in a:
        if k == 'img_norm_cfg':
            assert all(np.array_equal(a[k][j], b[k][j]) for j in ('mean', 'std', 'to_rgb'))
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
        else:
            assert a[k] == b[k], k


def _assert_same(got, want):
    assert len(got) == len(want)
    for (gb, gs, gm), (wb, ws, wm) in zip(got, want):
        assert gs == ws and gb == wb
        assert len(gm) == len(wm)
        for ga, wa in zip(gm, wm):
            assert len(ga) == len(wa)
            for a, b in zip(ga, wa):
                _same_meta(a, b)


@pytest.fixture(scope='module')
def by_hand(data_root, gpu_device):
    """Batches of 4 over the 17 files, composed by hand once: what every form of the loader must give."""
    ds = pkg.build_test_loader(_cfg(data_root)).dataset
    return _host(ByHand(ds, range(len(ds)), 4, gpu_device))


def test_batches_equal_the_composition_by_hand(data_root, by_hand, gpu_device):
    loader = pkg.build_test_loader(_cfg(data_root), samples_per_gpu=4, device=gpu_device)
    assert len(loader) == len(by_hand) == 5 and loader.dataset.test_mode and len(loader.dataset) == 17
    got = _host(loader)
    _assert_same(got, by_hand)
    assert [s[0][0] for _, s, _ in got] == [4, 4, 4, 4, 1] and len({s[0][2:] for _, s, _ in got}) > 1      # ragged canvases
    names = [m['ori_filename'] for _, _, metas in got for m in metas[0]]
    assert names == [d['filename'] for d in loader.dataset.data_infos]
    assert got[0][2][0][0]['filename'] == os.path.join(data_root, 'img/', '000001.jpg')
    _assert_same(_host(loader), by_hand)                                  # a second pass is the same pass
    assert all(v > 0 for v in loader.times.values())
    # the block's own samples_per_gpu, and the per-image pipeline form, give the same batches
    _assert_same(_host(pkg.build_test_loader(_cfg(data_root, samples_per_gpu=4), device=gpu_device, batched=False)), by_hand)


@pytest.mark.parametrize('entropy,prefetch', [('host', 1), ('device', 0), ('device', 1), ('device_sync', 0), ('device_sync', 1)])
def test_entropy_modes_and_prefetch_give_the_same_bytes(data_root, by_hand, gpu_device, entropy, prefetch):
    loader = pkg.build_test_loader(_cfg(data_root), samples_per_gpu=4, device=gpu_device, entropy=entropy,
                                   prefetch=prefetch)
    _assert_same(_host(loader), by_hand)
    loader.close()


def test_two_ranks_cover_the_sampler_order(data_root, gpu_device):
    seen = []
    for rank in (0, 1):
        loader = pkg.build_test_loader(_cfg(data_root), samples_per_gpu=4, rank=rank, world=2, device=gpu_device)
        idx = dist.sampler_indices(17, rank, 2)
        assert loader.indices == idx and len(loader) == 3
        ds = loader.dataset
        _assert_same(_host(loader), _host(ByHand(ds, idx, 4, gpu_device)))
        seen.append(idx)
    assert len(seen[0]) == len(seen[1]) == 9 and set(seen[0] + seen[1]) == set(range(17))
    merged = [j for pair in zip(*seen) for j in pair][:17]                # what collect_results undoes
    assert merged == list(range(17))


def test_tagged_file_arrives_rotated_unless_ignored(tmp_path, files, gpu_device):
    root = _write_set(str(tmp_path), files, replace={2: 'tagged_2'})
    seen = {}
    for color_type in ('color', 'color_ignore_orientation'):
        pipeline = [dict(TEST[0], color_type=color_type)] + TEST[1:]
        loader = pkg.build_test_loader(_cfg(root, pipeline), samples_per_gpu=4, device=gpu_device)
        assert loader.orientation == (color_type == 'color')
        got = _host(loader)
        _assert_same(got, _host(ByHand(loader.dataset, range(17), 4, gpu_device, orientation=color_type == 'color')))
        assert loader.dataset.data_infos[1]['id'] == 2
        seen[color_type] = got[0][2][0][1]['ori_shape']
    assert seen == {'color': (64, 48, 3), 'color_ignore_orientation': (48, 64, 3)}


def test_refused_file_raises_by_name_or_takes_the_fallback(tmp_path, files, gpu_device):
    root = _write_set(str(tmp_path), files, replace={10: 'progressive_10'})
    for prefetch in (0, 1):
        loader = pkg.build_test_loader(_cfg(root), samples_per_gpu=4, device=gpu_device, prefetch=prefetch)
        with pytest.raises(NotImplementedError, match=r'TestLoader.*000010\.jpg.*progressive'):
            _host(loader)
        loader.close()
    known = np.random.default_rng(10).integers(0, 256, (40, 64, 3), dtype=np.uint8)
    asked = []

    def fallback(path):
        asked.append(path)
        return known
    loader = pkg.build_test_loader(_cfg(root), samples_per_gpu=4, device=gpu_device, fallback=fallback)
    got = _host(loader)
    assert asked == [os.path.join(root, 'img/', '000010.jpg')]
    _assert_same(got, _host(ByHand(loader.dataset, range(17), 4, gpu_device, stand_in={9: known})))
    assert got[2][2][0][1]['ori_shape'] == (40, 64, 3) and got[2][2][0][1]['ori_filename'] == '000010.jpg'
    want, _ = pkg.FusedTestPipeline.from_config(TEST, device=gpu_device)([known])
    slot = np.frombuffer(got[2][0][0], np.float32).reshape(got[2][1][0])[1]
    hp, wp = want.shape[2:]
    assert np.array_equal(slot[:, :hp, :wp], want[0].cpu().numpy())       # the array's own letterbox is in the batch
    with pytest.raises(ValueError, match='fallback'):
        _host(pkg.build_test_loader(_cfg(root), samples_per_gpu=4, device=gpu_device, fallback=lambda p: known[:, :, 0]))
    # a damaged scan is a ValueError naming the file
    with open(os.path.join(root, 'img', '000013.jpg'), 'wb') as f:
        f.write(files['13'][:-40])
    for entropy in ('host', 'device'):
        with pytest.raises(ValueError, match='000013'):
            _host(pkg.build_test_loader(_cfg(root), samples_per_gpu=4, device=gpu_device, fallback=fallback, entropy=entropy))


def _random_head(det, seed=3):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for conv in det.bbox_head.convs_pred:
            conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=gen))
            conv.bias.zero_()


def test_the_test_loops_and_the_eval_hook_take_the_loader(data_root, gpu_device):
    det = DATA.tiny_v4(DATA.make_test_cfg(), gpu_device)
    _random_head(det)
    loader = pkg.build_test_loader(_cfg(data_root, samples_per_gpu=4), device=gpu_device)
    hand = ByHand(loader.dataset, range(17), 4, gpu_device)
    want = pkg.single_gpu_test(det, hand)
    got = pkg.single_gpu_test(det, loader)
    assert len(got) == len(want) == 17 and sum(len(c) for r in want for c in r) > 17
    for a, b in zip(got, want):
        assert len(a) == len(b) == DATA.NUM_CLASSES and all(np.array_equal(x, y) for x, y in zip(a, b))
    flat = pkg.single_gpu_test(det, loader, flat=True)
    for t, ref in zip(flat, flatten_results(want)):
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), ref)
    scores = []
    for ld in (loader, hand):
        hook = H.EvalHook(ld, interval=1, metric='bbox')
        assert hook.use_flat()                                            # the dataset accepts the flat table
        runner = H.Runner(det, None, max_epochs=1)
        hook.before_run(runner)
        hook.after_train_epoch(runner)
        assert runner.log_buffer.ready and 'bbox_mAP' in runner.log_buffer.output
        scores.append(dict(runner.log_buffer.output))
    assert scores[0] == scores[1]
    assert scores[0] == loader.dataset.evaluate(want, metric='bbox', logger='silent')


def test_tta_block_through_forward_test(data_root, gpu_device):
    det = DATA.tiny_v3(DATA.make_test_cfg(v3=True), gpu_device)
    # batches of three: every augmentation of every image in one launch, equal to the by-hand batches
    three = pkg.build_test_loader(_cfg(data_root, TTA), samples_per_gpu=3, device=gpu_device)
    assert three.pipeline.num_augs == 4 and three.pipeline.batched
    got3 = _host(three)
    _assert_same(got3, _host(ByHand(three.dataset, range(17), 3, gpu_device, pipeline=TTA)))
    assert [m[0]['flip'] for m in got3[0][2]] == [False, True, False, True] and len(got3[0][2][3]) == 3
    assert got3[0][1][0][2:] != got3[0][1][2][2:]                         # the two scales' canvases differ
    # the test loop: forward_test -> aug_test takes one image a batch (detectors/base.py:147-150)
    loader = pkg.build_test_loader(_cfg(data_root, TTA), device=gpu_device, prefetch=1)
    assert loader.samples_per_gpu == 1 and len(loader) == 17
    hand = ByHand(loader.dataset, range(17), 1, gpu_device, pipeline=TTA)
    first = next(iter(loader))
    assert len(first['img']) == 4 and all(len(m) == 1 for m in first['img_metas'])
    with torch.no_grad():
        direct = det.forward_test(first['img'], first['img_metas'], rescale=True)
    want = pkg.single_gpu_test(det, hand)
    got = pkg.single_gpu_test(det, loader)
    assert len(got) == len(want) == 17 and sum(len(c) for r in want for c in r) > 0
    for a, b in zip(got, want):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(direct[0], want[0]))
    flat = pkg.single_gpu_test(det, loader, flat=True)
    assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(flat, flatten_results(want)))
    loader.close()
