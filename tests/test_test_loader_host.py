"""``TestLoader`` / ``build_test_loader`` without a GPU: the order (``DistributedSampler(shuffle=False)``), the batches,
what ``build_test_loader`` takes from the dataset block and what it refuses.  Nothing here decodes a file."""
import ctypes
import os

import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import datasets as D
from mmdet_yolov4_amd import dist
from conftest import GOLDEN

ANN = os.path.join(GOLDEN, 'coco_train_set.json')
NORM = dict(mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True)
# the test_pipeline block of configs/yolov4/yolov4l_coco_mosaic.py at 64 pixels
TEST = [dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=(64, 64), flip=False,
             transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32),
                         dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                         dict(type='Collect', keys=['img'])])]


def _block(**kw):
    return dict(dict(type='CocoDataset', ann_file=ANN, classes=('cat', 'dog', 'bird'), pipeline=TEST), **kw)


class _Sized:
    """As much of a dataset as the loader's order needs."""

    def __init__(self, n):
        self.data_infos = [dict(filename=f'{i}.jpg') for i in range(n)]
        self.img_prefix = ''

    def __len__(self):
        return len(self.data_infos)


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [1, 5, 16, 17])
def test_order_is_the_distributed_sampler_without_shuffle(n, world):
    from torch.utils.data import DistributedSampler
    seen = []
    for rank in range(world):
        loader = D.TestLoader(_Sized(n), None, samples_per_gpu=4, rank=rank, world=world)
        assert loader.indices == dist.sampler_indices(n, rank, world)
        if n >= world:
            assert loader.indices == list(DistributedSampler(range(n), world, rank, shuffle=False))
        assert [j for b in loader.batches for j in b] == loader.indices          # consecutive runs of the order
        assert len(loader) == len(loader.batches) == -(-len(loader.indices) // 4)
        assert all(len(b) == 4 for b in loader.batches[:-1]) and len(loader.batches[-1]) == (len(loader.indices) - 1) % 4 + 1
        seen.append(loader.indices)
        loader.close()
    assert set(sum(seen, [])) == set(range(n)) and len({len(s) for s in seen}) == 1
    if world == 1:
        assert seen[0] == list(range(n))


def test_batch_count_and_ragged_tail_of_the_fixture():
    loader = pkg.build_test_loader(_block(), samples_per_gpu=4)
    assert len(loader.dataset) == 17 and len(loader) == 5
    assert [len(b) for b in loader.batches] == [4, 4, 4, 4, 1] and loader.batches[-1] == [16]
    assert loader.dataset.accepts_flat and isinstance(loader, pkg.TestLoader)
    assert loader._path(0) == os.path.join(loader.dataset.img_prefix, '000001.jpg')


def test_samples_per_gpu_comes_from_the_block_and_stays_out_of_the_dataset():
    block = _block(samples_per_gpu=8)
    loader = pkg.build_test_loader(block)
    assert loader.samples_per_gpu == 8 and len(loader) == 3
    assert block['samples_per_gpu'] == 8 and 'test_mode' not in block               # the caller's block is not edited
    assert pkg.build_test_loader(block, samples_per_gpu=3).samples_per_gpu == 3      # the argument wins
    assert pkg.build_test_loader(_block()).samples_per_gpu == 1


def test_test_mode_is_forced():
    train = pkg.build_dataset(_block())
    assert not train.test_mode and len(train) < 17                                   # the train side filters
    for kw in (dict(), dict(test_mode=False), dict(test_mode=True)):
        ds = pkg.build_test_loader(_block(**kw)).dataset
        assert ds.test_mode and len(ds) == 17 and not hasattr(ds, 'flag')
        assert [d['id'] for d in ds.data_infos] == list(range(1, 18))


def test_train_only_transform_is_refused_by_name():
    bad = [TEST[0], dict(type='LoadAnnotations', with_bbox=True)] + TEST[1:]
    with pytest.raises(NotImplementedError, match='LoadAnnotations'):
        pkg.build_test_loader(_block(pipeline=bad))
    inner = dict(TEST[1], transforms=[dict(type='PhotoMetricDistortion')] + TEST[1]['transforms'])
    with pytest.raises(NotImplementedError, match='PhotoMetricDistortion'):
        pkg.build_test_loader(_block(pipeline=[TEST[0], inner]))
    with pytest.raises(ValueError, match='pipeline'):
        pkg.build_test_loader(dict(type='CocoDataset', ann_file=ANN, classes=('cat', 'dog', 'bird')))


def test_color_type_decides_the_orientation():
    assert pkg.build_test_loader(_block()).orientation is True
    for color_type, want in (('color', True), ('color_ignore_orientation', False)):
        pipeline = [dict(TEST[0], color_type=color_type)] + TEST[1:]
        assert pkg.build_test_loader(_block(pipeline=pipeline)).orientation is want
    with pytest.raises(NotImplementedError, match='grayscale'):
        pkg.build_test_loader(_block(pipeline=[dict(TEST[0], color_type='grayscale')] + TEST[1:]))


def test_pipeline_form_and_bad_arguments():
    loader = pkg.build_test_loader(_block())
    assert isinstance(loader.pipeline, pkg.FusedTestPipeline) and loader.pipeline.batched is D.TEST_LOADER_BATCHED
    assert loader.pipeline.img_scale == (64, 64) and loader.pipeline.size_divisor == 32 and loader.pipeline.pad_first
    assert pkg.build_test_loader(_block(), batched=False).pipeline.batched is False
    assert pkg.build_test_loader(_block(), batched=True).pipeline.batched is True
    assert pkg.FusedTestPipeline().batched is False                                  # the default pipeline is per image
    assert pkg._lib.has('letterbox_batch')
    # yv4_letterbox_slot (include/yv4.h): a pointer, two doubles, an int64, ten int32
    slot = pkg._lib.LetterboxSlot
    assert ctypes.sizeof(slot) == 72
    assert (slot.inv_sx.offset, slot.dst_off.offset, slot.src_h.offset, slot.flip.offset) == (8, 24, 32, 68)
    for kw in (dict(prefetch=2), dict(rank=2, world=2), dict(samples_per_gpu=0), dict(fallback='cv2')):
        with pytest.raises(ValueError):
            D.TestLoader(_Sized(3), None, **kw)
