"""The training dataset and samplers without a GPU, against what the reference's own ``CocoDataset``, ``GroupSampler`` and
``DistributedGroupSampler`` return for ``tests/golden/coco_train_set.json`` (``coco_train_set.npz``,
make_golden_coco_train.py): the tables exactly, the random partner draws draw for draw, the sampler orders exactly."""
import json
import os

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import datasets as D
from conftest import GOLDEN

ANN = os.path.join(GOLDEN, 'coco_train_set.json')


@pytest.fixture(scope='module')
def ref(golden):
    g = golden('coco_train_set')
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def ds():
    return pkg.CocoDataset(ANN, pipeline=[], classes=('cat', 'dog'))


def test_fixture_file_holds_the_cases(ref):
    with open(ANN) as f:
        d = json.load(f)
    by_img = {}
    for a in d['annotations']:
        by_img.setdefault(a['image_id'], []).append(a)
    sizes = {im['id']: (im['width'], im['height']) for im in d['images']}
    assert any(w > h for w, h in sizes.values()) and any(w < h for w, h in sizes.values()) and any(w == h for w, h in sizes.values())
    assert any(min(s) < 32 for s in sizes.values()) and any(i not in by_img for i in sizes)
    assert any(all(a['iscrowd'] for a in v) for v in by_img.values())
    assert any(all(a['category_id'] == 3 for a in v) for v in by_img.values())
    anns = d['annotations']
    assert any(a['bbox'][2] < 1 for a in anns) and any(a['area'] == 0 for a in anns) and any(a.get('ignore') for a in anns)
    assert any(a['bbox'][0] >= sizes[a['image_id']][0] for a in anns)                                          # wholly outside
    assert any(0 <= a['bbox'][0] < sizes[a['image_id']][0] < a['bbox'][0] + a['bbox'][2] for a in anns)      # partly
    where = [k for k, a in enumerate(anns) if a['image_id'] == 1]
    assert len(where) >= 2 and where[1] - where[0] > 1                                                          # not adjacent
    assert set(np.unique(ref['flag'])) == {0, 1}


def test_tables_equal_the_reference(ds, ref):
    assert ds.valid_inds == ref['valid_inds'].tolist()
    assert ds.img_ids == ref['img_ids'].tolist() and len(ds) == len(ref['img_ids'])
    assert ds.flag.dtype == ref['flag'].dtype and ds.flag.tolist() == ref['flag'].tolist()
    assert [d['filename'] for d in ds.data_infos] == [f'{i:06d}.jpg' for i in ds.img_ids]
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        for key, name in (('bboxes', 'bboxes'), ('labels', 'labels'), ('bboxes_ignore', 'ignore')):
            want = ref[f'{name}_{i}']
            assert ann[key].dtype == want.dtype and ann[key].shape == want.shape, (i, key)
            np.testing.assert_array_equal(ann[key], want, err_msg=f'{key} of {i}')
    assert ds.get_ann_info(3)['bboxes'].shape == (0, 4) and ds.get_ann_info(3)['labels'].shape == (0,)      # crowd only
    assert ds.get_ann_info(0)['bboxes'].shape == (3, 4)                  # image 1: its three records, in file order


def test_unfiltered_and_test_mode(ref):
    everything = pkg.CocoDataset(ANN, classes=('cat', 'dog'), filter_empty_gt=False)
    assert everything.img_ids == ref['unfiltered_img_ids'].tolist()
    t = pkg.CocoDataset(ANN, classes=('cat', 'dog'), test_mode=True)
    assert len(t) == 17 and not hasattr(t, 'flag')
    assert pkg.DATASETS.build(dict(type='CocoDataset', ann_file='coco_train_set.json', data_root=GOLDEN,
                                   classes=('cat', 'dog'), img_prefix='img/')).img_prefix == os.path.join(GOLDEN, 'img/')


def test_duplicate_annotation_ids_are_refused():
    with open(ANN) as f:
        d = json.load(f)
    d['annotations'][3]['id'] = d['annotations'][0]['id']
    with pytest.raises(AssertionError, match='not unique'):
        pkg.CocoDataset(d, classes=('cat', 'dog'))


def _draws(ds, ref, prefix):
    for seed in (0, 1, 2):
        rng = np.random.RandomState(seed)
        got = np.stack([ds.batch_rand_others(i, 3, rng) for i in range(len(ds))])
        np.testing.assert_array_equal(got, ref[f'{prefix}others_{seed}'], err_msg=f'{prefix}others_{seed}')
        rng = np.random.RandomState(seed)
        got = np.array([ds._rand_another(i, rng) for i in range(len(ds))])
        np.testing.assert_array_equal(got, ref[f'{prefix}another_{seed}'], err_msg=f'{prefix}another_{seed}')
        np.random.seed(seed)                                  # the module-level generator is the default
        got = np.stack([ds.batch_rand_others(i, 3) for i in range(len(ds))])
        np.testing.assert_array_equal(got, ref[f'{prefix}others_{seed}'])


def test_batch_rand_others_draw_for_draw(ds, ref):
    _draws(ds, ref, '')
    others = ref['others_0']
    assert all(i not in others[i] and len(set(others[i])) == 3 for i in np.where(ref['flag'] == 1)[0])      # no replacement
    assert all((ref['flag'][others[i]] == ref['flag'][i]).all() for i in range(len(ds)))


def test_groups_smaller_than_the_batch(ref):
    bird = pkg.CocoDataset(ANN, classes=('bird',))
    assert bird.img_ids == ref['bird_img_ids'].tolist() and bird.flag.tolist() == ref['bird_flag'].tolist()
    assert sorted(np.bincount(bird.flag)) == [2, 3]                       # pools of 1 and 2: drawn with replacement
    _draws(bird, ref, 'bird_')
    with open(ANN) as f:
        d = json.load(f)
    d['images'] = [im for im in d['images'] if im['id'] in (13, 7)]
    d['annotations'] = [a for a in d['annotations'] if a['image_id'] in (13, 7)]
    solo = pkg.CocoDataset(d, classes=('bird',))
    assert solo.img_ids == ref['solo_img_ids'].tolist() and solo.flag.tolist() == ref['solo_flag'].tolist() == [0, 1]
    _draws(solo, ref, 'solo_')
    assert solo.batch_rand_others(1, 3).tolist() == [1, 1, 1]              # an empty pool: [idx] * batch


def test_group_sampler_orders(ds, ref):
    for seed in (3, 4):
        for spg in (2, 3):
            s = D.GroupSampler(ds, spg, rng=np.random.RandomState(seed))
            got = list(s)
            assert got == ref[f'group_{seed}_{spg}'].tolist() and len(s) == len(got)
            np.random.seed(seed)
            assert list(D.GroupSampler(ds, spg)) == got                   # the module-level generator is the default
            flags = ds.flag[np.array(got)].reshape(-1, spg)
            assert (flags == flags[:, :1]).all()                          # every batch from one group
    assert len(D.GroupSampler(ds, 2)) == 4 + 10 and len(D.GroupSampler(ds, 3)) == 12


def test_group_sampler_seed_and_epoch(ds):
    a, b = D.GroupSampler(ds, 2, seed=5), D.GroupSampler(ds, 2, seed=5)
    first = list(a)
    assert first == list(b)
    a.set_epoch(1)
    second = list(a)
    assert second != first and sorted(set(second)) == sorted(set(first)) == list(range(len(ds)))
    a.set_epoch(0)
    assert list(a) == first
    assert list(D.GroupSampler(ds, 2, seed=6)) != first


def test_distributed_group_sampler_orders(ds, ref):
    for world in (1, 2, 3):
        per_epoch = {0: [], 1: []}
        for rank in range(world):
            s = D.DistributedGroupSampler(ds, 2, world, rank, seed=7)
            for epoch in (0, 1):
                s.set_epoch(epoch)
                got = list(s)
                assert got == ref[f'dist_{world}_{rank}_{epoch}'].tolist() and len(s) == len(got), (world, rank, epoch)
                assert list(s) == got                                     # the same epoch gives the same order
                per_epoch[epoch].append(got)
        assert per_epoch[0] != per_epoch[1]                               # set_epoch changes it
        assert set(sum(per_epoch[0], [])) == set(range(len(ds)))
    assert len(D.DistributedGroupSampler(ds, 2, 3, 0)) == 2 + 4


def test_loader_refuses_bad_arguments(ds):
    for kw in (dict(on_unsupported='skip'), dict(prefetch=2), dict(rank=2, world=2)):
        with pytest.raises(ValueError):
            D.TrainLoader(ds, None, 2, **kw)
    with pytest.raises(ValueError, match='pipeline'):
        pkg.build_train_loader(dict(type='CocoDataset', ann_file=ANN, classes=('cat', 'dog')), 2)
