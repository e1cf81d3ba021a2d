"""The datasets beyond COCO, their wrappers and the plain train pipeline's host side without a GPU, against what the
reference's own classes return for the hand-made sources (``tests/golden/custom_sets.npz``,
make_golden_custom_sets.py): tables, flags, filtered names, partner draws draw for draw, sampler orders and repeat
indices exactly; every nesting form of ``build_dataset``; the refusals by name; the plain pipeline's draws and boxes
against a restatement of ``Resize`` / ``RandomFlip`` written here."""
import importlib.util
import json
import os
import pickle
import shutil
import warnings

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import datasets as D
from conftest import GOLDEN
from _custom_sets_data import (CLASSES_ABC, SEEDS, WRAPPER_FORMS, circle_block, fill, jpgs_of, plain_blocks, write_tree)


@pytest.fixture(scope='module')
def ref(golden):
    g = golden('custom_sets')
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def root(tmp_path_factory, golden):
    return write_tree(str(tmp_path_factory.mktemp('custom_sets') / 'sets'), jpgs_of(golden('custom_sets')))


@pytest.fixture(scope='module')
def blocks(root):
    return plain_blocks(root)


def build(cfg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)      # CustomDataset's "does not support filtering empty gt images"
        return pkg.build_dataset(dict(cfg, **kw) if isinstance(cfg, dict) else cfg)


def _same(got, want, what):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _tables(ds, ref, prefix, draws=True):
    assert [d['filename'] for d in ds.data_infos] == ref[f'{prefix}/names'].tolist(), prefix
    if f'{prefix}/flag' in ref:
        _same(ds.flag, ref[f'{prefix}/flag'], f'{prefix}/flag')
    else:
        assert not hasattr(ds, 'flag')
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        for key in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            if f'{prefix}/{key}_{i}' in ref:
                _same(ann[key], ref[f'{prefix}/{key}_{i}'], f'{prefix}/{key}_{i}')
        assert ds.get_cat_ids(i) == ref[f'{prefix}/cats_{i}'].tolist(), (prefix, i)
        assert all(type(c) is int for c in ds.get_cat_ids(i))
    if draws:
        for seed in SEEDS:
            rng = np.random.RandomState(seed)
            got = np.stack([ds.batch_rand_others(i, 3, rng) for i in range(len(ds))])
            np.testing.assert_array_equal(got, ref[f'{prefix}/others_{seed}'], err_msg=f'{prefix}/others_{seed}')
            rng = np.random.RandomState(seed)
            got = np.array([ds._rand_another(i, rng) for i in range(len(ds))])
            np.testing.assert_array_equal(got, ref[f'{prefix}/another_{seed}'], err_msg=f'{prefix}/another_{seed}')
            np.random.seed(seed)                              # the module-level generator is the default
            got = np.stack([ds.batch_rand_others(i, 3) for i in range(len(ds))])
            np.testing.assert_array_equal(got, ref[f'{prefix}/others_{seed}'])


def test_all_five_are_registered_under_the_references_names():
    for name in ('CustomDataset', 'XMLDataset', 'VOCDataset', 'TrafficSignDataset', 'GarbageDataset', 'RepeatDataset',
                 'ConcatDataset', 'ClassBalancedDataset', 'CocoDataset'):
        assert name in pkg.DATASETS, name
    assert issubclass(pkg.CustomDataset, pkg.CustomBBoxDataset) and pkg.CustomDataset.accepts_flat


# ---- CustomDataset -----------------------------------------------------------------------------------------------------
def test_middle_format_tables_flags_and_draws(blocks, ref):
    with pytest.warns(UserWarning, match='does not support filtering empty gt'):
        ca = pkg.build_dataset(blocks['{A}'])
    _tables(ca, ref, 'ca')
    _tables(build(blocks['{B}']), ref, 'cb')
    assert len(ca) == 11 and ca.valid_inds == [0, 1, 2] + list(range(4, 12))            # image 3 is 31 pixels wide
    assert set(np.unique(ca.flag)) == {0, 1} and ca.get_ann_info(3)['bboxes'].shape == (0, 4)      # a04: no boxes
    assert ca._map_gt is None and ca._annotations is None                                # nothing built for training
    t = build(blocks['{A}'], test_mode=True)
    assert len(t) == 12 and not hasattr(t, 'flag')


def test_json_twin_class_file_paths_and_refusals(root, blocks, ref, tmp_path):
    with open(os.path.join(root, 'middle_a.pkl'), 'rb') as f:
        infos = pickle.load(f)
    twin = [dict(d, ann={k: np.asarray(v).tolist() for k, v in d['ann'].items()}) for d in infos]
    with open(tmp_path / 'twin.json', 'w') as f:
        json.dump(twin, f)
    js = build(blocks['{A}'], ann_file=str(tmp_path / 'twin.json'), classes=os.path.join(root, 'classes_abc.txt'))
    assert list(js.CLASSES) == list(CLASSES_ABC)                                          # a file of names
    assert [d['filename'] for d in js.data_infos] == ref['ca/names'].tolist() and js.flag.tolist() == ref['ca/flag'].tolist()
    for i in range(len(js)):
        np.testing.assert_array_equal(np.asarray(js.get_ann_info(i)['bboxes'], np.float32).reshape(-1, 4), ref[f'ca/bboxes_{i}'])
        assert js.get_cat_ids(i) == ref[f'ca/cats_{i}'].tolist()
    with pytest.raises(NotImplementedError, match=r'list\.txt'):
        build(blocks['{A}'], ann_file=os.path.join(root, 'list.txt'))
    with pytest.raises(NotImplementedError, match="proposal_file='p.pkl'"):
        build(blocks['{A}'], proposal_file='p.pkl')
    with pytest.raises(NotImplementedError, match="seg_prefix='seg/'"):
        build(blocks['{A}'], seg_prefix='seg/')
    with pytest.raises(ValueError, match='Unsupported type'):
        build(blocks['{A}'], classes=3)
    rel = build(dict(type='CustomDataset', ann_file='middle_a.pkl', data_root=root, img_prefix='img_a/', classes=CLASSES_ABC,
                     seg_prefix=None, proposal_file=None))
    assert rel.ann_file == os.path.join(root, 'middle_a.pkl') and rel.img_prefix == os.path.join(root, 'img_a/')
    with pytest.raises(KeyError, match='metric bbox is not supported'):
        rel.evaluate([], metric='bbox')


# ---- XMLDataset / VOCDataset -------------------------------------------------------------------------------------------
def test_voc_tables_sizes_years_and_filters(root, blocks, ref, tmp_path):
    v07, v12 = build(blocks['{V07}']), build(blocks['{V12}'])
    _tables(v07, ref, 'v07')
    _tables(v12, ref, 'v12')
    assert (v07.year, v12.year) == (2007, 2012) and (v07._ap_dataset, v12._ap_dataset) == ('voc07', None)
    everything = build(blocks['{V07}'], test_mode=True)
    np.testing.assert_array_equal([[d['width'], d['height']] for d in everything.data_infos], ref['v07/wh'])
    assert everything.data_infos[2]['id'] == '000003' and ref['v07/wh'][2].tolist() == [48, 64]      # from the JPEG header
    assert [d['id'] for d in v07.data_infos] == ['000001', '000002', '000003']     # 000004: unlisted only; 000005: 30 wide
    assert len(v07.get_ann_info(1)['bboxes_ignore']) == 1                                 # the difficult object
    np.testing.assert_array_equal(v07.get_ann_info(1)['bboxes'], [[9, 11, 39, 59]])       # int(float(text)) - 1
    _tables(build(blocks['{V12}'], min_size=8), ref, 'v12m', draws=False)
    assert len(ref['v12m/bboxes_ignore_1']) == 1 and len(ref['v12/bboxes_ignore_1']) == 0      # the 6-pixel box
    _tables(build(blocks['{V07}'], filter_empty_gt=False), ref, 'v07e', draws=False)
    assert len(ref['v07e/names']) == 4
    shutil.copytree(os.path.join(root, 'VOC2007'), str(tmp_path / 'VOC07'))
    with pytest.raises(ValueError, match='Cannot infer dataset year'):
        build(blocks['{V07}'], img_prefix=str(tmp_path / 'VOC07'))
    with pytest.raises(AssertionError, match='can not be None'):
        pkg.XMLDataset(ann_file=blocks['{V07}']['ann_file'], img_prefix=blocks['{V07}']['img_prefix'])
    x = pkg.XMLDataset(ann_file=blocks['{V07}']['ann_file'], img_prefix=blocks['{V07}']['img_prefix'], classes=('dog',))
    assert [d['id'] for d in x.data_infos] == ['000001', '000003'] and x.get_cat_ids(0) == [0]


# ---- TrafficSignDataset / GarbageDataset -------------------------------------------------------------------------------
def test_traffic_sign_folder(root, ref):
    ts = build(circle_block(root))
    _tables(ts, ref, 'ts')
    assert ts.CLASSES == ('sign',) and ts.flag.tolist() == [0] * 6 and ts.difficulty_thresh == 100
    assert all('width' not in d and 'height' not in d for d in ts.data_infos)
    assert ts.img_ids == [f't{i:02d}' for i in range(8)]                                  # set by the load, before the filter
    _tables(build(circle_block(root), test_mode=True), ref, 'tsv', draws=False)
    assert len(ref['tsv/names']) == 8 and len(ref['tsv/bboxes_3']) == 1                   # t03: the w <= 0 row is dropped
    _tables(build(circle_block(root, difficulty_thresh=0), test_mode=True), ref, 'ts0', draws=False)
    assert len(ref['ts0/bboxes_0']) == 0 and len(ref['ts0/bboxes_ignore_0']) == 2
    tst = build(circle_block(root), ann_file=os.path.join(root, 'circle_img'), test_mode=True)
    assert [d['filename'] for d in tst.data_infos] == ref['tst/names'].tolist() == sorted(ref['tst/names'].tolist())
    assert all(d['ann'] == dict(bboxes=[], labels=[]) for d in tst.data_infos)


def test_garbage_dataset_class_agnostic(blocks, ref):
    ga = build(blocks['{A}'], type='GarbageDataset', class_agnostic=True)
    _tables(ga, ref, 'ga', draws=False)
    assert list(ga.CLASSES) == ['x'] and all((ga.get_ann_info(i)['labels'] == 0).all() for i in range(len(ga)))
    assert any(ga.data_infos[i]['ann']['labels'].any() for i in range(len(ga)))            # the copy was zeroed, not the file
    plain = build(blocks['{A}'], type='GarbageDataset')
    assert plain.get_ann_info(0) is not plain.data_infos[0]['ann']
    np.testing.assert_array_equal(plain.get_ann_info(0)['labels'], ref['ca/labels_0'])


# ---- wrappers and build_dataset ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(WRAPPER_FORMS))
def test_build_dataset_takes_every_nesting_form(blocks, ref, name):
    w = build(fill(WRAPPER_FORMS[name], blocks))
    assert len(w) == int(ref[f'{name}/len'])
    _same(w.flag, ref[f'{name}/flag'], f'{name}/flag')
    assert w.CLASSES == w.leaves()[0].CLASSES and w.pipeline == []
    leaves = w.leaves()
    for i in range(len(w)):
        assert w.get_cat_ids(i) == ref[f'{name}/cats_{i}'].tolist(), (name, i)
        ds, j = w.resolve(i)                              # the index map: down to the owner and back
        assert any(ds is leaf for leaf in leaves) and 0 <= j < len(ds)
        assert ds.get_cat_ids(j) == w.get_cat_ids(i) and ds.flag[j] == w.flag[i]
    owners = [w.resolve(i) for i in range(len(w))]
    if name in ('concat_ab', 'list_ab', 'ann_list'):
        assert [(leaves.index(d), j) for d, j in owners] == [(0, j) for j in range(11)] + [(1, j) for j in range(5)]
        assert w.resolve(-1) == w.resolve(len(w) - 1)
    if name == 'repeat_v07':
        assert [j for _, j in owners] == [0, 1, 2] * 3
    if name == 'concat_repeat':
        assert [(leaves.index(d), j) for d, j in owners] == [(0, j % 5) for j in range(10)] + [(1, j) for j in range(11)]
    if name == 'ann_list':
        assert w.separate_eval is False and [d.img_prefix[-6:] for d in leaves] == ['img_a/', 'img_b/']


def test_group_sampler_orders_over_wrappers(blocks, ref):
    for name in ('repeat_v07', 'concat_ab'):
        w = build(fill(WRAPPER_FORMS[name], blocks))
        for seed in (3, 4):
            got = list(D.GroupSampler(w, 2, rng=np.random.RandomState(seed)))
            assert got == ref[f'group_{name}_{seed}'].tolist(), (name, seed)


def test_class_balanced_repeat_factors(blocks, ref):
    for thr in (0.5, 0.9):
        w = build(dict(WRAPPER_FORMS['cbd_v'], oversample_thr=thr, dataset=fill('{VV}', blocks)))
        assert w.repeat_indices == ref[f'cbd_{thr}/repeat_indices'].tolist()
        _same(w.flag, ref[f'cbd_{thr}/flag'], f'cbd_{thr}/flag')
        assert [w.resolve(i)[1] for i in range(len(w))] == [r if r < 3 else r - 3 for r in w.repeat_indices]
    assert len(ref['cbd_0.9/repeat_indices']) > len(ref['cbd_0.5/repeat_indices']) > 6      # the rare classes repeat


def test_concat_refusals_name_what_they_refuse(blocks):
    coco = dict(type='CocoDataset', ann_file=os.path.join(GOLDEN, 'coco_train_set.json'), classes=('cat', 'dog'))
    with pytest.raises(NotImplementedError, match='concatenated CocoDataset as a whole'):
        build(dict(type='ConcatDataset', separate_eval=False, datasets=[coco, coco]))
    with pytest.raises(NotImplementedError, match='same types'):
        build(dict(type='ConcatDataset', separate_eval=False, datasets=[blocks['{A}'], dict(blocks['{A}'], type='GarbageDataset')]))
    both = build(dict(type='ConcatDataset', datasets=[coco, blocks['{A}']]))                # separately, any mix
    assert both.accepts_flat and len(both) == 12 + 11
    with pytest.raises(ValueError, match='should not exceed dataset length'):
        both.resolve(-24)


def test_loaders_resolve_samples_through_wrappers(blocks):
    w = build(fill(WRAPPER_FORMS['concat_repeat'], blocks))
    loader = D.TrainLoader(w, None, 2)
    assert loader._own(3) == (0, 3) and loader._own(7) == (0, 2) and loader._own(10) == (1, 0)
    assert loader._path((1, 0)).endswith(os.path.join('img_a', 'a00.jpg')) and loader._path((0, 2)).endswith('b02.jpg')
    assert loader._sibling((1, 0), np.int64(4)) == (1, 4) and loader._at((1, 4))[0] is w.leaves()[1]
    plain = D.TrainLoader(w.leaves()[1], None, 2)
    assert plain._own(3) == 3 and plain._at(3) == (w.leaves()[1], 3) and plain._sibling(3, np.int64(5)) == 5
    loader.close()
    plain.close()


# ---- the plain train pipeline's host side ------------------------------------------------------------------------------
PLAIN = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
         dict(type='Resize', img_scale=(1000, 600), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
         dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
         dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
         dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def _with(typ, **kw):
    return [dict(t, **kw) if t['type'] == typ else t for t in PLAIN]


def _reference_chain(rng, h, w, boxes, img_scale, mode, flip_ratio, direction):
    """``Resize`` (transforms.py:101-244, ``mmcv.imrescale``'s size rule) and ``RandomFlip`` (:384-452) restated for one
    image's boxes: the draws from ``rng`` in their order, the boxes in float32."""
    if len(img_scale) == 1:
        scale = img_scale[0]
    elif mode == 'range':
        long_edge = rng.randint(min(max(s) for s in img_scale), max(max(s) for s in img_scale) + 1)
        short_edge = rng.randint(min(min(s) for s in img_scale), max(min(s) for s in img_scale) + 1)
        scale = (long_edge, short_edge)
    else:
        scale = img_scale[rng.randint(len(img_scale))]
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    new_w, new_h = int(w * float(factor) + 0.5), int(h * float(factor) + 0.5)
    scale_factor = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
    bboxes = boxes * scale_factor
    bboxes[:, 0::2] = np.clip(bboxes[:, 0::2], 0, new_w)
    bboxes[:, 1::2] = np.clip(bboxes[:, 1::2], 0, new_h)
    cur_dir = rng.choice([direction, None], p=[flip_ratio, 1 - flip_ratio])
    if cur_dir is not None:
        flipped = bboxes.copy()
        if cur_dir in ('horizontal', 'diagonal'):
            flipped[..., 0::4] = new_w - bboxes[..., 2::4]
            flipped[..., 2::4] = new_w - bboxes[..., 0::4]
        if cur_dir in ('vertical', 'diagonal'):
            flipped[..., 1::4] = new_h - bboxes[..., 3::4]
            flipped[..., 3::4] = new_h - bboxes[..., 1::4]
        bboxes = flipped
    return scale, (new_h, new_w), None if cur_dir is None else str(cur_dir), bboxes, scale_factor


@pytest.mark.parametrize('img_scale,mode,direction', [((1000, 600), 'range', 'horizontal'),
                                                       ([(64, 48), (100, 80)], 'range', 'vertical'),
                                                       ([(64, 48), (96, 64), (75, 51)], 'value', 'diagonal')])
def test_plain_pipeline_draws_and_boxes_seed_for_seed(img_scale, mode, direction):
    block = _with('Resize', img_scale=img_scale, multiscale_mode=mode)
    block = [dict(t, direction=direction) if t['type'] == 'RandomFlip' else t for t in block]
    pipe = pkg.build_train_pipeline(block)
    assert isinstance(pipe, pkg.PlainTrainPipeline)
    scales = [tuple(s) for s in img_scale] if isinstance(img_scale, list) else [tuple(img_scale)]
    data = np.random.RandomState(99)
    flips = set()
    for seed in range(12):
        ours, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
        for h, w in ((33, 47), (64, 48), (48, 64), (375, 500)):
            n = data.randint(0, 4)
            boxes = (data.uniform(0, 1, (n, 4)) * [w, h, w, h]).astype(np.float32)
            boxes = np.concatenate([np.minimum(boxes[:, :2], boxes[:, 2:]), np.maximum(boxes[:, :2], boxes[:, 2:]) + 3], 1)
            p = pipe.draw_params(ours, h, w)
            got, labels, sf = pipe.transform_boxes(p, h, w, boxes, np.arange(n))
            scale, (rh, rw), flip, want, want_sf = _reference_chain(theirs, h, w, boxes, scales, mode, 0.5, direction)
            assert (p['scale'], p['rh'], p['rw'], p['flip']) == (tuple(int(v) for v in scale), rh, rw, flip)
            assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes()
            assert sf.tobytes() == want_sf.tobytes() and labels.tolist() == list(range(n))
            assert pipe.pad_shape(p) == (-(-rh // 32) * 32, -(-rw // 32) * 32)
            flips.add(flip)
        assert ours.randint(1 << 30) == theirs.randint(1 << 30)                          # the same number of draws
    assert flips == {None, direction}


def test_plain_pipeline_refuses_by_name():
    for block, match in ((_with('Resize', keep_ratio=False), 'keep_ratio=False'),
                         (_with('Resize', ratio_range=(0.5, 1.5)), 'ratio_range'),
                         (_with('Resize', interpolation='nearest'), "option 'interpolation'"),
                         (_with('Resize', multiscale_mode='cubic'), "multiscale_mode='cubic'"),
                         (_with('RandomFlip', flip_ratio=[0.3, 0.3]), 'flip_ratio must be one float'),
                         (_with('RandomFlip', direction=['horizontal', 'vertical']), 'direction lists'),
                         (_with('Pad', size=(64, 64)), 'size= is not built'),
                         (_with('Pad', pad_val=114), 'pad_val=0'),
                         (_with('Normalize', eps=1), "option 'eps'"),
                         (_with('LoadImageFromFile', to_float32=True), 'to_float32=True'),
                         (_with('LoadAnnotations', with_mask=True), 'with_mask'),
                         (PLAIN[:4] + [PLAIN[5], PLAIN[4]] + PLAIN[6:], 'order'),
                         (PLAIN[:3] + PLAIN[4:], 'order'),
                         (PLAIN[:4] + [dict(type='CutOut', n_holes=1)] + PLAIN[4:], "'CutOut' is not built")):
        with pytest.raises(NotImplementedError, match=match):
            pkg.build_train_pipeline(block)
    with pytest.raises(NotImplementedError, match='no fused train pipeline'):
        pkg.build_train_pipeline([dict(type='LoadImageFromFile'), dict(type='Normalize', mean=[0] * 3, std=[1] * 3)])


def test_recipe_blocks_build(root):
    """The traffic-sign recipe's parsed settings (custom_sets_recipe.json): its dataset type is registered and takes the
    recipe's keys; its train pipeline is the mosaic one; its model block builds."""
    with open(os.path.join(GOLDEN, 'custom_sets_recipe.json')) as f:
        recipe = json.load(f)
    train = recipe['data']['train']
    assert train['type'] == 'TrafficSignDataset' and recipe['evaluation']['metric'] == 'mAP'
    ds = pkg.build_dataset(dict(train, ann_file=os.path.join(root, 'circle'), img_prefix=os.path.join(root, 'circle_img')))
    assert len(ds) == 6 and ds.pipeline == train['pipeline']
    assert isinstance(pkg.build_train_pipeline(train['pipeline']), pkg.FusedTrainPipeline)
    head = recipe['model']['bbox_head']
    assert head['class_agnostic'] is True and head['num_classes'] == 1 and len(head['anchor_generator']['strides']) == 4
    assert recipe['model']['backbone']['out_indices'] == [2, 3, 4, 5]


# ---- the split tool's host side ----------------------------------------------------------------------------------------
def split_tool():
    spec = importlib.util.spec_from_file_location('tool_tencent_image_split',
                                                  os.path.join(os.path.dirname(GOLDEN), os.pardir, 'tools', 'tencent_image_split.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name,w,h', [('big', 100, 70), ('fit', 64, 48), ('small', 40, 30)])
def test_split_tool_offsets_and_labels_equal_the_reference(ref, name, w, h):
    """Tile (64, 48), overlap (16, 16): 100 x 70 steps to 48 / 32 and is clamped to 36 / 22; 64 x 48 is one whole tile;
    40 x 30 one short tile."""
    T = split_tool()
    tiles = T.tiles_of(h, w, T.parse_annotation(ref[f'split/{name}/rows'].tolist()), (64, 48), (16, 16))
    assert [f'{name}_{t[0]}_{t[1]}' for t in tiles] == ref[f'split/{name}/tiles'].tolist()
    np.testing.assert_array_equal([[t[0], t[1]] for t in tiles], ref[f'split/{name}/offsets'])
    np.testing.assert_array_equal([[t[2], t[3]] for t in tiles], ref[f'split/{name}/shapes'])
    for t in tiles:
        assert ''.join(t[4]) == str(ref[f'split/{name}/label/{name}_{t[0]}_{t[1]}'])
    if name == 'big':
        assert ref['split/big/offsets'].tolist() == [[0, 0], [36, 0], [0, 22], [36, 22]]
        assert sum(len(t[4]) for t in tiles) > 4                     # a centre in the overlap goes to several tiles
    if name == 'small':
        assert ref['split/small/shapes'].tolist() == [[30, 40]]
