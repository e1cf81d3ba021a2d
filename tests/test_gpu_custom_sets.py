"""The datasets beyond COCO on the GPU: a ``TrainLoader`` epoch over the ``.circle`` folder, over
``RepeatDataset(VOCDataset)`` and over a ``ConcatDataset`` of two pickles against the same samples composed by hand
through the pipeline objects, in every entropy mode and with ``prefetch``; the plain train pipeline's pixels against
``yv4_letterbox_u8_flip`` per image; and ``evaluate`` of every dataset and of ``ConcatDataset`` against what the
reference's own ``evaluate`` returns for the same detections (tests/golden/custom_sets.npz), from the per-image lists and
from the flat table on the device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd.ops import stream_ptr
from _custom_sets_data import EVAL_CASES, as_lists, as_proposals, circle_block, jpgs_of, plain_blocks, write_tree
from test_gpu_train_loader import MOSAIC, _assert_same, _epoch

pytestmark = pytest.mark.gpu

# the plain block of configs/_base_/datasets/voc0712.py at 48 .. 100 pixels; the two scales make 'range' draw
PLAIN = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
         dict(type='Resize', img_scale=[(64, 48), (100, 80)], keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
         dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
         dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
         dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


@pytest.fixture(scope='module')
def ref(golden):
    g = golden('custom_sets')
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def root(tmp_path_factory, golden):
    return write_tree(str(tmp_path_factory.mktemp('custom_sets_gpu') / 'sets'), jpgs_of(golden('custom_sets')))


def _train_cfg(root, name):
    b = plain_blocks(root)
    if name == 'circle':
        return dict(circle_block(root), pipeline=MOSAIC), True
    if name == 'repeat_voc':
        return dict(type='RepeatDataset', times=2, dataset=dict(b['{V07}'], pipeline=PLAIN)), False
    return dict(type='ConcatDataset', datasets=[dict(b['{A}'], pipeline=MOSAIC), dict(b['{B}'], pipeline=MOSAIC)]), True


def _owner(dataset, j):
    """``(dataset that owns the recorded sample j, its index)``: wrappers record ``(owner's number, index)``."""
    return (dataset.leaves()[j[0]], j[1]) if isinstance(j, tuple) else (dataset, j)


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['circle', 'repeat_voc', 'concat_pickles'])
def test_loader_batches_equal_the_composition_by_hand(root, gpu_device, name):
    cfg, mosaic = _train_cfg(root, name)
    loader = pkg.build_train_loader(cfg, 2, seed=5, device=gpu_device)
    ds = loader.dataset
    assert isinstance(loader.pipeline, pkg.FusedTrainPipeline if mosaic else pkg.PlainTrainPipeline)
    epoch = _epoch(loader)
    assert len(epoch) == len(loader) == {'circle': 3, 'repeat_voc': 3, 'concat_pickles': 3 + 5}[name]
    for img, boxes, labels, draws, metas in epoch:
        samples = []
        for index, group in zip(draws['indices'], draws['sources']):
            assert len(group) == (4 if mosaic else 1)
            if hasattr(ds, 'resolve'):                     # the sample and its partners: one owner, the owner's indices
                owner, i = ds.resolve(index)
                assert _owner(ds, group[0]) == (owner, i) and all(_owner(ds, j)[0] is owner for j in group)
            owner = _owner(ds, group[0])[0]
            inner = [_owner(ds, j)[1] for j in group]
            assert (owner.flag[inner] == owner.flag[inner[0]]).all()
            paths = [os.path.join(owner.img_prefix, owner.data_infos[i]['filename']) for i in inner]
            imgs = pkg.imread(paths, device=gpu_device, orientation=True)
            anns = [owner.get_ann_info(i) for i in inner]
            triples = [(im, a['bboxes'], a['labels']) for im, a in zip(imgs, anns)]
            samples.append(tuple(triples) if mosaic else triples[0])
        want = loader.pipeline(samples, params=draws['params'])
        assert img.tobytes() == want['img'].cpu().numpy().tobytes()
        for n in range(len(samples)):
            np.testing.assert_array_equal(boxes[n], want['gt_bboxes'][n].cpu().numpy())
            np.testing.assert_array_equal(labels[n], want['gt_labels'][n].cpu().numpy())
            assert labels[n].dtype == np.int64 and boxes[n].dtype == np.float32
        assert all(os.path.isfile(m['filename']) and m['filename'].endswith(m['ori_filename']) for m in metas)
    assert sum(len(b) for _, boxes, _, _, _ in epoch for b in boxes) > 0
    if name == 'concat_pickles':                           # both pickles were drawn from, each with its own prefix
        assert {g[0][0] for *_, d, _ in epoch for g in d['sources']} == {0, 1}
    # the same (seed, epoch, rank, world) gives the same bytes, in every entropy mode, with and without prefetch
    for entropy in ('host', 'device', 'device_sync'):
        for prefetch in (0, 1):
            again = pkg.build_train_loader(cfg, 2, seed=5, device=gpu_device, entropy=entropy, prefetch=prefetch)
            _assert_same(epoch, _epoch(again))
            again.close()
    ranks = [_epoch(pkg.build_train_loader(cfg, 2, seed=5, rank=1, world=2, device=gpu_device)) for _ in (0, 1)]
    _assert_same(ranks[0], ranks[1])
    loader.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def _letterbox_flip(src, rh, rw, ph, pw, pipe, flip):
    """``yv4_letterbox_u8_flip`` of one contiguous image into its own (3, ph, pw) image: Pad after Normalize, value 0."""
    h, w = int(src.shape[0]), int(src.shape[1])
    out = torch.empty((3, ph, pw), dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().yv4_letterbox_u8_flip(src.data_ptr(), h, w, 3 * w, out.data_ptr(), ph, pw, ph * pw, rh, rw,
                                                pipe.mean.ctypes.data_as(C.c_void_p), pipe.std.ctypes.data_as(C.c_void_p),
                                                int(pipe.to_rgb), 0, 0, flip, stream_ptr()), 'yv4_letterbox_u8_flip')
    return out


@pytest.mark.parametrize('divisor', [32, 1, 6])
def test_plain_pipeline_pixels_equal_letterbox_per_image(gpu_device, divisor):
    """Sources of 33 x 47, 64 x 48 and 48 x 64 (h x w), the second one a view inside a wider canvas, at scales that give
    odd widths (83 and 61).  ``size_divisor=32``: the canvas is 96 wide (16-byte stores, padded widths multiples of 4);
    6: it is 84 wide with padded widths of 66 and 72, so a group of four crosses an image's own border; 1: it is 83 wide
    (one float at a time)."""
    g = torch.Generator().manual_seed(7)
    canvas = torch.randint(0, 256, (70, 60, 3), dtype=torch.uint8, generator=g).to(gpu_device)
    srcs = [torch.randint(0, 256, (33, 47, 3), dtype=torch.uint8, generator=g).to(gpu_device), canvas[3:67, 5:53],
            torch.randint(0, 256, (48, 64, 3), dtype=torch.uint8, generator=g).to(gpu_device),
            torch.randint(0, 256, (33, 47, 3), dtype=torch.uint8, generator=g).to(gpu_device)]
    assert srcs[1].stride(0) == 180 and tuple(srcs[1].shape) == (64, 48, 3)
    pipe = pkg.build_train_pipeline([dict(t, size_divisor=divisor) if t['type'] == 'Pad' else t for t in PLAIN],
                                    device=gpu_device)
    # (scale, flip) as drawn; the resized extents are asserted below
    drawn = [((83, 58), None), ((85, 64), 'horizontal'), ((77, 51), 'vertical'), ((61, 43), 'diagonal')]
    pipe.flip_direction = 'diagonal'
    params = []
    for s, (scale, flip) in zip(srcs, drawn):
        rh, rw = pkg.augment.rescale_size(int(s.shape[0]), int(s.shape[1]), scale)
        params.append(dict(scale=scale, rh=rh, rw=rw, flip=flip))
    assert [(p['rh'], p['rw']) for p in params] == [(58, 83), (85, 64), (51, 68), (43, 61)]
    boxes = np.array([[2, 3, 20, 30]], np.float32)
    out = pipe([(s, boxes, np.array([1])) for s in srcs], params=params)
    img = out['img']
    pads = [pipe.pad_shape(p) for p in params]
    H, W = max(p[0] for p in pads), max(p[1] for p in pads)
    assert tuple(img.shape) == (4, 3, H, W) and (W % 4 == 0) == (divisor == 32 or divisor == 6)
    want = torch.zeros_like(img)
    for n, (s, p, (ph, pw)) in enumerate(zip(srcs, params, pads)):
        flip = 0 if p['flip'] is None else _lib.FLIP_CODES[p['flip']]
        want[n, :, :ph, :pw] = _letterbox_flip(s.contiguous(), p['rh'], p['rw'], ph, pw, pipe, flip)
    torch.cuda.synchronize()
    assert img.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert float(img[0, :, 58:, :].abs().max()) == 0 and float(img[:, :, :43, :61].abs().max()) > 0
    for n, (p, m) in enumerate(zip(params, out['img_metas'])):
        assert m['img_shape'] == (p['rh'], p['rw'], 3) and m['pad_shape'] == pads[n] + (3,) and m['flip'] == (p['flip'] is not None)
        got, _, sf = pipe.transform_boxes(p, int(srcs[n].shape[0]), int(srcs[n].shape[1]), boxes, [1])
        np.testing.assert_array_equal(out['gt_bboxes'][n].cpu().numpy(), got)
        np.testing.assert_array_equal(m['scale_factor'], sf)
    with pytest.raises(TypeError, match='on the GPU'):
        pipe([(srcs[0].cpu(), boxes, [1])], params=params[:1])


# ---- evaluate against the reference's own --------------------------------------------------------------------------------
def _test_set(root, name):
    b = plain_blocks(root)
    test = dict(test_mode=True)
    if name == 'ts':
        return dict(circle_block(root), **test)
    if name in ('concat_sep', 'concat_joint'):
        return dict(type='ConcatDataset', separate_eval=name == 'concat_sep',
                    datasets=[dict(b['{A}'], **test), dict(b['{B}'], **test)])
    return dict(b[{'ca': '{A}', 'v07': '{V07}', 'v12': '{V12}'}[name]], **test)


@pytest.mark.parametrize('name', ['ca', 'v07', 'v12', 'ts', 'concat_sep', 'concat_joint'])
def test_evaluate_equals_the_reference(root, ref, gpu_device, name):
    ds = pkg.build_dataset(_test_set(root, name))
    flat = tuple(ref[f'det_{name}/{k}'] for k in ('dets', 'labels', 'img_index'))
    assert len(np.unique(flat[0][:, 4])) == len(flat[0])                                   # distinct scores: one order
    on_device = tuple(torch.from_numpy(a).to(gpu_device) for a in flat)
    assert ds.accepts_flat
    for case, kw in EVAL_CASES.items():
        want = {k[len(f'eval_{name}/{case}/'):]: float(v) for k, v in ref.items() if k.startswith(f'eval_{name}/{case}/')}
        assert want
        lists = as_proposals(flat, len(ds)) if kw['metric'] == 'recall' else as_lists(flat, len(ds), len(ds.CLASSES))
        for results in (lists, on_device, flat):
            got = ds.evaluate(results, logger='silent', **kw)
            assert list(got) == list(want), (name, case)
            assert {k: float(v) for k, v in got.items()} == want, (name, case)
    if name == 'v07':
        assert ds.year == 2007          # the 11-point form; v12 scores the area form on the same kind of data
    if name == 'ca':
        assert ds._map_gt is not None and ds.map_gt is ds.map_gt                           # built once, on first use
        with pytest.raises(NotImplementedError):
            pkg.CustomBBoxDataset.evaluate(ds, lists, metric='recall')                     # the base class keeps raising


def test_test_loader_walks_a_concat_dataset_in_order(root, gpu_device):
    """``build_test_loader`` over a ``ConcatDataset``: ``test_mode`` reaches both pickles (nothing is filtered), the order
    is the first dataset's images then the second's, each read under its own prefix."""
    b = plain_blocks(root)
    test = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(64, 64), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32),
                             dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    cfg = dict(type='ConcatDataset', datasets=[dict(b['{A}'], pipeline=test), dict(b['{B}'], pipeline=test)])
    loader = pkg.build_test_loader(cfg, samples_per_gpu=5, device=gpu_device, prefetch=1)
    ds = loader.dataset
    assert len(ds) == 12 + 5 and all(d.test_mode and not hasattr(d, 'flag') for d in ds.datasets) and ds.accepts_flat
    names = []
    for data in loader:
        assert data['img'][0].is_cuda and data['img'][0].shape[0] == len(data['img_metas'][0])
        names += [m['filename'] for m in data['img_metas'][0]]
    want = [os.path.join(root, 'img_a', f'a{i:02d}.jpg') for i in range(12)] + \
           [os.path.join(root, 'img_b', f'b{i:02d}.jpg') for i in range(5)]
    assert names == want
    loader.close()
