"""Drawing on the GPU against the numpy restatement (tests/_draw_ref.py), bit for bit; ``show_result`` on a tiny
detector; ``single_gpu_test(out_dir=...)`` over a four-image test loader."""
import json
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from conftest import GOLDEN

import _draw_data as D
import _draw_ref as R
import _eval_hook_data as DATA

pytestmark = pytest.mark.gpu


def _gpu(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize('name', sorted(D.cases()))
def test_kernel_equals_the_restatement(name, gpu_device):
    img, dets, labels, names, style = D.cases()[name]
    src = torch.from_numpy(img).to(gpu_device)
    got, = pkg.draw_boxes([src], _gpu([dets], gpu_device), _gpu([np.asarray(labels, np.int64)], gpu_device), names, **style)
    np.testing.assert_array_equal(got.cpu().numpy(), R.draw(img, dets, labels, names, **style))
    np.testing.assert_array_equal(src.cpu().numpy(), img)             # draw_boxes draws on a copy


def test_batch_of_three_sizes_in_place_behind_guards(gpu_device):
    """0, 1 and 40 boxes in one launch, every image at a wider pitch in a guarded buffer: the kernel equals the
    restatement, and no byte outside frames and labels -- guard columns included -- changes."""
    imgs, dets, labels = D.batch()
    places, end = [], 64
    for a in imgs:
        pitch = 3 * a.shape[1] + 7
        places.append((a.shape[0], a.shape[1], end, pitch))
        end += pitch * a.shape[0] + 64
    host = np.full(end, 0x5A, np.uint8)
    want = host.copy()
    for a, d, lab, (h, w, off, pitch) in zip(imgs, dets, labels, places):
        drawn = R.draw(a, d, lab, D.NAMES, score_thr=0.3)
        for y in range(h):
            host[off + y * pitch:off + y * pitch + 3 * w] = a[y].reshape(-1)
            want[off + y * pitch:off + y * pitch + 3 * w] = drawn[y].reshape(-1)
    flat = torch.from_numpy(host).to(gpu_device)
    pkg.draw_boxes_into(flat, places, _gpu(dets, gpu_device), _gpu(labels, gpu_device), D.NAMES, score_thr=0.3)
    got = flat.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert (want != host).any() and (want == host).mean() > 0.5      # something was drawn, most pixels were not touched
    flat2 = torch.from_numpy(host).to(gpu_device)                   # two runs: identical bytes
    pkg.draw_boxes_into(flat2, places, _gpu(dets, gpu_device), _gpu(labels, gpu_device), D.NAMES, score_thr=0.3)
    assert torch.equal(flat, flat2)
    with pytest.raises(pkg._lib.Yv4Error, match='outside the buffer'):      # refused before the launch
        pkg.draw_boxes_into(flat[:end - 100], places, _gpu(dets, gpu_device), _gpu(labels, gpu_device), D.NAMES)


def _detector(dev):
    det = DATA.tiny_v4(DATA.make_test_cfg(), dev)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for conv in det.bbox_head.convs_pred:
            conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=gen))
            conv.bias.zero_()
    return det


def test_show_result(tmp_path, gpu_device):
    det = _detector(gpu_device)
    img = D.image(96, 128, 21)
    res = [np.array([[10, 12, 70, 60, 0.9], [30, 30, 50, 90, 0.2]], np.float32), np.zeros((0, 5), np.float32),
           np.array([[60, 5, 120, 80, 0.5]], np.float32)][:DATA.NUM_CLASSES]
    res += [np.zeros((0, 5), np.float32)] * (DATA.NUM_CLASSES - len(res))
    names = [f'class {k}' for k in range(DATA.NUM_CLASSES)]
    flat_d = np.concatenate(res)
    flat_l = np.concatenate([np.full(len(r), k) for k, r in enumerate(res)])
    want = R.draw(img, flat_d, flat_l, names)
    out = det.show_result(img, res)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    pair = (torch.from_numpy(flat_d).to(gpu_device), torch.from_numpy(flat_l).to(gpu_device))
    np.testing.assert_array_equal(det.show_result(torch.from_numpy(img).to(gpu_device), pair).cpu().numpy(), want)
    det.CLASSES = ('cat', 'dog', 'bird', 'fish')[:DATA.NUM_CLASSES]
    np.testing.assert_array_equal(det.show_result(img, res, bbox_color='red', thickness=1).cpu().numpy(),
                                  R.draw(img, flat_d, flat_l, det.CLASSES, bbox_color='red', thickness=1))
    # a file name in, a file out: decoded and encoded on the device
    src = tmp_path / 'in.jpg'
    pkg.imwrite(img, src)
    out_file = tmp_path / 'shown' / 'out.jpg'
    assert det.show_result(str(src), res, out_file=str(out_file)) is None
    back = pkg.imread(out_file, device=gpu_device)
    assert tuple(back.shape) == (96, 128, 3)
    drawn = det.show_result(str(src), res)
    assert out_file.read_bytes() == pkg.imencode(drawn)
    with pytest.raises(NotImplementedError, match='display'):
        det.show_result(img, res, show=True)
    with pytest.raises(NotImplementedError, match='masks'):
        det.show_result(img, (res, [[] for _ in res]))
    with pytest.raises(NotImplementedError, match='PNG'):
        det.show_result(img, res, out_file=str(tmp_path / 'out.png'))
    with pytest.raises(NotImplementedError, match='masks'):
        det.show_result(img, res, mask_color=(0, 255, 0))


def test_single_gpu_test_out_dir(tmp_path, golden, gpu_device):
    g = golden('coco_train_set')
    with open(os.path.join(GOLDEN, 'coco_train_set.json')) as f:
        d = json.load(f)
    d['images'] = d['images'][:4]
    keep = {im['id'] for im in d['images']}
    d['annotations'] = [a for a in d['annotations'] if a['image_id'] in keep]
    root = tmp_path / 'set'
    (root / 'img').mkdir(parents=True)
    (root / 'ann.json').write_text(json.dumps(d))
    for im in d['images']:
        (root / 'img' / im['file_name']).write_bytes(g[f"jpg_{im['id']}"].tobytes())
    norm = dict(mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True)
    pipeline = [dict(type='LoadImageFromFile'),
                dict(type='MultiScaleFlipAug', img_scale=(64, 64), flip=False,
                     transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                 dict(type='Pad', size_divisor=32), dict(type='Normalize', **norm),
                                 dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    cfg = dict(type='CocoDataset', ann_file='ann.json', data_root=str(root), img_prefix='img/',
               classes=('cat', 'dog', 'bird'), pipeline=pipeline, samples_per_gpu=3)
    det = _detector(gpu_device)
    loader = pkg.build_test_loader(cfg, device=gpu_device)
    want = pkg.single_gpu_test(det, loader)
    out_dir = tmp_path / 'shown'
    got = pkg.single_gpu_test(det, loader, out_dir=str(out_dir), show_score_thr=0.05)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert sorted(os.listdir(out_dir)) == sorted(im['file_name'] for im in d['images'])
    for im, res in zip(d['images'], want):
        src = pkg.imread(root / 'img' / im['file_name'], device=gpu_device)
        assert (out_dir / im['file_name']).read_bytes() == pkg.imencode(det.show_result(src, res, score_thr=0.05))
    with pytest.raises(ValueError, match='flat'):
        pkg.single_gpu_test(det, loader, flat=True, out_dir=str(out_dir))
    with pytest.raises(NotImplementedError, match='display'):
        pkg.single_gpu_test(det, loader, show=True)

    class NoName:
        def __iter__(self):
            for data in loader:
                metas = data['img_metas']
                nested = isinstance(metas[0], (list, tuple))
                for m in (metas[0] if nested else metas):
                    m.pop('filename', None)
                yield data

    with pytest.raises(ValueError, match='filename'):
        pkg.single_gpu_test(det, NoName(), out_dir=str(out_dir))
