"""Boxes without a score on the GPU (``YV4_DRAW_NO_SCORE``): ``draw_boxes`` with ``(k, 4)`` boxes against the numpy
restatement (tests/_draw_gt_ref.py) and the host twin, ``imshow_gt_det_bboxes`` against two successive reference
draws, and ``yv4_draw_boxes`` against ``yv4_draw_boxes_ex(flags=0)``."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import draw as DR

import _draw_data as D
import _draw_gt_data as G
import _draw_gt_ref as GR
import _draw_ref as R

pytestmark = pytest.mark.gpu


def _gpu(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


@pytest.mark.parametrize('name', sorted(G.cases()))
def test_boxes_without_score_equal_the_restatement_and_the_host_twin(name, gpu_device):
    img, boxes, labels, names, style = G.cases()[name]
    src = _gpu(img, gpu_device)
    got, = pkg.draw_boxes([src], [_gpu(boxes, gpu_device)], [_gpu(labels, gpu_device, np.int64)], names, **style)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, GR.draw_gt(img, boxes, labels, names, **style))
    np.testing.assert_array_equal(got, DR.draw_boxes_host(img, boxes, labels, names, **style))
    np.testing.assert_array_equal(src.cpu().numpy(), img)
    # no box is skipped by score_thr
    again, = pkg.draw_boxes([src], [_gpu(boxes, gpu_device)], [_gpu(labels, gpu_device, np.int64)], names, score_thr=2.0,
                            **style)
    np.testing.assert_array_equal(again.cpu().numpy(), got)


def test_batch_without_scores_in_one_launch(gpu_device):
    imgs, dets, labels = D.batch()
    boxes = [d[:, :4] for d in dets]
    got = pkg.draw_boxes([_gpu(a, gpu_device) for a in imgs], [_gpu(b, gpu_device) for b in boxes],
                         [_gpu(l, gpu_device, np.int64) for l in labels], D.NAMES, thickness=3)
    for g, a, b, l in zip(got, imgs, boxes, labels):
        np.testing.assert_array_equal(g.cpu().numpy(), GR.draw_gt(a, b, list(l), D.NAMES, thickness=3))
    with pytest.raises(ValueError, match='all'):
        pkg.draw_boxes([_gpu(a, gpu_device) for a in imgs], [_gpu(boxes[0], gpu_device), _gpu(dets[1], gpu_device),
                                                             _gpu(dets[2], gpu_device)],
                       [_gpu(l, gpu_device, np.int64) for l in labels], D.NAMES)


def test_imshow_gt_det_bboxes_equals_two_reference_draws(gpu_device, tmp_path):
    img = D.image(72, 104, 41)
    gt = np.array([[6.0, 8.0, 60.0, 50.0], [40.0, 30.0, 120.0, 90.0]], np.float32)
    gt_labels = np.array([0, 2])
    result = [np.array([[8.0, 6.0, 58.0, 52.0, 0.91], [70.0, 10.0, 90.0, 30.0, 0.2]], np.float32), np.zeros((0, 5), np.float32),
              np.array([[38.0, 33.0, 110.0, 80.0, 0.55]], np.float32)]
    dets = np.concatenate(result)
    det_labels = [0, 0, 2]
    for ann in (dict(gt_bboxes=gt, gt_labels=gt_labels), dict(bboxes=gt, labels=gt_labels)):
        got = pkg.imshow_gt_det_bboxes(_gpu(img, gpu_device), ann, result, D.NAMES[:3])
        assert got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), GR.draw_gt_det(img, gt, gt_labels, dets, det_labels, D.NAMES[:3]))
    # the reference's defaults: ground truth in (255, 102, 61), detections in (72, 101, 241), score_thr 0
    first = GR.draw_gt(img, gt, gt_labels, D.NAMES[:3], (255, 102, 61), (255, 102, 61))
    np.testing.assert_array_equal(got.cpu().numpy(), R.draw(first, dets, det_labels, D.NAMES[:3], score_thr=0))
    # a threshold, a numpy image, a (bbox, None) tuple and an output file
    out_file = str(tmp_path / 'sub' / 'drawn.jpg')
    got = pkg.imshow_gt_det_bboxes(img, dict(gt_bboxes=gt, gt_labels=gt_labels), (result, None), D.NAMES[:3], score_thr=0.3,
                                   thickness=1, out_file=out_file)
    want = GR.draw_gt_det(img, gt, gt_labels, dets, det_labels, D.NAMES[:3], score_thr=0.3, thickness=1)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert open(out_file, 'rb').read() == pkg.imencode(want)
    with pytest.raises(NotImplementedError, match='masks'):
        pkg.imshow_gt_det_bboxes(img, dict(gt_bboxes=gt, gt_labels=gt_labels), (result, [[]]), D.NAMES[:3])
    with pytest.raises(NotImplementedError, match='masks'):
        pkg.imshow_gt_det_bboxes(img, dict(gt_bboxes=gt, gt_labels=gt_labels, gt_masks=object()), result, D.NAMES[:3])
    with pytest.raises(NotImplementedError, match='display'):
        pkg.imshow_gt_det_bboxes(img, dict(gt_bboxes=gt, gt_labels=gt_labels), result, D.NAMES[:3], show=True)


def test_draw_boxes_is_the_ex_call_with_flags_zero(gpu_device):
    imgs, dets, labels = D.batch()
    lib = pkg._lib.lib()
    offs, end = [], 0
    for a in imgs:
        offs.append(end)
        end += (a.size + 255) // 256 * 256
    places = [(a.shape[0], a.shape[1], o, 3 * a.shape[1]) for o, a in zip(offs, imgs)]
    table, total = DR._tables(places, [len(d) for d in dets])
    st = DR._style(len(D.NAMES), 0.3, (72, 101, 241), (72, 101, 241), 2, 13)
    host = np.zeros(end, np.uint8)
    for o, a in zip(offs, imgs):
        host[o:o + a.size] = a.reshape(-1)
    table_dev = _gpu(np.frombuffer(bytes(table), np.uint8).copy(), gpu_device)
    names = _gpu(DR.name_table(D.NAMES).reshape(-1), gpu_device)
    d = _gpu(np.concatenate(dets), gpu_device, np.float32)
    lab = _gpu(np.concatenate(labels), gpu_device, np.int32)
    stream = pkg.ops.stream_ptr()
    a, b, c = (_gpu(host, gpu_device) for _ in range(3))
    assert lib.yv4_draw_boxes(table, table_dev.data_ptr(), len(table), a.data_ptr(), a.numel(), d.data_ptr(), lab.data_ptr(),
                              total, names.data_ptr(), C.byref(st), stream) == 0
    assert lib.yv4_draw_boxes_ex(table, table_dev.data_ptr(), len(table), b.data_ptr(), b.numel(), d.data_ptr(),
                                 lab.data_ptr(), total, names.data_ptr(), C.byref(st), 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    for o, img, dd, ll in zip(offs, imgs, dets, labels):
        np.testing.assert_array_equal(a[o:o + img.size].cpu().numpy().reshape(img.shape), R.draw(img, dd, list(ll), D.NAMES))
    # an unknown flag is refused before the launch
    assert lib.yv4_draw_boxes_ex(table, table_dev.data_ptr(), len(table), c.data_ptr(), c.numel(), d.data_ptr(),
                                 lab.data_ptr(), total, names.data_ptr(), C.byref(st), 4, stream) == -1
    torch.cuda.synchronize()
    assert torch.equal(c.cpu(), torch.from_numpy(host))
