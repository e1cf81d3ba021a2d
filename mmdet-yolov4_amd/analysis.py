"""Which images does the detector get wrong: per-image mAP on the GPU and the good / bad gallery of
``tools/analysis_tools/analyze_results.py`` (``bbox_map_eval``, ``ResultVisualizer``).

The reference scores one image at a time: ten ``eval_map`` calls per image (``np.linspace(.5, .95, 10)``), each of which
opens a process pool and recomputes the IoU matrix.  ``image_maps`` scores every image of a dataset in one pass.  The
(image, class) problems are the ones ``eval_map``'s flat path already handles for a whole dataset -- ``yv4_map_rank``,
ONE ``yv4_bbox_overlaps_batched`` and ONE ``yv4_tpfp_batched`` for the ten thresholds -- and csrc/map_image.hip
accumulates per problem instead of per class (``yv4_map_image_ap``) and averages per image (``yv4_map_image_mean``).
One read-back brings the result.

Parity: bit-exact against the reference's ``bbox_map_eval`` as numpy 2.2 evaluates it, wherever no two detections of
one (image, class) share a score (``tests/golden/image_map.npz``).  Three rules carry that, beyond ``map_eval``'s:

Thresholds.  ``bbox_map_eval`` hands ``eval_map`` ``np.float64`` scalars, and numpy 2 compares a float32 IoU with an
``np.float64`` scalar in float64 -- unlike the Python floats of ``map_eval``'s docstring, which compare in float32.  For
a float32 ``x``, ``x >= thr`` in float64 holds exactly when ``x >= ceil32(thr)``, the smallest float32 not below ``thr``:
the kernels keep their float32 comparison and the host hands them ``ceil32`` of every threshold.  An IoU of exactly
``float32(0.7)`` is then a miss at 0.7, as in the reference (``float32(0.7) < 0.7``).

The mean over classes.  ``np.array(aps).mean()`` over the float32 APs of the classes that have gts is numpy's PAIRWISE
float32 sum and one float32 division: fewer than 8 values are added left to right from 0; 8 to 128 go through eight
accumulators; more are split in halves (``yv4.h`` states it; ``tests/_image_map_ref.py`` restates it).

The mean over thresholds is Python's ``sum(mean_aps) / len(mean_aps)``: float64, left to right from 0.

Ties.  List input goes through the same flat path (``flatten_results``), so equal scores inside an (image, class) fall
as the flat path's do: stable, in table order -- the difference from the list path that ``map_eval`` states.
"""
import os

import numpy as np
import torch

from . import _eval_common, _lib, image_io
from ._eval_common import PhaseTimer, _dev, _flat_to_device, _is_flat, _ptr, rank_flat
from ._lib import check
from .coco_eval import flatten_results
from .draw import draw_gt_det_into
from .map_eval import MapGt
from .ops import stream_ptr


def default_iou_thrs():
    """``bbox_map_eval``'s thresholds: ten ``np.float64`` values."""
    return np.linspace(0.5, 0.95, 10)


def ceil32(thr):
    """The smallest float32 not below each float64 threshold: for a float32 ``x``, ``x >= np.float64(thr)`` (compared
    in float64) holds exactly when ``x >= ceil32(thr)`` (compared in float32)."""
    t = np.asarray(thr, np.float64)
    f = t.astype(np.float32)
    low = f.astype(np.float64) < t
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _device():
    return _eval_common._device('image_maps', 'map_image')


def _as_flat(results):
    """``(flat, num_classes or None)`` of the per-image lists, the flat tuple or a ``DeviceResults``."""
    if hasattr(results, 'tensors') and hasattr(results, 'num_classes'):
        return results.tensors(), int(results.num_classes)
    if _is_flat(results):
        return results, None
    return flatten_results(results), (len(results[0]) if len(results) else None)


def image_maps_device(flat, gt, iou_thrs=None, phases=None):
    """The device pass behind ``image_maps``.  ``flat``: ``(dets, labels, img_index)``, numpy arrays or GPU tensors
    (those never visit the host); ``gt``: a ``MapGt``.  Returns ``(image_map (N,) float64, image_map_thr (T, N) float32)``
    host arrays.  ``phases``: an optional dict that receives seconds per phase (each closed by a synchronise)."""
    dev = _device()
    timer = PhaseTimer(phases, dev)
    thrs = ceil32(default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1))
    T = len(thrs)
    if T == 0:
        raise ValueError('image_maps needs at least one IoU threshold')
    N, C = gt.num_imgs, gt.num_classes
    P, G = N * C, len(gt.gt)
    g = gt.device(dev)
    flat = _flat_to_device(flat, dev)
    t_thr = _dev(thrs, np.float32, dev)
    timer.mark('upload')
    lib = _lib.lib()
    det4, det_off, iou_off, order, rank, cls_order, pairs, Dv, counts = rank_flat(flat, g['gt_off'], N, C, dev)
    timer.mark('rank')
    iou = torch.empty(max(pairs, 1), dtype=torch.float32, device=dev)
    if pairs:
        check(lib.yv4_bbox_overlaps_batched(det4.data_ptr(), g['gt'].data_ptr(), det_off.data_ptr(), g['gt_off'].data_ptr(),
                                            iou_off.data_ptr(), P, pairs, _lib.OVERLAPS_IOU, float(np.float32(1e-6)),
                                            iou.data_ptr(), stream_ptr()), 'yv4_bbox_overlaps_batched')
    else:
        iou.zero_()
    tp = torch.empty((T, 1, Dv), dtype=torch.uint8, device=dev)
    fp = torch.empty((T, 1, Dv), dtype=torch.uint8, device=dev)
    if Dv:
        work = torch.empty(max(int(lib.yv4_tpfp_work(_lib.TPFP_DEFAULT, Dv, G, T)), 4), dtype=torch.uint8, device=dev)
        check(lib.yv4_tpfp_batched(_lib.TPFP_DEFAULT, det4.data_ptr(), _ptr(g['gt']), _ptr(g['ign']), None, None,
                                   rank.data_ptr(), det_off.data_ptr(), g['gt_off'].data_ptr(), iou_off.data_ptr(), P, Dv, G,
                                   iou.data_ptr(), t_thr.data_ptr(), T, None, 1, work.data_ptr(), tp.data_ptr(), fp.data_ptr(),
                                   stream_ptr()), 'yv4_tpfp_batched')
    timer.mark('tpfp')
    ap = torch.empty((T, P), dtype=torch.float32, device=dev)
    ngt = torch.empty(P, dtype=torch.int32, device=dev)
    work = torch.empty(max(int(lib.yv4_map_image_ap_work(Dv)), 4), dtype=torch.uint8, device=dev)
    # both results in one buffer, so that one copy brings them: image_map (N) float64, then image_map_thr (T, N) float32
    out = torch.empty(8 * N + 4 * T * N, dtype=torch.uint8, device=dev)
    check(lib.yv4_map_image_ap(_ptr(tp), _ptr(fp), tp.numel(), det_off.data_ptr(), g['gt_off'].data_ptr(),
                               min(det_off.numel(), g['gt_off'].numel()), _ptr(g['ign']), G, Dv, N, C, T, work.data_ptr(),
                               work.numel(), ap.data_ptr(), ap.numel(), ngt.data_ptr(), ngt.numel(), stream_ptr()),
          'yv4_map_image_ap')
    check(lib.yv4_map_image_mean(ap.data_ptr(), ap.numel(), ngt.data_ptr(), ngt.numel(), N, C, T, out.data_ptr(), N,
                                 out.data_ptr() + 8 * N, T * N, stream_ptr()), 'yv4_map_image_mean')
    timer.mark('accumulate')
    host = out.cpu().numpy()                                   # the one read-back of the results
    timer.mark('download')
    return host[:8 * N].view(np.float64).copy(), host[8 * N:].view(np.float32).reshape(T, N).copy()


def image_maps(results, annotations, num_classes=None, iou_thrs=None, per_threshold=False):
    """``bbox_map_eval`` of every image at once: ``(N,)`` float64, image i's mAP over ``iou_thrs`` (default: the ten
    COCO thresholds).  ``results``: the per-image per-class lists, the flat ``(dets (D, 5), labels (D,), img_index
    (D,))`` of numpy arrays or GPU tensors, or a ``DeviceResults`` table; ``annotations``: the ``get_ann_info`` dicts or
    a cached ``MapGt``; ``num_classes``: needed only where neither says it.  ``per_threshold=True`` also returns the
    ``(T, N)`` float32 ``mean_ap`` of every image at every threshold."""
    flat, C = _as_flat(results)
    if isinstance(annotations, MapGt):
        gt = annotations
    else:
        C = num_classes if num_classes is not None else C
        if C is None:
            raise ValueError('flat results carry no class count: pass a MapGt or num_classes')
        gt = MapGt(annotations, C)
    if not _is_flat(results) and not hasattr(results, 'tensors') and len(results) != gt.num_imgs:
        raise ValueError(f'{len(results)} results for {gt.num_imgs} annotations')
    maps, per_thr = image_maps_device(flat, gt, iou_thrs)
    return (maps, per_thr) if per_threshold else maps


def bbox_map_eval(det_result, annotation):
    """The reference's ``bbox_map_eval``: the mAP of one image's per-class detections (or the ``bbox`` half of a
    ``(bbox, segm)`` tuple) against its annotation, over the ten COCO thresholds, as a Python float."""
    if isinstance(det_result, tuple):
        det_result = det_result[0]
    return float(image_maps([det_result], [annotation])[0])


def rank_images(maps, topk):
    """``(bad, good)``: lists of ``(index, mAP)`` -- the first and last ``topk`` of the images sorted by mAP, ascending
    and stable (equal scores stay in index order), as ``sorted(_mAPs.items(), key=lambda kv: kv[1])`` leaves them."""
    items = sorted(enumerate(maps), key=lambda kv: kv[1])
    return items[:topk], items[-topk:]


def clip_topk(topk, num_images):
    """``assert topk > 0``; ``topk * 2 > len(dataset)`` clips it to ``len // 2``."""
    assert topk > 0
    return num_images // 2 if topk * 2 > num_images else topk


def gallery_name(filename, mAP):
    """The output name of an image: ``fname + '_' + str(round(mAP, 3)) + ext``."""
    fname, ext = os.path.splitext(os.path.basename(filename))
    return fname + '_' + str(round(mAP, 3)) + ext


def _source_path(dataset, index):
    info = dataset.data_infos[index]
    prefix = getattr(dataset, 'img_prefix', None)
    return os.path.join(prefix, info['filename']) if prefix is not None else info['filename']


def _image_result(results, index, device):
    """Image ``index`` of the results for drawing: the per-class list, or its rows of the flat table."""
    if _is_flat(results):                           # already on the device (evaluate_and_show puts it there once)
        dets, labels, img_index = results
        rows = img_index == index
        return dets[rows], labels[rows]
    res = results[index]
    if isinstance(res, tuple):                      # (bbox, segm): the bbox half, as bbox_map_eval does
        if len(res) > 1 and res[1] is not None:
            raise NotImplementedError('analyze_results: a (bbox, segm) result carries masks, which are not built')
        res = res[0]
    return res


class ResultVisualizer(object):
    """``ResultVisualizer`` of ``analyze_results.py``: ranks the images of a dataset by their mAP and writes the ``topk``
    best and worst, ground truth and detections drawn, into ``show_dir/good`` and ``show_dir/bad``.  ``score_thr``:
    minimum score of the detections drawn.  There is no display: ``show=True`` raises ``NotImplementedError`` in
    ``evaluate_and_show``, as ``show_result`` does."""

    def __init__(self, show=False, wait_time=0, score_thr=0):
        self.show = show
        self.wait_time = wait_time
        self.score_thr = score_thr

    def _save_image_gts_results(self, dataset, results, mAPs, out_dir=None):
        """One directory: ONE ``imread`` of its files, the ground truth drawn, the detections over it, ONE encode, the
        files written on threads.  Returns the written paths."""
        os.makedirs(out_dir, exist_ok=True)
        if not mAPs:
            return []
        sources = [_source_path(dataset, index) for index, _ in mAPs]
        out_files = [os.path.join(out_dir, gallery_name(src, mAP)) for src, (_, mAP) in zip(sources, mAPs)]
        bufs = []
        for src in sources:
            with open(src, 'rb') as f:
                bufs.append(f.read())
        pixels, table = image_io.decode_into(bufs)
        places = [image_io.oriented_size(t) + (int(t.out_off), int(t.out_pitch)) for t in table]
        dev = pixels.device
        draw_gt_det_into(pixels, places, [dataset.get_ann_info(index) for index, _ in mAPs],
                         [_image_result(results, index, dev) for index, _ in mAPs], list(dataset.CLASSES),
                         score_thr=self.score_thr)
        image_io._write_files(image_io.encode_into(pixels, table), out_files, True)
        return out_files

    def evaluate_and_show(self, dataset, results, topk=20, show_dir='work_dir', eval_fn=None):
        """``dataset``: ``__len__``, ``get_ann_info``, ``data_infos[i]['filename']``, ``img_prefix`` and ``CLASSES``
        (``CocoDataset(test_mode=True)``; its cached ``MapGt`` is used where it has one as ``map_gt``).  ``results``: the
        per-image lists of a test run, or the flat table.  With ``eval_fn=None`` ONE ``image_maps`` call scores every
        image; a callable ``eval_fn(result, ann_info)`` is applied per image on the host, as the reference does.
        Returns ``(good, bad)``: the ``(index, mAP)`` lists."""
        topk = clip_topk(topk, len(dataset))
        if self.show:
            raise NotImplementedError('ResultVisualizer(show=True): there is no display window; the pictures go to show_dir')
        if eval_fn is None:
            gt = getattr(dataset, 'map_gt', None)
            if not isinstance(gt, MapGt):
                gt = [dataset.get_ann_info(i) for i in range(len(dataset))]
            maps = [float(m) for m in image_maps(results, gt, num_classes=len(dataset.CLASSES))]
        else:
            assert callable(eval_fn)
            maps = [eval_fn(result, dataset.get_ann_info(i)) for i, result in enumerate(results)]
        bad, good = rank_images(maps, topk) if topk else ([], [])
        if hasattr(results, 'tensors'):
            results = results.tensors()
        if _is_flat(results):                       # the rows of the chosen images are cut out on the device
            results = _flat_to_device(results, _device())
        good_dir = os.path.abspath(os.path.join(show_dir, 'good'))
        bad_dir = os.path.abspath(os.path.join(show_dir, 'bad'))
        # refuse a source the decoder cannot read before anything is written, by its name
        image_io.check_jpeg_paths([_source_path(dataset, index) for index, _ in good + bad], 'analyze_results')
        self._save_image_gts_results(dataset, results, good, good_dir)
        self._save_image_gts_results(dataset, results, bad, bad_dir)
        return good, bad
