"""VOC-style mean average precision: ``bbox_overlaps`` / ``tpfp_default`` / ``tpfp_imagenet`` / ``eval_map`` under the
reference's names, and ``evaluate_map``, the ``metric='mAP'`` branch of ``CustomDataset.evaluate``.

Mirror of ``mmdet/core/evaluation/bbox_overlaps.py`` and ``mean_ap.py`` (reached through
``datasets/custom.py:280-337`` and ``datasets/voc.py:27-98``).  Where the reference walks every (image, class) pair in
Python over a process pool, once per IoU threshold, and recomputes the IoU matrix each time, ``eval_map`` here gathers
every problem of the dataset into one table (class-major, so that a class's detections are one contiguous slice) and
evaluates it with ONE ``yv4_bbox_overlaps_batched`` call and ONE ``yv4_tpfp_batched`` call for all thresholds and area
ranges (csrc/map_eval.hip).  The accumulation into recall / precision / AP stays on the host in numpy, in the
reference's dtypes: a float32 cumulative sum (exact below 2**24 detections per class; more raises), ``recall`` float64
(a float32 count over ``np.maximum(int64 num_gts, float32 eps)``), ``precision`` and ``ap`` float32.  There is no CPU
implementation of the ops in this package: without a GPU they raise.

Parity: bit-exact against the reference as numpy 2.2 evaluates it.  Three rules carry that claim.

Sorting.  The visiting order inside a problem and the per-class global order are ``np.argsort(-scores)`` on the host:
the reference's very call.  numpy's default sort is not stable (already at 16 elements its tie order differs from
``kind='stable'``) and its tie order may depend on the host CPU, so making the same call on the same host is the only
way to order exact score ties as the reference would there.  The kernels take the order as an input.

Thresholds.  The reference compares a float32 IoU (or area) with a Python float.  Under numpy 2 that comparison is made
in float32 -- ``np.float32(0.7) >= 0.7`` is True -- so IoU thresholds and area bounds are rounded to float32 once on
the host and compared in float32 on the device.  numpy 1.x, the reference's era, promoted the float32 to float64 and
answered False for that pair; results on an IoU that equals a rounded threshold differ between the two.

Boxes.  Boxes are float32, which is what the reference's dataset loaders produce.  float64 annotation boxes are rounded
to float32 first; the reference would have computed their areas and (in ``tpfp_imagenet``) thresholds in float64.  This
is a stated deviation.  Boxes are expected to be finite.

The flat form.  ``eval_map`` / ``evaluate_map`` also take ``(dets (D, 5), labels (D,), img_index (D,))`` as numpy arrays
or GPU tensors -- a test loop's table before ``bbox2result`` (``results.DeviceResults``); GPU tensors never visit the
host.  Then the two host ends move to the device too (csrc/map_flat.hip): ``yv4_map_rank`` orders the table, and after
the same overlaps and tpfp calls ``yv4_map_accumulate`` forms recall / precision / AP; ``MapGt`` keeps the ground-truth
tables of a dataset between calls.  Definition, where it is more than the list path's:

* A detection's problem is ``label * N + img_index``; one with a label outside ``[0, C)`` or an image index outside
  ``[0, N)`` takes no part.
* Ties -- the stated difference from the list path.  The visiting order inside a problem and the per-class order are
  descending score, STABLE: equal scores (``+0`` and ``-0`` are equal) keep the order of the flat table.  The list path
  orders them as the host's ``np.argsort`` happens to.  The two paths agree whenever no two detections of a class share
  a score; scores are expected finite.
* Accumulation per (class, threshold, area range): integer cumulative tp / fp (the float32 sums of the list path are
  exact below 2**24 detections per class; more raises here too), ``recall = float32(ctp) / max(num_gts, float32 eps)`` in
  float64, ``precision = float32(ctp) / max(float32(ctp + cfp), float32 eps)`` in float32, and ``average_precision`` on
  those dtypes.  ``'area'`` sums ``(mrec[i+1] - mrec[i]) * mpre[i+1]`` over the positions where recall changes into ONE
  float64 accumulator in rank order (``np.cumsum(terms)[-1]``; ``np.sum`` adds pairwise, which can differ in the last
  bit of the float64 sum before it is rounded to float32); ``'11points'`` is eleven float32 adds and one division.
* By default ``eval_results[c]['recall']`` / ``['precision']`` hold the curve's last point only (all that the summary
  table and ``evaluate_map`` read); ``curves=True`` downloads the full arrays.
* A foreign ``tpfp_fn`` has no device form: with flat input it raises.

``eval_recalls`` (``recall.py``) lives in ``recall_eval.py``; ``evaluate_map(metric='recall')`` keeps refusing the name
(``CustomBBoxDataset.eval_recalls`` is the way in).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _eval_common, _lib
from ._eval_common import PhaseTimer, _dev, _flat_to_device, _is_flat, _log, _offsets, _ptr, rank_flat
from ._lib import check
from .eval_utils import average_precision
from .ops import stream_ptr

_F32_EPS = np.finfo(np.float32).eps


def _device():
    return _eval_common._device('map_eval', 'map_eval')


def _boxes(a, cols=4):
    a = np.asarray(a, dtype=np.float32)
    return a.reshape(-1, cols) if a.size == 0 else a


def _areas(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _area_table(area_ranges):
    """None or [(None, None)] -> None ("no range"); else the (K, 2) float32 bounds, rounded once."""
    if area_ranges is None or all(lo is None for lo, _ in area_ranges):
        return None
    if any(lo is None or hi is None for lo, hi in area_ranges):
        raise ValueError('area_ranges mixes (None, None) with bounded ranges')
    return np.array([[lo, hi] for lo, hi in area_ranges], dtype=np.float32).reshape(-1, 2)


# ---- device calls ---------------------------------------------------------------------------------------------------
def bbox_overlaps_batched(boxes1, boxes2, off1, off2, mode='iou', eps=1e-6, dev_tables=None):
    """Overlap blocks of P problems.  boxes1 (N1, 4) / boxes2 (N2, 4) float32 torch tensors on the GPU, off1 / off2
    (P+1,) int64 numpy; ``dev_tables``: the device copies of off1, off2 and the pair offsets where the caller has them.
    Returns (flat float32 device tensor, iou_off numpy)."""
    assert mode in ('iou', 'iof')
    iou_off = _offsets(np.diff(off1) * np.diff(off2))
    dev = boxes1.device
    iou = torch.empty(int(iou_off[-1]), dtype=torch.float32, device=dev)
    if iou.numel():
        t_1, t_2, t_io = dev_tables or (_dev(o, np.int64, dev) for o in (off1, off2, iou_off))
        check(_lib.lib().yv4_bbox_overlaps_batched(
            boxes1.data_ptr(), boxes2.data_ptr(), t_1.data_ptr(), t_2.data_ptr(), t_io.data_ptr(), len(off1) - 1,
            int(iou_off[-1]), _lib.OVERLAPS_IOF if mode == 'iof' else _lib.OVERLAPS_IOU, float(np.float32(eps)),
            iou.data_ptr(), stream_ptr()), 'yv4_bbox_overlaps_batched')
    return iou, iou_off


def _gt_tables(annotations, C):
    """(gt (G, 4) float32, gt_ignore (G,) uint8, ng (C * N,) int64): every image's regular and ignored gts keyed by
    problem, then one stable sort (regular before ignored, each in the annotation's order)."""
    N = len(annotations)
    boxes, key, ign = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, bool)]
    for i, a in enumerate(annotations):
        parts = [(a['bboxes'], a['labels'], False)]
        if a.get('labels_ignore', None) is not None:
            parts.append((a['bboxes_ignore'], a['labels_ignore'], True))
        for b, lab, flag in parts:
            lab = np.asarray(lab).reshape(-1)
            if len(lab):
                boxes.append(_boxes(b)[:, :4])
                key.append(lab.astype(np.int64) * N + i)
                ign.append(np.full(len(lab), flag))
    boxes, key, ign = np.concatenate(boxes), np.concatenate(key), np.concatenate(ign)
    keep = (key >= 0) & (key < C * N)                        # labels outside [0, C) belong to no problem
    boxes, key, ign = boxes[keep], key[keep], ign[keep]
    by = np.lexsort((ign, key))                              # stable: ties keep the gathering order
    return (np.ascontiguousarray(boxes[by], dtype=np.float32).reshape(-1, 4), ign[by].astype(np.uint8),
            np.bincount(key, minlength=C * N).astype(np.int64))


class MapTables:
    """The (image, class) problems of a dataset as flat host tables, class-major: problem ``c * num_imgs + i``.

    det (D, 5) float32 in the given order; gt (G, 4): per problem the class's gts followed by its ignored gts, with
    ``gt_ignore`` bytes; nd / ng per problem.  ``sort()`` adds the visiting order and its inverse per problem
    (``np.argsort(-scores)``), and the per-class global order."""

    def __init__(self, det_results, annotations):
        assert len(det_results) == len(annotations)
        self.num_imgs = N = len(det_results)
        self.num_classes = C = len(det_results[0])
        # detections: one concatenation in class-major order
        dets = [det_results[i][c] for c in range(C) for i in range(N)]
        self.nd = nd = np.fromiter((len(d) for d in dets), np.int64, C * N)
        dets = [d for d in dets if len(d)]
        self.det = (np.concatenate(dets).astype(np.float32, copy=False).reshape(-1, 5) if dets
                    else np.zeros((0, 5), np.float32))
        self.gt, self.gt_ignore, self.ng = _gt_tables(annotations, C)
        self.det_off, self.gt_off = _offsets(nd), _offsets(self.ng)
        self.order = self.rank = self.cls_order = None

    def class_slice(self, c):
        return slice(int(self.det_off[c * self.num_imgs]), int(self.det_off[(c + 1) * self.num_imgs]))

    def sort(self):
        neg = -self.det[:, 4]
        order = np.empty(len(neg), np.int32)
        off = self.det_off
        for p in np.flatnonzero(self.nd):
            lo, hi = off[p], off[p + 1]
            order[lo:hi] = np.argsort(neg[lo:hi]) if hi - lo > 1 else 0
        rank = np.empty_like(order)
        base = np.repeat(off[:-1], self.nd)
        rank[base + order] = np.arange(len(neg), dtype=np.int64) - base
        self.order, self.rank = order, rank
        self.cls_order = [np.argsort(neg[self.class_slice(c)]) for c in range(self.num_classes)]
        return self


def tpfp_batched(tab, mode, iou_thrs, area_ranges=None, phases=None):
    """tp / fp of every detection of ``tab`` (a sorted MapTables) for every threshold and area range: upload, one
    overlaps call, one tpfp call, download.  Returns two (T, K, D) uint8 numpy arrays, columns in ``tab.det`` order.
    ``phases``: an optional dict that receives upload / launch / download seconds (each closed by a synchronise)."""
    dev = _device()
    thrs = np.ascontiguousarray(iou_thrs, dtype=np.float32).reshape(-1)
    area = _area_table(area_ranges)
    T, K = len(thrs), 1 if area is None else len(area)
    D, G = len(tab.det), len(tab.gt)
    imagenet = mode == _lib.TPFP_IMAGENET
    if D == 0:
        return np.zeros((T, K, 0), np.uint8), np.zeros((T, K, 0), np.uint8)
    timer = PhaseTimer(phases, dev)
    det4 = _dev(tab.det[:, :4], np.float32, dev)
    gt = _dev(tab.gt, np.float32, dev)
    ign = _dev(tab.gt_ignore, np.uint8, dev)
    gt_iou, ratio = gt, None
    if imagenet:
        gt_iou = _dev(tab.gt - np.float32(1), np.float32, dev)
        w, h = tab.gt[:, 2] - tab.gt[:, 0], tab.gt[:, 3] - tab.gt[:, 1]
        with np.errstate(all='ignore'):
            ratio = _dev((w * h) / ((w + 10.0) * (h + 10.0)), np.float32, dev)
    order = _dev(tab.order, np.int32, dev) if imagenet else None
    rank = None if imagenet else _dev(tab.rank, np.int32, dev)
    t_do, t_go = _dev(tab.det_off, np.int64, dev), _dev(tab.gt_off, np.int64, dev)
    t_io = _dev(_offsets(tab.nd * tab.ng), np.int64, dev)
    t_thr = _dev(thrs, np.float32, dev)
    t_area = None if area is None else _dev(area, np.float32, dev)
    timer.mark('upload')
    lib = _lib.lib()
    iou, _ = bbox_overlaps_batched(det4, gt_iou, tab.det_off, tab.gt_off, dev_tables=(t_do, t_go, t_io))
    if iou.numel() == 0:                                   # no problem has both detections and gts
        iou = torch.zeros(1, dtype=torch.float32, device=dev)
    work = torch.empty(max(int(lib.yv4_tpfp_work(mode, D, G, T)), 4), dtype=torch.uint8, device=dev)
    tp = torch.empty((T, K, D), dtype=torch.uint8, device=dev)
    fp = torch.empty((T, K, D), dtype=torch.uint8, device=dev)
    check(lib.yv4_tpfp_batched(mode, _ptr(det4), _ptr(gt), _ptr(ign), _ptr(ratio), _ptr(order), _ptr(rank), t_do.data_ptr(),
                               t_go.data_ptr(), t_io.data_ptr(), len(tab.nd), D, G, _ptr(iou), t_thr.data_ptr(), T,
                               _ptr(t_area), K, work.data_ptr(), tp.data_ptr(), fp.data_ptr(), stream_ptr()),
          'yv4_tpfp_batched')
    timer.mark('launch')
    tp, fp = tp.cpu().numpy(), fp.cpu().numpy()
    timer.mark('download')
    return tp, fp


# ---- the reference's one-problem ops ----------------------------------------------------------------------------------
def bbox_overlaps(bboxes1, bboxes2, mode='iou', eps=1e-6):
    """bbox_overlaps.py:4: (n, 4+), (k, 4+) -> (n, k) float32; 'iof' divides by the area of bboxes1's box.  The
    reference swaps its operands when n > k and transposes back, which changes no bit (one commutative add)."""
    assert mode in ['iou', 'iof']
    dev = _device()
    b1, b2 = _boxes(bboxes1)[:, :4], _boxes(bboxes2)[:, :4]
    n, k = len(b1), len(b2)
    if n * k == 0:
        return np.zeros((n, k), np.float32)
    iou, _ = bbox_overlaps_batched(_dev(b1, np.float32, dev), _dev(b2, np.float32, dev), np.array([0, n]),
                                      np.array([0, k]), mode, eps)
    return iou.view(n, k).cpu().numpy()


def _tpfp_single(mode, det_bboxes, gt_bboxes, gt_bboxes_ignore, iou_thr, area_ranges):
    _device()
    det = _boxes(det_bboxes, 5)
    ann = dict(bboxes=_boxes(gt_bboxes), labels=np.zeros(len(gt_bboxes), np.int64))
    if gt_bboxes_ignore is not None:
        ann.update(bboxes_ignore=_boxes(gt_bboxes_ignore), labels_ignore=np.zeros(len(gt_bboxes_ignore), np.int64))
    tp, fp = tpfp_batched(MapTables([[det]], [ann]).sort(), mode, [iou_thr], area_ranges)
    return tp[0].astype(np.float32), fp[0].astype(np.float32)


def tpfp_default(det_bboxes, gt_bboxes, gt_bboxes_ignore=None, iou_thr=0.5, area_ranges=None):
    """mean_ap.py:153: (m, 5), (n, 4), (k, 4) -> (tp, fp), float32 (num_scales, m) of 0 / 1."""
    return _tpfp_single(_lib.TPFP_DEFAULT, det_bboxes, gt_bboxes, gt_bboxes_ignore, iou_thr, area_ranges)


def tpfp_imagenet(det_bboxes, gt_bboxes, gt_bboxes_ignore=None, default_iou_thr=0.5, area_ranges=None):
    """mean_ap.py:59: the ImageNet rule (per-gt thresholds, overlaps against gt - 1)."""
    return _tpfp_single(_lib.TPFP_IMAGENET, det_bboxes, gt_bboxes, gt_bboxes_ignore, default_iou_thr, area_ranges)


# ---- accumulation (host, numpy) -----------------------------------------------------------------------------------------
def _num_gts(tab, area):
    """(C, K) int: the class's regular gts per area range."""
    C, N = tab.num_classes, tab.num_imgs
    K = 1 if area is None else len(area)
    cls = np.repeat(np.arange(C * N) // N, tab.ng)[tab.gt_ignore == 0]
    ga = _areas(tab.gt[tab.gt_ignore == 0])
    out = np.zeros((C, K), dtype=int)
    for k in range(K):
        sel = cls if area is None else cls[(ga >= area[k, 0]) & (ga < area[k, 1])]
        out[:, k] = np.bincount(sel, minlength=C)
    return out


def _mean_ap(eval_results, scale_ranges):
    """mean_ap.py:385-396: the mean over the classes that have gts (per scale range)."""
    if scale_ranges is not None:
        all_ap = np.vstack([r['ap'] for r in eval_results])
        all_num_gts = np.vstack([r['num_gts'] for r in eval_results])
        mean_ap = []
        for k in range(all_ap.shape[1]):
            has = all_num_gts[:, k] > 0
            mean_ap.append(all_ap[has, k].mean() if np.any(has) else 0.0)
    else:
        aps = [r['ap'] for r in eval_results if r['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    return mean_ap


def accumulate(tab, tp, fp, num_gts, scale_ranges, dataset):
    """mean_ap.py:353-396 for one threshold: tp / fp (K, D) flags -> (mean_ap, eval_results)."""
    mode = 'area' if dataset != 'voc07' else '11points'
    eval_results = []
    for c in range(tab.num_classes):
        sl = tab.class_slice(c)
        num_dets = sl.stop - sl.start
        if num_dets >= 2 ** 24:
            raise ValueError(f'class {c} has {num_dets} detections: the float32 cumulative sums of the reference are '
                             'exact only below 2**24')
        sort_inds = tab.cls_order[c]
        ctp = np.cumsum(tp[:, sl].astype(np.float32)[:, sort_inds], axis=1)
        cfp = np.cumsum(fp[:, sl].astype(np.float32)[:, sort_inds], axis=1)
        n = num_gts[c].copy()
        recalls = ctp / np.maximum(n[:, np.newaxis], _F32_EPS)
        precisions = ctp / np.maximum((ctp + cfp), _F32_EPS)
        if scale_ranges is None:
            recalls, precisions, n = recalls[0, :], precisions[0, :], n.item()
        ap = average_precision(recalls, precisions, mode)
        eval_results.append({'num_gts': n, 'num_dets': num_dets, 'recall': recalls, 'precision': precisions, 'ap': ap})
    return _mean_ap(eval_results, scale_ranges), eval_results


def _custom_tpfp_all(tab, tpfp_fn, thrs, area_ranges, K):
    """Any other callable: called per (image, class) and threshold on the host, serially, as the reference's pool does."""
    T, D = len(thrs), len(tab.det)
    tp, fp = np.zeros((T, K, D), np.uint8), np.zeros((T, K, D), np.uint8)
    for p in range(len(tab.nd)):
        d = tab.det[tab.det_off[p]:tab.det_off[p + 1]]
        g = tab.gt[tab.gt_off[p]:tab.gt_off[p + 1]]
        ign = tab.gt_ignore[tab.gt_off[p]:tab.gt_off[p + 1]] != 0
        for t, thr in enumerate(thrs):
            a, b = tpfp_fn(d, g[~ign], g[ign], thr, area_ranges)
            tp[t, :, tab.det_off[p]:tab.det_off[p + 1]] = a
            fp[t, :, tab.det_off[p]:tab.det_off[p + 1]] = b
    return tp, fp


# ---- the flat form: ordering and accumulation on the device too (csrc/map_flat.hip) ------------------------------------
class MapGt:
    """The ground-truth side of ``MapTables``, built once per dataset: class-major gts (problem ``c * num_imgs + i``),
    a problem's ignored gts behind its regular ones, ``gt_off``.  The imagenet rule's ``gt - 1`` boxes and ratios are
    today's numpy expressions on the host; the device copies are cached per device; ``num_gts(area)`` is today's
    ``_num_gts`` arithmetic.  ``annotations``: what the dataset's ``get_ann_info`` returns per image."""

    def __init__(self, annotations, num_classes):
        self.annotations = annotations
        self.num_imgs, self.num_classes = len(annotations), int(num_classes)
        if self.num_imgs <= 0 or self.num_classes <= 0:
            raise ValueError('MapGt needs at least one image and one class')
        if self.num_imgs * self.num_classes >= 2 ** 31 - 1:
            raise ValueError(f'{self.num_imgs} images x {self.num_classes} classes: the problem index does not fit 31 bits')
        self.gt, self.gt_ignore, self.ng = _gt_tables(annotations, self.num_classes)
        self.gt_off = _offsets(self.ng)
        self._host_imagenet = None
        self._num_gts = {}
        self._device = {}

    def imagenet_tables(self):
        """(gt - 1, w*h / ((w+10)*(h+10))) as ``tpfp_batched`` forms them."""
        if self._host_imagenet is None:
            w, h = self.gt[:, 2] - self.gt[:, 0], self.gt[:, 3] - self.gt[:, 1]
            with np.errstate(all='ignore'):
                self._host_imagenet = (self.gt - np.float32(1), (w * h) / ((w + 10.0) * (h + 10.0)))
        return self._host_imagenet

    def device(self, dev, imagenet=False):
        """The device copies: gt, ign, gt_off, and gt_m1 / ratio once the imagenet rule asked for them."""
        d = self._device.setdefault((dev.type, dev.index), {})
        if 'gt' not in d:
            d.update(gt=_dev(self.gt, np.float32, dev), ign=_dev(self.gt_ignore, np.uint8, dev),
                     gt_off=_dev(self.gt_off, np.int64, dev))
        if imagenet and 'gt_m1' not in d:
            gt_m1, ratio = self.imagenet_tables()
            d.update(gt_m1=_dev(gt_m1, np.float32, dev), ratio=_dev(ratio, np.float32, dev))
        return d

    def num_gts(self, area):
        """(C, K) per area table, kept: the tables do not change."""
        key = None if area is None else area.tobytes()
        if key not in self._num_gts:
            self._num_gts[key] = _num_gts(self, area)
        return self._num_gts[key]


def _device_flat():
    _device()
    return _eval_common._device('map_eval', 'map_flat')


def map_flat_device(flat, gt, mode, iou_thrs, area_ranges=None, ap_mode='area', curves=False, phases=None):
    """The whole flat pipeline for every threshold and area range: ``yv4_map_rank``, one read-back (the pair total and
    the class counts), ``yv4_bbox_overlaps_batched``, ``yv4_tpfp_batched``, ``yv4_map_accumulate``, one download.
    ``flat``: ``(dets (D, 5), labels (D,), img_index (D,))``, numpy arrays or GPU tensors (those never visit the host);
    ``gt``: a ``MapGt``.  Returns host arrays: ap (T, C, K) float32, last_recall float64 / last_precision float32
    (T, C, K), num_dets (C,), num_gts (C, K) and, with ``curves``, recall float64 / precision float32 (T, K, Dv) whose
    columns ``[cls_off[c], cls_off[c + 1])`` are class c's curve.  ``phases``: an optional dict that receives seconds
    per phase (each closed by a synchronise)."""
    dev = _device_flat()
    timer = PhaseTimer(phases, dev)
    thrs = np.ascontiguousarray(iou_thrs, dtype=np.float32).reshape(-1)
    area = _area_table(area_ranges)
    T, K = len(thrs), 1 if area is None else len(area)
    N, C = gt.num_imgs, gt.num_classes
    P, G = N * C, len(gt.gt)
    imagenet = mode == _lib.TPFP_IMAGENET
    g = gt.device(dev, imagenet)
    num_gts = gt.num_gts(area)
    flat = _flat_to_device(flat, dev)
    t_thr = _dev(thrs, np.float32, dev)
    t_area = None if area is None else _dev(area, np.float32, dev)
    t_ngts = _dev(num_gts, np.int64, dev)
    timer.mark('upload')
    lib = _lib.lib()
    det4, det_off, iou_off, order, rank, cls_order, pairs, Dv, counts = rank_flat(flat, g['gt_off'], N, C, dev)
    timer.mark('rank')
    iou = torch.empty(max(pairs, 1), dtype=torch.float32, device=dev)
    if pairs:
        check(lib.yv4_bbox_overlaps_batched(det4.data_ptr(), (g['gt_m1'] if imagenet else g['gt']).data_ptr(),
                                            det_off.data_ptr(), g['gt_off'].data_ptr(), iou_off.data_ptr(), P, pairs,
                                            _lib.OVERLAPS_IOU, float(np.float32(1e-6)), iou.data_ptr(), stream_ptr()),
              'yv4_bbox_overlaps_batched')
    else:
        iou.zero_()
    tp = torch.empty((T, K, Dv), dtype=torch.uint8, device=dev)
    fp = torch.empty((T, K, Dv), dtype=torch.uint8, device=dev)
    if Dv:
        work = torch.empty(max(int(lib.yv4_tpfp_work(mode, Dv, G, T)), 4), dtype=torch.uint8, device=dev)
        check(lib.yv4_tpfp_batched(mode, det4.data_ptr(), _ptr(g['gt']), _ptr(g['ign']), _ptr(g.get('ratio')),
                                   order.data_ptr() if imagenet else None, None if imagenet else rank.data_ptr(),
                                   det_off.data_ptr(), g['gt_off'].data_ptr(), iou_off.data_ptr(), P, Dv, G, iou.data_ptr(),
                                   t_thr.data_ptr(), T, _ptr(t_area), K, work.data_ptr(), tp.data_ptr(), fp.data_ptr(),
                                   stream_ptr()), 'yv4_tpfp_batched')
    timer.mark('tpfp')
    ap = torch.empty((T, C, K), dtype=torch.float32, device=dev)
    last_r = torch.empty((T, C, K), dtype=torch.float64, device=dev)
    last_p = torch.empty((T, C, K), dtype=torch.float32, device=dev)
    num_dets = torch.empty(C, dtype=torch.int64, device=dev)
    rec = torch.empty((T, K, Dv), dtype=torch.float64, device=dev) if curves else None
    prec = torch.empty((T, K, Dv), dtype=torch.float32, device=dev) if curves else None
    work = torch.empty(max(int(lib.yv4_map_accumulate_work(Dv, T, K)), 4), dtype=torch.uint8, device=dev)
    check(lib.yv4_map_accumulate(_ptr(tp), _ptr(fp), cls_order.data_ptr(), det_off.data_ptr(), t_ngts.data_ptr(), Dv, N, C, T,
                                 K, _lib.MAP_AP_11POINTS if ap_mode == '11points' else _lib.MAP_AP_AREA, work.data_ptr(),
                                 ap.data_ptr(), last_r.data_ptr(), last_p.data_ptr(), _ptr(rec), _ptr(prec),
                                 num_dets.data_ptr(), stream_ptr()), 'yv4_map_accumulate')
    timer.mark('accumulate')
    out = dict(ap=ap.cpu().numpy(), last_recall=last_r.cpu().numpy(), last_precision=last_p.cpu().numpy(),
               num_dets=num_dets.cpu().numpy(), num_gts=num_gts, cls_off=_offsets(counts), total_det=Dv, pairs=pairs)
    if curves:
        out.update(recall=rec.cpu().numpy(), precision=prec.cpu().numpy())
    timer.mark('download')
    return out


def _flat_eval_results(out, t, scale_ranges, curves):
    """One threshold of ``map_flat_device`` in ``accumulate``'s structure.  Without ``curves`` recall / precision hold
    the curve's last point only (nothing for a class without detections)."""
    eval_results = []
    for c in range(out['ap'].shape[1]):
        n = out['num_gts'][c].copy()
        num_dets = int(out['num_dets'][c])
        if curves:
            sl = slice(int(out['cls_off'][c]), int(out['cls_off'][c + 1]))
            recalls, precisions = out['recall'][t][:, sl].copy(), out['precision'][t][:, sl].copy()
        else:
            recalls = out['last_recall'][t, c][:, np.newaxis][:, :min(num_dets, 1)].copy()
            precisions = out['last_precision'][t, c][:, np.newaxis][:, :min(num_dets, 1)].copy()
        ap = out['ap'][t, c].copy()
        if scale_ranges is None:
            recalls, precisions, n, ap = recalls[0, :], precisions[0, :], n.item(), ap[0]
        eval_results.append({'num_gts': n, 'num_dets': num_dets, 'recall': recalls, 'precision': precisions, 'ap': ap})
    return _mean_ap(eval_results, scale_ranges), eval_results


def _as_map_gt(annotations, dataset, num_classes):
    if isinstance(annotations, MapGt):
        return annotations
    if num_classes is None and isinstance(dataset, (list, tuple)):
        num_classes = len(dataset)
    if num_classes is None:
        raise ValueError('flat results carry no class count: pass a MapGt, num_classes, or the class names as dataset')
    return MapGt(annotations, num_classes)


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None, logger=None, tpfp_fn=None, nproc=4,
             curves=False, num_classes=None):
    """mean_ap.py:267: ``(mean_ap, eval_results)``; ``eval_results[c]`` holds num_gts / num_dets / recall / precision /
    ap of class c.  ``iou_thr`` may also be a list or tuple: the batched entry, which returns one ``(mean_ap,
    eval_results)`` per threshold from one overlaps call and one tpfp call over the whole dataset.  ``nproc`` is
    accepted and unused.  ``tpfp_fn=None`` selects the ImageNet rule for ``dataset in ('det', 'vid')`` and the default
    rule otherwise; this module's ``tpfp_default`` / ``tpfp_imagenet`` select their rule; any other callable is called
    per (image, class) on the host.

    ``det_results`` may also be the flat form ``(dets (D, 5), labels (D,), img_index (D,))`` of numpy arrays or GPU
    tensors (see the module docstring): ordering and accumulation then run on the device as well.  ``annotations`` may
    be a ``MapGt`` (with per-image lists, ``num_classes`` or the class names as ``dataset`` give the class count);
    ``curves=True`` downloads the full recall / precision arrays instead of their last points; only the two rules of
    this module are available."""
    flat = _is_flat(det_results)
    if not flat:
        if isinstance(annotations, MapGt):
            annotations = annotations.annotations
        assert len(det_results) == len(annotations)
    many = isinstance(iou_thr, (list, tuple, np.ndarray))
    thrs = list(iou_thr) if many else [iou_thr]
    area_ranges = [(rg[0] ** 2, rg[1] ** 2) for rg in scale_ranges] if scale_ranges is not None else None
    if tpfp_fn is None:
        tpfp_fn = tpfp_imagenet if dataset in ['det', 'vid'] else tpfp_default
    if not callable(tpfp_fn):
        raise ValueError(f'tpfp_fn has to be a function or None, but got {tpfp_fn}')
    if flat:
        if tpfp_fn is not tpfp_default and tpfp_fn is not tpfp_imagenet:
            raise ValueError('flat results are scored on the device, which knows tpfp_default and tpfp_imagenet only; '
                             f'for {tpfp_fn!r} pass the per-image lists')
        out = map_flat_device(det_results, _as_map_gt(annotations, dataset, num_classes),
                              _lib.TPFP_IMAGENET if tpfp_fn is tpfp_imagenet else _lib.TPFP_DEFAULT, thrs, area_ranges,
                              '11points' if dataset == 'voc07' else 'area', curves)
        res = []
        for t, thr in enumerate(thrs):
            mean_ap, eval_results = _flat_eval_results(out, t, scale_ranges, curves)
            if many and logger != 'silent':
                _log(f'\n{"-" * 15}iou_thr: {thr}{"-" * 15}', logger)
            print_map_summary(mean_ap, eval_results, dataset, area_ranges, logger=logger)
            res.append((mean_ap, eval_results))
        return res if many else res[0]
    area = _area_table(area_ranges)
    K = 1 if area is None else len(area)
    if tpfp_fn is tpfp_default or tpfp_fn is tpfp_imagenet:
        _device()
        tab = MapTables(det_results, annotations).sort()
        tp, fp = tpfp_batched(tab, _lib.TPFP_IMAGENET if tpfp_fn is tpfp_imagenet else _lib.TPFP_DEFAULT, thrs, area_ranges)
    else:
        tab = MapTables(det_results, annotations).sort()
        tp, fp = _custom_tpfp_all(tab, tpfp_fn, thrs, area_ranges, K)
    num_gts = _num_gts(tab, area)
    out = []
    for t, thr in enumerate(thrs):
        mean_ap, eval_results = accumulate(tab, tp[t], fp[t], num_gts, scale_ranges, dataset)
        if many and logger != 'silent':
            _log(f'\n{"-" * 15}iou_thr: {thr}{"-" * 15}', logger)
        print_map_summary(mean_ap, eval_results, dataset, area_ranges, logger=logger)
        out.append((mean_ap, eval_results))
    return out if many else out[0]


def evaluate_map(results, annotations, classes=None, iou_thr=0.5, scale_ranges=None, logger=None, metric='mAP',
                 num_classes=None):
    """``dataset.evaluate(results, metric='mAP')`` (datasets/custom.py:309-325): ``AP50``-style keys (rounded to three
    places) plus ``mAP``, their mean, from ONE device pass over all thresholds.  ``annotations``: what the dataset's
    ``get_ann_info`` returns per image, or a ``MapGt``.  ``results``: the per-image lists or the flat tuple."""
    if not isinstance(metric, str):
        assert len(metric) == 1
        metric = metric[0]
    if metric == 'recall':
        raise NotImplementedError("metric='recall' (eval_recalls) is not built: it scores RPN proposals, which no "
                                  'detector of this package produces')
    if metric != 'mAP':
        raise KeyError(f'metric {metric} is not supported')
    iou_thrs = [iou_thr] if isinstance(iou_thr, float) else iou_thr
    assert isinstance(iou_thrs, list)
    eval_results = OrderedDict()
    mean_aps = []
    for thr, (mean_ap, _) in zip(iou_thrs, eval_map(results, annotations, scale_ranges=scale_ranges, iou_thr=iou_thrs,
                                                    dataset=classes, logger=logger, num_classes=num_classes)):
        mean_aps.append(mean_ap)
        eval_results[f'AP{int(thr * 100):02d}'] = round(mean_ap, 3)
    eval_results['mAP'] = sum(mean_aps) / len(mean_aps)
    return eval_results


# ---- the summary table (the project's own text; terminaltables is not used and no parity is claimed) -----------------
def print_map_summary(mean_ap, results, dataset=None, scale_ranges=None, logger=None):
    """gts / dets / recall / ap per class and the mAP, one plain-text table per scale range.  ``dataset``: a list of
    class names (a dataset NAME such as 'voc07' only selects a metric variant here; classes are then numbered)."""
    if logger == 'silent':
        return
    num_scales = len(results[0]['ap']) if isinstance(results[0]['ap'], np.ndarray) else 1
    if scale_ranges is not None:
        assert len(scale_ranges) == num_scales
    names = [str(i) for i in range(len(results))] if dataset is None or isinstance(dataset, str) else list(dataset)
    mean_ap = mean_ap if isinstance(mean_ap, list) else [mean_ap]
    for k in range(num_scales):
        rows = [('class', 'gts', 'dets', 'recall', 'ap')]
        for name, r in zip(names, results):
            rec = np.array(r['recall'], ndmin=2)
            rows.append((str(name), str(np.array(r['num_gts'], ndmin=1)[k]), str(r['num_dets']),
                         f'{rec[k, -1] if rec.shape[1] else 0.0:.3f}', f'{np.array(r["ap"], ndmin=1)[k]:.3f}'))
        rows.append(('mAP', '', '', '', f'{mean_ap[k]:.3f}'))
        width = [max(len(r[j]) for r in rows) for j in range(5)]
        rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
        lines = [rule]
        for n, r in enumerate(rows):
            lines.append('| ' + ' | '.join(c.ljust(w) for c, w in zip(r, width)) + ' |')
            if n == 0 or n == len(rows) - 2:
                lines.append(rule)
        lines.append(rule)
        head = f'Scale range {scale_ranges[k]}\n' if scale_ranges is not None else ''
        _log('\n' + head + '\n'.join(lines), logger)
