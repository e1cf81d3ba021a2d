"""Detection evaluation: ``iou_coco`` / ``match_coco`` and ``eval_map_flexible`` under the reference's names.

Mirror of ``mmdet/ops/eval_utils/iou/iou_coco.pyx:58`` and ``match/match_coco.pyx:59`` (numpy in, numpy
out, one problem per call) and of ``mmdet/core/evaluation/mean_ap_flexible.py`` (registries
``EVAL_BREAKDOWN`` / ``EVAL_IOU_CALCULATOR`` / ``EVAL_MATCHER``, ``IOU2DCoCo``, ``MatcherCoCo``,
``ScaleBreakdown``, ``FlexibleStatisticsEval``, ``eval_map_flexible``; selected by
``metric='fast-bbox'`` in ``datasets/coco.py:464-496``).

Where the reference walks the (image, class) problems one by one (optionally over a process pool) and
calls the two Cython ops per problem, ``FlexibleStatisticsEval.statistics_eval`` here gathers every
problem of the dataset into one table and evaluates it with ONE ``yv4_iou_coco_batched`` launch and ONE
``yv4_match_coco_batched`` launch (all breakdowns and thresholds in parallel).  Sorting by score keeps
numpy's ``argsort()[::-1]`` on the host so that exact score ties order as in the reference.  There is no
CPU implementation of the two ops in this package.

The flat path.  ``statistics_eval`` / ``eval_map_flexible`` / ``evaluate_fast_bbox`` also take the flat table of a test
loop in place of the per-image lists, and a ``FlexGt`` in place of ``annotations``; the whole evaluation then runs on the
device (``flex_flat_device``; csrc/flex_eval.hip with csrc/map_flat.hip's ``yv4_map_rank`` and the two batched ops
above).  Its definition (stated in include/yv4.h, restated here):

* Input: ``dets (D, 5) float32``, ``labels (D,) int64``, ``img_index (D,) int64``, numpy arrays or GPU tensors; the
  ground truth as a ``FlexGt``.
* Problems: N images x C classes give P = C * N problems, class-major (``p = c * N + i``), exactly as in ``map_flat``.
  B breakdown rows: row 0 is ``'All'``, then one per ``ScaleBreakdown`` range.  Matching problem ``q = p * B + b`` shares
  problem p's IoU block.
* Order: ``yv4_map_rank``'s two stable orders.  Score ties keep the table's order -- the one stated difference from the
  list path, whose ties follow ``argsort()[::-1]``.
* Per class c, breakdown b, threshold t, over the class's detections in ``cls_order`` (a detection sits in problem p at
  local position d): ``mg_own = matched[q(p, b)][t][d]``, ``mg_last = matched[q(p, B-1)][t][d]``,
  ``tp = (mg_last if shared_tp else mg_own) > -1``; ``in = gt_bkd[b][gt_off[p] + mg_own]`` when ``mg_own > -1``, else the
  detection's own breakdown flag (row 0 always true, row b >= 1 is ``lo <= area < hi`` with
  ``area = (x2-x1)*(y2-y1)``, each float32 operation rounded on its own, the bounds rounded to float32 once on the
  host).  A problem with no ground truth matches nothing (the list path's ``ious is None`` branch).
* With ``k`` the running count of ``in`` and ``ctp`` the running count of ``in & tp`` (integers):
  ``precision = double(ctp) / double(k)``, ``recall = double(ctp) / double(num_gt)`` (``/ 1e-7`` when ``num_gt == 0``).
  The AP is taken over the compacted list (the ``in`` positions only): precision's suffix maximum, the sum of
  ``(recall_m - recall_prev) * envelope_m`` over the positions where recall changes (``recall_prev`` starts at 0), added
  in rank order into a single float64 accumulator, then rounded to float32.  (``np.sum`` adds pairwise: the definition's
  one freedom.)
* Outputs, each ``(C, B, T)``: ``num_det`` int64, the last recall float64 (0 when ``num_det == 0``), ``mAP`` float32.
  No float atomics: two runs give identical bytes.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _eval_common, _lib
from ._eval_common import PhaseTimer, _dev, _flat_to_device, _is_flat, _offsets, rank_flat
from ._lib import check
from .ops import stream_ptr
from .registry import Registry, build_from_cfg

EVAL_BREAKDOWN = Registry('Evaluation Breakdown')
EVAL_IOU_CALCULATOR = Registry('Evaluation IOU calculator')
EVAL_MATCHER = Registry('Evaluation Matcher')


def _device():
    return _eval_common._device('eval_utils')


def iou_coco_batched(det, gt, is_crowd, det_off, gt_off):
    """IoU blocks of P problems.  det (D,4) / gt (G,4) float32 and is_crowd (G,) bool torch tensors on the
    GPU, det_off / gt_off (P+1,) int64 numpy.  Returns (iou flat float32 device tensor, iou_off numpy)."""
    nd, ng = np.diff(det_off), np.diff(gt_off)
    iou_off = _offsets(nd * ng)
    dev = det.device
    iou = torch.empty(int(iou_off[-1]), dtype=torch.float32, device=dev)
    if iou.numel():
        t_do, t_go, t_io = (_dev(o, np.int64, dev) for o in (det_off, gt_off, iou_off))
        crowd = is_crowd.to(torch.uint8)
        check(_lib.lib().yv4_iou_coco_batched(det.data_ptr(), gt.data_ptr(), crowd.data_ptr(), t_do.data_ptr(),
                                              t_go.data_ptr(), t_io.data_ptr(), len(nd), int(iou_off[-1]),
                                              iou.data_ptr(), stream_ptr()), 'yv4_iou_coco_batched')
    return iou, iou_off


def match_coco_batched(iou, det_off, gt_off, iou_off, iou_thrs, is_ignore, is_crowd):
    """Greedy COCO matching of Q problems over one flat IoU buffer.  det_off / gt_off are (Q+1,) int64
    cumulative tables (they place each problem's output and its is_ignore / is_crowd slice), iou_off (Q,)
    the start of each problem's IoU block (blocks may be shared between problems).  Returns the flat int32
    device tensor ``matched``: problem q's (num_thrs, num_det) block starts at det_off[q] * num_thrs."""
    dev = iou.device
    Q = len(det_off) - 1
    nt = len(iou_thrs)
    matched = torch.empty(int(det_off[-1]) * nt, dtype=torch.int32, device=dev)
    if Q == 0 or matched.numel() == 0:
        return matched
    work = torch.empty(max(int(gt_off[-1]) * nt, 1), dtype=torch.uint8, device=dev)
    t_do, t_go = _dev(det_off, np.int64, dev), _dev(gt_off, np.int64, dev)
    t_io = _dev(np.append(iou_off[:Q], 0), np.int64, dev)
    thr = _dev(iou_thrs, np.float32, dev)
    ign, crowd = is_ignore.to(torch.uint8), is_crowd.to(torch.uint8)
    if ign.numel() == 0:                                   # every problem has zero gts
        ign = crowd = torch.zeros(1, dtype=torch.uint8, device=dev)
    check(_lib.lib().yv4_match_coco_batched(iou.data_ptr(), t_do.data_ptr(), t_go.data_ptr(), t_io.data_ptr(),
                                            thr.data_ptr(), nt, ign.data_ptr(), crowd.data_ptr(), Q,
                                            work.data_ptr(), matched.data_ptr(), stream_ptr()),
          'yv4_match_coco_batched')
    return matched


def iou_coco(det_boxes, gt_boxes, is_crowd):
    """iou_coco.pyx:58: (num_det, 4), (num_gt, 4) float32 and (num_gt,) bool -> (num_det, num_gt) float32."""
    det_boxes, gt_boxes = np.asarray(det_boxes), np.asarray(gt_boxes)
    if det_boxes.dtype != np.float32 or gt_boxes.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'npy_float32'")      # the Cython signature's check
    if det_boxes.ndim != 2 or gt_boxes.ndim != 2:
        raise ValueError('Buffer has wrong number of dimensions (expected 2)')
    nd, ng = det_boxes.shape[0], gt_boxes.shape[0]
    if nd == 0 or ng == 0:
        return np.zeros((nd, ng), np.float32)
    dev = _device()
    iou, _ = iou_coco_batched(_dev(det_boxes[:, :4], np.float32, dev), _dev(gt_boxes[:, :4], np.float32, dev),
                              _dev(is_crowd, np.bool_, dev), np.array([0, nd]), np.array([0, ng]))
    return iou.view(nd, ng).cpu().numpy()


def match_coco(iou_mat, iou_thrs, is_ignore, is_crowd):
    """match_coco.pyx:59: (num_det, num_gt) float32 IoU, (num_thrs,) float32, two (num_gt,) bool ->
    (num_thrs, num_det) int32 index of the matched gt or -1."""
    iou_mat, iou_thrs = np.asarray(iou_mat), np.asarray(iou_thrs)
    if iou_mat.dtype != np.float32 or iou_thrs.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'npy_float32'")
    nd, ng = iou_mat.shape
    nt = iou_thrs.shape[0]
    if nd == 0 or nt == 0:
        return np.empty((nt, nd), np.int32)
    dev = _device()
    out = match_coco_batched(_dev(iou_mat, np.float32, dev), np.array([0, nd]), np.array([0, ng]), np.array([0]),
                             iou_thrs, _dev(is_ignore, np.bool_, dev), _dev(is_crowd, np.bool_, dev))
    return out.view(nt, nd).cpu().numpy()


def average_precision(recalls, precisions, mode='area'):
    """mean_ap.py:12-58: area under the monotone precision envelope ('area') or the 11-point average."""
    recalls, precisions = np.asarray(recalls), np.asarray(precisions)
    single = recalls.ndim == 1
    if single:
        recalls, precisions = recalls[None], precisions[None]
    assert recalls.shape == precisions.shape and recalls.ndim == 2
    ap = np.zeros(recalls.shape[0], np.float32)
    for i, (r, p) in enumerate(zip(recalls, precisions)):
        if mode == 'area':
            mrec = np.concatenate(([0], r, [1])).astype(recalls.dtype)
            mpre = np.concatenate(([0], p, [0])).astype(recalls.dtype)
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            step = np.nonzero(mrec[1:] != mrec[:-1])[0]
            ap[i] = np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1])
        elif mode == '11points':
            for thr in np.arange(0, 1 + 1e-3, 0.1):
                sel = p[r >= thr]
                ap[i] += sel.max() if sel.size else 0
            ap[i] /= 11
        else:
            raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap[0] if single else ap


@EVAL_IOU_CALCULATOR.register_module()
class IOU2DCoCo:
    """mean_ap_flexible.py:19-25."""

    def __call__(self, det_bboxes, gt_bboxes, gt_iscrowd=None):
        if gt_iscrowd is None:
            gt_iscrowd = np.zeros(gt_bboxes.shape[0], dtype=bool)
        return iou_coco(det_bboxes, gt_bboxes, gt_iscrowd)


@EVAL_MATCHER.register_module()
class MatcherCoCo:
    """mean_ap_flexible.py:28-36."""

    def __call__(self, ious, iou_thrs, gt_isignore=None, gt_iscrowd=None):
        if gt_iscrowd is None:
            gt_iscrowd = np.zeros(ious.shape[1], dtype=bool)
        if gt_isignore is None:
            gt_isignore = np.zeros(ious.shape[1], dtype=bool)
        return match_coco(ious, iou_thrs, gt_isignore, gt_iscrowd)


class NoBreakdown:
    """mean_ap_flexible.py:39-67: the single 'All' group; ignored gts drop out of it."""

    def __init__(self, classes, apply_to=None, *args, **kwargs):
        self.classes = classes
        self.apply_to = classes if apply_to is None else apply_to
        self.names = ['All']

    def breakdown_flags(self, boxes, attrs=None):
        flags = np.ones((1, len(boxes)), dtype=bool)
        if attrs is not None and 'ignore' in attrs:
            flags[:, attrs['ignore']] = False
        return flags

    def breakdown(self, boxes, label, attrs=None):
        flags = self.breakdown_flags(boxes, attrs)
        return flags if self.classes[label] in self.apply_to else flags[:0]

    def breakdown_names(self, label):
        return [f'{n}' for n in self.names] if self.classes[label] in self.apply_to else []


@EVAL_BREAKDOWN.register_module()
class ScaleBreakdown(NoBreakdown):
    """mean_ap_flexible.py:70-96: one group per (min_side, max_side) range, by box area."""

    def __init__(self, scale_ranges, classes, apply_to=None, *args, **kwargs):
        super().__init__(classes, apply_to, *args, **kwargs)
        self.names = list(scale_ranges)
        self.area_ranges = [(lo * lo, hi * hi) for lo, hi in scale_ranges.values()]

    def breakdown_flags(self, boxes, attrs=None):
        if attrs is not None and 'area' in attrs:
            area = attrs['area']
        else:
            wh = boxes[:, 2:] - boxes[:, :2]
            area = wh[:, 0] * wh[:, 1]
        flags = np.zeros((len(self.area_ranges), len(boxes)), dtype=bool)
        for i, (lo, hi) in enumerate(self.area_ranges):
            flags[i][(area >= lo) & (area < hi)] = True
        if attrs is not None and 'ignore' in attrs:
            flags[:, attrs['ignore']] = False
        return flags


class FlexGt:
    """The ground-truth side of the flat path, built once per dataset from the ``gt_bboxes`` / ``gt_labels`` /
    ``gt_attrs`` dicts ``eval_map_flexible`` takes per image (``coco_test_annotation``).  ``scale_ranges``: the
    ``ScaleBreakdown`` argument, name -> (min_side, max_side) (or a list of such pairs); B = 1 + their number.

    Holds the class-major gts (problem ``c * num_imgs + i``; a gt whose label is outside [0, C) takes no part) as
    ``gt (G, 4)``, ``gt_off (P + 1)``, ``crowd (G)``; ``gt_bkd (B, G)``: ``NoBreakdown`` / ``ScaleBreakdown.breakdown_flags``
    with ``ignore`` applied (``attrs['area']`` where given, else the box product); ``num_gt (C, B)``; ``bounds (B - 1, 2)``
    float32, the squared sides the device compares a detection's area with; and the matching kernel's static tables for
    the Q = P * B problems ``q = p * B + b``: ``q_gt_off (Q + 1)``, ``q_ignore`` / ``q_crowd (B * G)``.  Device copies are
    kept per device."""

    def __init__(self, annotations, num_classes, scale_ranges=None):
        self.annotations = annotations
        self.num_imgs, self.num_classes = len(annotations), int(num_classes)
        pairs = list(scale_ranges.items()) if isinstance(scale_ranges, dict) else list(scale_ranges or [])
        self.names = ['All'] + [str(k) for k, _ in pairs]
        self.area_ranges = [(lo * lo, hi * hi) for _, (lo, hi) in pairs]
        N, C, B = self.num_imgs, self.num_classes, len(self.names)
        if N <= 0 or C <= 0:
            raise ValueError('FlexGt needs at least one image and one class')
        if N * C * B >= 2 ** 31 - 1:
            raise ValueError(f'{N} images x {C} classes x {B} breakdowns: the problem index does not fit 31 bits')
        self.num_bkd = B
        self.bounds = np.array(self.area_ranges, dtype=np.float32).reshape(-1, 2)
        boxes, labels, imgs, crowd, flags = [np.zeros((0, 4), np.float32)], [], [], [], [np.zeros((B, 0), bool)]
        for i, anno in enumerate(annotations):
            gtb = np.asarray(anno['gt_bboxes'], dtype=np.float32).reshape(-1, 4)
            attrs = anno.get('gt_attrs') or {}
            n = len(gtb)
            if 'area' in attrs:
                area = np.asarray(attrs['area'])
            else:
                wh = gtb[:, 2:] - gtb[:, :2]
                area = wh[:, 0] * wh[:, 1]
            rows = np.ones((B, n), dtype=bool)
            for b, (lo, hi) in enumerate(self.area_ranges):
                rows[1 + b] = (area >= lo) & (area < hi)
            if 'ignore' in attrs:
                rows[:, np.asarray(attrs['ignore'], dtype=bool)] = False
            boxes.append(gtb)
            labels.append(np.asarray(anno['gt_labels'], dtype=np.int64).reshape(-1))
            imgs.append(np.full(n, i, np.int64))
            crowd.append(np.asarray(attrs['iscrowd'], dtype=bool) if 'iscrowd' in attrs else np.zeros(n, dtype=bool))
            flags.append(rows)
        boxes, flags = np.concatenate(boxes), np.concatenate(flags, axis=1)
        labels, imgs, crowd = (np.concatenate(x) if x else np.zeros(0, t) for x, t in
                               ((labels, np.int64), (imgs, np.int64), (crowd, bool)))
        if not (len(boxes) == len(labels) == len(crowd) == flags.shape[1]):
            raise ValueError('FlexGt: gt_bboxes, gt_labels and gt_attrs disagree in length')
        keep = np.flatnonzero((labels >= 0) & (labels < C))
        prob = labels[keep] * N + imgs[keep]
        sel = keep[np.argsort(prob, kind='stable')]          # class-major, the image's own gt order inside a problem
        P = N * C
        ng = np.bincount(prob, minlength=P).astype(np.int64)
        self.gt = np.ascontiguousarray(boxes[sel])
        self.crowd = crowd[sel].astype(np.uint8)
        self.gt_bkd = np.ascontiguousarray(flags[:, sel]).astype(np.uint8)
        self.gt_off = _offsets(ng)
        G = len(sel)
        cls_of = labels[sel]
        self.num_gt = np.stack([np.bincount(cls_of[self.gt_bkd[b] != 0], minlength=C) for b in range(B)],
                               axis=1).astype(np.int64)
        # the Q-side: problem p's gts once per breakdown, row b of its (B, ng) block at B * gt_off[p] + b * ng[p]
        self.q_gt_off = (B * np.repeat(self.gt_off[:-1], B) + np.tile(np.arange(B), P) * np.repeat(ng, B))
        self.q_gt_off = np.append(self.q_gt_off, B * G).astype(np.int64)
        pg = np.repeat(np.arange(P), ng)
        idx = (B * self.gt_off[pg] + (np.arange(G) - self.gt_off[pg]))[None, :] + np.arange(B)[:, None] * ng[pg][None, :]
        self.q_ignore, self.q_crowd = np.zeros(B * G, np.uint8), np.zeros(B * G, np.uint8)
        self.q_ignore[idx] = self.gt_bkd == 0
        self.q_crowd[idx] = self.crowd[None, :]
        self._device = {}

    def same_breakdown(self, names, area_ranges):
        return list(names) == self.names and [tuple(r) for r in area_ranges] == [tuple(r) for r in self.area_ranges]

    def device(self, dev):
        d = self._device.setdefault((dev.type, dev.index), {})
        if not d:
            pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)      # noqa: E731
            d.update(gt=_dev(pad(self.gt), np.float32, dev), crowd=_dev(pad(self.crowd), np.uint8, dev),
                     gt_off=_dev(self.gt_off, np.int64, dev), gt_bkd=_dev(pad(self.gt_bkd.reshape(-1)), np.uint8, dev),
                     num_gt=_dev(self.num_gt, np.int64, dev), bounds=_dev(pad(self.bounds.reshape(-1)), np.float32, dev),
                     q_gt_off=_dev(self.q_gt_off, np.int64, dev), q_ignore=_dev(pad(self.q_ignore), np.uint8, dev),
                     q_crowd=_dev(pad(self.q_crowd), np.uint8, dev))
        return d


def flex_flat_device(flat, gt, iou_thrs, shared_tp=True, phases=None):
    """The flat path of the module docstring on the device: ``yv4_map_rank``, one read-back (the pair total and the class
    counts), ``yv4_iou_coco_batched``, ``yv4_flex_tables``, ``yv4_match_coco_batched`` over the Q = P * B problems,
    ``yv4_flex_accumulate``, one download.  ``flat``: numpy arrays or GPU tensors (those never visit the host); ``gt``: a
    ``FlexGt``.  Returns host arrays shaped (C, B, T): ``num_det`` int64, ``recall`` float64, ``mAP`` float32.
    ``phases``: an optional dict that receives seconds per phase (each closed by a synchronise)."""
    dev = _eval_common._device('eval_utils', 'flex_flat')
    timer = PhaseTimer(phases, dev)
    thrs = np.ascontiguousarray(iou_thrs, dtype=np.float32).reshape(-1)
    N, C, B, T = gt.num_imgs, gt.num_classes, gt.num_bkd, len(thrs)
    if T == 0:
        raise ValueError('flat results need at least one IoU threshold')
    P, G = N * C, len(gt.gt)
    g = gt.device(dev)
    flat = _flat_to_device(flat, dev)
    t_thr = _dev(thrs, np.float32, dev)
    timer.mark('upload')
    lib = _lib.lib()
    det4, det_off, iou_off, _, _, cls_order, pairs, Dv, _ = rank_flat(flat, g['gt_off'], N, C, dev)
    timer.mark('rank')
    iou = torch.empty(max(pairs, 1), dtype=torch.float32, device=dev)
    if pairs:
        check(lib.yv4_iou_coco_batched(det4.data_ptr(), g['gt'].data_ptr(), g['crowd'].data_ptr(), det_off.data_ptr(),
                                       g['gt_off'].data_ptr(), iou_off.data_ptr(), P, pairs, iou.data_ptr(), stream_ptr()),
              'yv4_iou_coco_batched')
    matched = torch.empty(max(B * Dv * T, 1), dtype=torch.int32, device=dev)
    if Dv:
        Q = P * B
        q_det_off, q_iou_off = (torch.empty(Q + 1, dtype=torch.int64, device=dev) for _ in range(2))
        check(lib.yv4_flex_tables(det_off.data_ptr(), iou_off.data_ptr(), P, B, q_det_off.data_ptr(), q_iou_off.data_ptr(),
                                  stream_ptr()), 'yv4_flex_tables')
        work = torch.empty(max(B * G * T, 1), dtype=torch.uint8, device=dev)
        check(lib.yv4_match_coco_batched(iou.data_ptr(), q_det_off.data_ptr(), g['q_gt_off'].data_ptr(), q_iou_off.data_ptr(),
                                         t_thr.data_ptr(), T, g['q_ignore'].data_ptr(), g['q_crowd'].data_ptr(), Q,
                                         work.data_ptr(), matched.data_ptr(), stream_ptr()), 'yv4_match_coco_batched')
    timer.mark('match')
    num_det = torch.empty((C, B, T), dtype=torch.int64, device=dev)
    recall = torch.empty((C, B, T), dtype=torch.float64, device=dev)
    ap = torch.empty((C, B, T), dtype=torch.float32, device=dev)
    work = torch.empty(max(int(lib.yv4_flex_accumulate_work(Dv, T, B)), 8), dtype=torch.uint8, device=dev)
    check(lib.yv4_flex_accumulate(matched.data_ptr(), det4.data_ptr(), cls_order.data_ptr(), det_off.data_ptr(),
                                  g['gt_off'].data_ptr(), g['gt_bkd'].data_ptr(), g['num_gt'].data_ptr(),
                                  g['bounds'].data_ptr(), Dv, G, N, C, B, T, 1 if shared_tp else 0, work.data_ptr(),
                                  num_det.data_ptr(), recall.data_ptr(), ap.data_ptr(), stream_ptr()), 'yv4_flex_accumulate')
    timer.mark('accumulate')
    out = dict(num_det=num_det.cpu().numpy(), recall=recall.cpu().numpy(), mAP=ap.cpu().numpy(), num_gt=gt.num_gt,
               total_det=Dv, pairs=pairs)
    timer.mark('download')
    return out


class FlexibleStatisticsEval(object):
    """mean_ap_flexible.py:99-276.  ``nproc`` is accepted and ignored: the per-problem work the reference
    spreads over a process pool is one batched GPU launch here.  A custom ``iou_calculator`` / ``matcher``
    (anything but IOU2DCoCo / MatcherCoCo) is called per problem exactly as the reference does.

    ``shared_tp`` (default True = the reference's behaviour): statistics_single fills one ``cls_tp`` array
    in place per breakdown (:172,191-192) and appends that same object every time (:199-202), so all
    breakdowns of an (image, class) problem carry the true-positive flags of the LAST breakdown's matching.
    ``shared_tp=False`` gives every breakdown the flags of its own matching.

    ``statistics_eval`` also takes the flat table ``(dets (D, 5), labels (D,), img_index (D,))`` in place of the
    per-image lists and a ``FlexGt`` in place of ``annotations``: the module docstring's flat path, which knows exactly
    ``IOU2DCoCo``, ``MatcherCoCo`` and ``ScaleBreakdown`` entries with ``apply_to=None``."""

    def __init__(self, classes, iou_thrs, breakdown, iou_calculator, matcher, nproc, shared_tp=True):
        self.shared_tp = shared_tp
        self._breakdown_cfg = list(breakdown)
        self.classes = classes
        self.iou_thrs = iou_thrs
        self.breakdown = [NoBreakdown(classes)]
        self.breakdown += [build_from_cfg(b, EVAL_BREAKDOWN, default_args=dict(classes=classes))
                           for b in breakdown]
        self.iou_calculator = build_from_cfg(iou_calculator, EVAL_IOU_CALCULATOR)
        self.matcher = build_from_cfg(matcher, EVAL_MATCHER)
        self.nproc = nproc

    # ---- host: the (image, class) problems ------------------------------------------------------------
    def _problems(self, det_results, annotations):
        """Per (image, class): score-sorted detections, the class's gts, flags and breakdown masks."""
        probs = []
        for det, anno in zip(det_results, annotations):
            gt_bboxes, gt_labels, gt_attrs = anno['gt_bboxes'], anno['gt_labels'], anno['gt_attrs']
            for cls in range(len(det)):
                scores = det[cls][:, -1]
                order = scores.argsort()[::-1]
                boxes = det[cls][order, :-1]
                scores = scores[order]
                msk = gt_labels == cls
                gtb = gt_bboxes[msk]
                attrs = {k: v[msk] for k, v in gt_attrs.items()}
                crowd = attrs['iscrowd'] if 'iscrowd' in attrs else np.zeros(len(gtb), dtype=bool)
                det_bkd = np.concatenate([f.breakdown(boxes, cls) for f in self.breakdown], axis=0)
                gt_bkd = np.concatenate([f.breakdown(gtb, cls, attrs) for f in self.breakdown], axis=0)
                names = sum([f.breakdown_names(cls) for f in self.breakdown], [])
                probs.append((cls, boxes, scores, gtb, np.asarray(crowd, dtype=bool), det_bkd, gt_bkd, names))
        return probs

    def _match_all(self, probs):
        """One IoU launch + one matching launch for every problem with both detections and gts.
        Returns {problem index: (num_bkd, num_thrs, num_det) int32}."""
        live = [i for i, p in enumerate(probs) if len(p[1]) and len(p[3])]
        if not live:
            return {}
        dev = _device()
        nt = len(self.iou_thrs)
        nd = np.array([len(probs[i][1]) for i in live], np.int64)
        ng = np.array([len(probs[i][3]) for i in live], np.int64)
        nb = np.array([probs[i][6].shape[0] for i in live], np.int64)
        det = _dev(np.concatenate([probs[i][1][:, :4] for i in live]), np.float32, dev)
        gt = _dev(np.concatenate([probs[i][3][:, :4] for i in live]), np.float32, dev)
        crowd = _dev(np.concatenate([probs[i][4] for i in live]), np.bool_, dev)
        iou, iou_off = iou_coco_batched(det, gt, crowd, _offsets(nd), _offsets(ng))
        # matching problems: (problem, breakdown); the breakdowns of a problem share its IoU block
        q_det, q_gt = np.repeat(nd, nb), np.repeat(ng, nb)
        q_iou = np.repeat(iou_off[:-1], nb)
        ignore = _dev(np.concatenate([~probs[i][6].reshape(-1) for i in live]), np.bool_, dev)
        q_crowd = _dev(np.concatenate([np.tile(probs[i][4], probs[i][6].shape[0]) for i in live]), np.bool_, dev)
        q_det_off = _offsets(q_det)
        matched = match_coco_batched(iou, q_det_off, _offsets(q_gt), q_iou,
                                     np.array(self.iou_thrs, dtype=np.float32), ignore, q_crowd).cpu().numpy()
        out, q = {}, 0
        for k, i in enumerate(live):
            lo = q_det_off[q] * nt
            out[i] = matched[lo:lo + nb[k] * nt * nd[k]].reshape(nb[k], nt, nd[k])
            q += nb[k]
        return out

    def _custom_match_all(self, probs):
        thrs = np.array(self.iou_thrs, dtype=np.float32)
        out = {}
        for i, (cls, boxes, scores, gtb, crowd, det_bkd, gt_bkd, names) in enumerate(probs):
            if len(boxes) and len(gtb):
                ious = self.iou_calculator(boxes, gtb, crowd)
                out[i] = np.stack([self.matcher(ious, thrs, ~m, crowd) for m in gt_bkd]) if len(gt_bkd) else \
                    np.empty((0, len(thrs), len(boxes)), np.int32)
        return out

    # ---- the flat path ----------------------------------------------------------------------------------------------
    def _flat_breakdown(self):
        """(names, area_ranges) of the breakdown rows when the flat path knows this configuration."""
        if type(self.iou_calculator) is not IOU2DCoCo:
            raise NotImplementedError(f'flat results are scored on the device, which knows IOU2DCoCo only; for the '
                                      f'iou_calculator {type(self.iou_calculator).__name__} pass the per-image lists')
        if type(self.matcher) is not MatcherCoCo:
            raise NotImplementedError(f'flat results are scored on the device, which knows MatcherCoCo only; for the '
                                      f'matcher {type(self.matcher).__name__} pass the per-image lists')
        names, ranges = ['All'], []
        for cfg, f in zip(self._breakdown_cfg, self.breakdown[1:]):
            if type(f) is not ScaleBreakdown:
                raise NotImplementedError(f'flat results are scored on the device, which knows ScaleBreakdown only; for '
                                          f'the breakdown {type(f).__name__} pass the per-image lists')
            if cfg.get('apply_to') is not None:
                raise NotImplementedError(f'flat results are scored on the device, which knows ScaleBreakdown with '
                                          f'apply_to=None only; for apply_to={cfg["apply_to"]!r} pass the per-image lists')
            names += [str(n) for n in f.names]
            ranges += list(f.area_ranges)
        return names, ranges

    def _flat_gt(self, annotations):
        """The ``FlexGt`` the flat path scores against: the one given (checked against this configuration) or one built
        from the per-image dicts."""
        names, ranges = self._flat_breakdown()
        if isinstance(annotations, FlexGt):
            gt = annotations
            if not gt.same_breakdown(names, ranges):
                raise ValueError(f'the FlexGt was built for the breakdowns {gt.names} with areas {gt.area_ranges}, the '
                                 f'evaluation asks for {names} with {ranges}')
        else:
            if self.classes is None:
                raise ValueError('flat results carry no class count: pass a FlexGt or the class names')
            _device()                                           # refuse before the tables are built
            gt = FlexGt(annotations, len(self.classes),
                        [kv for cfg in self._breakdown_cfg for kv in cfg['scale_ranges'].items()])
        if self.classes is not None and len(self.classes) != gt.num_classes:
            raise ValueError(f'{len(self.classes)} class names, the FlexGt holds {gt.num_classes} classes')
        return gt

    def _flat_list(self, out, gt):
        """``flex_flat_device``'s tables as the list path's (key, value) pairs: class, breakdown, threshold."""
        results = []
        for c in range(gt.num_classes):
            cls_name = self.classes[c] if self.classes is not None else c
            for b, bkd in enumerate(gt.names):
                num_gt = int(gt.num_gt[c, b])
                for t, iou_thr in enumerate(self.iou_thrs):
                    results.append((dict(class_name=cls_name, breakdown=bkd, iou_threshold=iou_thr),
                                    dict(num_det=int(out['num_det'][c, b, t]), num_gt=num_gt,
                                         recall=out['recall'][c, b, t], mAP=out['mAP'][c, b, t])))
        return results

    def _flat_eval(self, flat, annotations):
        gt = self._flat_gt(annotations)
        return self._flat_list(flex_flat_device(flat, gt, self.iou_thrs, self.shared_tp), gt)

    def statistics_eval(self, det_results, annotations):
        """mean_ap_flexible.py:119-208 (per problem) and :225-260 (accumulate over the dataset); the flat tuple goes to
        the device whole."""
        if _is_flat(det_results):
            return self._flat_eval(det_results, annotations)
        if isinstance(annotations, FlexGt):
            annotations = annotations.annotations
        nt = len(self.iou_thrs)
        probs = self._problems(det_results, annotations)
        batched = type(self.iou_calculator) is IOU2DCoCo and type(self.matcher) is MatcherCoCo
        matched = self._match_all(probs) if batched else self._custom_match_all(probs)
        groups = OrderedDict()                       # (class index, breakdown row) -> accumulators
        for i, (cls, boxes, scores, gtb, crowd, det_bkd, gt_bkd, names) in enumerate(probs):
            cls_name = self.classes[cls] if self.classes is not None else cls
            for b in range(gt_bkd.shape[0]):
                g = groups.setdefault((cls, b), [cls_name, names[b], 0, [], [], []])
                g[2] += int(np.count_nonzero(gt_bkd[b]))
                g[3].append(scores)
                if i in matched:
                    mg = matched[i][b]
                    g[4].append((matched[i][-1] if self.shared_tp else mg) > -1)
                    g[5].append((det_bkd[b:b + 1] & (mg == -1)) | (gt_bkd[b][mg] & (mg > -1)))
                else:
                    g[4].append(np.zeros((nt, len(boxes)), dtype=bool))
                    g[5].append(det_bkd[b:b + 1].repeat(nt, axis=0))
        results = []
        for cls_name, bkd, num_gt, scores, tps, msks in groups.values():
            results += self.statistics_accumulate((cls_name, bkd, num_gt, np.concatenate(scores, axis=0),
                                                   np.concatenate(tps, axis=1), np.concatenate(msks, axis=1)))
        return results

    def statistics_accumulate(self, input):
        """mean_ap_flexible.py:210-227."""
        cls, bkd, num_gt, score, tp, bkd_msk = input
        rank = score.argsort()[::-1]
        tp, bkd_msk = tp[:, rank], bkd_msk[:, rank]
        out = []
        for t, iou_thr in enumerate(self.iou_thrs):
            tpcumsum = tp[t, bkd_msk[t]].cumsum()
            num_det = len(tpcumsum)
            recall = tpcumsum / max(num_gt, 1e-7)
            precision = tpcumsum / np.arange(1, num_det + 1)
            out.append((dict(class_name=cls, breakdown=bkd, iou_threshold=iou_thr),
                        dict(num_det=num_det, num_gt=num_gt, recall=recall.max() if len(recall) > 0 else 0,
                             mAP=average_precision(recall, precision))))
        return out

    def report(self, eval_result_list, group_by):
        """mean_ap_flexible.py:265-276."""
        report_dict = OrderedDict()
        for name, cond in group_by:
            report_dict[name] = np.mean([v['mAP'] for k, v in eval_result_list if cond(k) and v['num_gt'] > 0])
        return report_dict


def eval_map_flexible(det_results, annotations, iou_thrs=[0.5], breakdown=[], iou_calculator=dict(type='IOU2DCoCo'),
                      matcher=dict(type='MatcherCoCo'), classes=None, logger=None,
                      report_config=[('map', lambda x: x['breakdown'] == 'All')], nproc=None):
    """mean_ap_flexible.py:279-302.  ``det_results`` may be the flat tuple and ``annotations`` a ``FlexGt`` (the module
    docstring's flat path)."""
    if not _is_flat(det_results):
        assert len(det_results) == len(annotations.annotations if isinstance(annotations, FlexGt) else annotations)
    fse = FlexibleStatisticsEval(classes, iou_thrs, breakdown, iou_calculator, matcher, nproc or 0)
    return fse.report(fse.statistics_eval(det_results, annotations), report_config)


def coco_test_annotation(ann_info, cat_ids, cat2label):
    """One image's COCO annotation records -> the dict ``eval_map_flexible`` consumes
    (``CocoDataset.get_ann_info_test``, datasets/coco.py:357-409, without the mask / seg-map fields the bbox
    evaluation never reads).  ``ann_info``: the image's ``annotations`` entries (``bbox`` = x, y, w, h);
    crowd boxes and boxes of unlisted categories are kept and flagged ``ignore``."""
    boxes, labels, ignore, crowd, area = [], [], [], [], []
    for ann in ann_info:
        is_crowd = ann.get('iscrowd', False)
        ignore.append(bool(ann.get('ignore', False) or is_crowd or ann['category_id'] not in cat_ids))
        crowd.append(bool(is_crowd))
        area.append(ann['area'])
        x, y, w, h = ann['bbox']
        boxes.append([x, y, x + w, y + h])
        labels.append(cat2label[ann['category_id']])
    return dict(gt_bboxes=np.array(boxes, dtype=np.float32).reshape(-1, 4), gt_labels=np.array(labels, dtype=np.int64),
                gt_attrs=dict(ignore=np.array(ignore, dtype=bool), iscrowd=np.array(crowd, dtype=bool),
                              area=np.array(area, dtype=np.float32)))


#: the three object scales of ``metric='fast-bbox'`` (datasets/coco.py:476-479)
FAST_BBOX_SCALE_RANGES = OrderedDict(Scale_S=(0, 32), Scale_M=(32, 96), Scale_L=(96, 10000))


def evaluate_fast_bbox(results, annotations, classes, logger=None):
    """``dataset.evaluate(results, metric='fast-bbox')`` (datasets/coco.py:464-496): the ten COCO IoU thresholds, the
    three object-scale breakdowns, and the six-number report ``map, map50, map75, s_map, m_map, l_map``.  ``results``: the
    per-image lists or the flat tuple; ``annotations``: the per-image dicts or a ``FlexGt`` built with
    ``FAST_BBOX_SCALE_RANGES``."""
    return eval_map_flexible(
        results, annotations, iou_thrs=[0.5 + 0.05 * x for x in range(10)],
        breakdown=[dict(type='ScaleBreakdown', scale_ranges=dict(FAST_BBOX_SCALE_RANGES))],
        report_config=[('map', lambda x: x['breakdown'] == 'All'),
                       ('map50', lambda x: x['iou_threshold'] == 0.5 and x['breakdown'] == 'All'),
                       ('map75', lambda x: x['iou_threshold'] == 0.75 and x['breakdown'] == 'All'),
                       ('s_map', lambda x: x['breakdown'] == 'Scale_S'),
                       ('m_map', lambda x: x['breakdown'] == 'Scale_M'),
                       ('l_map', lambda x: x['breakdown'] == 'Scale_L')],
        classes=classes, iou_calculator=dict(type='IOU2DCoCo'), matcher=dict(type='MatcherCoCo'), nproc=-1, logger=logger)
