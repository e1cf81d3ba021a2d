"""COCO bbox evaluation, ``metric='bbox'``: ``CocoGt``, ``COCOeval`` (evaluate / accumulate / summarize) and
``evaluate_bbox``, the ``'bbox'`` branch of ``CocoDataset.evaluate`` (``mmdet/datasets/coco.py:451-643``).

The reference scores through ``pycocotools.cocoeval.COCOeval``.  Here the whole pipeline runs on the device
(csrc/coco_eval.hip): ``yv4_coco_rank`` orders the flat detection table by (problem, descending score),
``yv4_coco_match`` runs every (image, category) problem's IoU block and its A x T greedy walks on one wave, and
``yv4_coco_accumulate`` orders by (category, descending score), scans tp / fp, builds the precision envelope and samples
it at the recall thresholds.  Only ``precision`` / ``scores`` (T, R, K, A, M), ``recall`` (T, K, A, M) and the gt counts
(K, A) come back; ``summarize`` is a handful of ``np.mean`` calls.  There is no CPU implementation: without a GPU, or
with a library that lacks the entry points, the calls raise.

Parity: **bit-exact against the definition below; parity unpinned against pycocotools itself** (pycocotools is third
party and absent from the build image, as mmcv is).  COCOeval sorts with ``kind='mergesort'`` everywhere, so its order
is fully defined by (score, position) and two stable device sorts reproduce it.  Scores and boxes are expected finite.

Definition (COCOeval, ``iouType='bbox'``, ``useCats=1``, pycocotools 2.0.x):

* ``imgIds`` / ``catIds`` are replaced by ``np.unique`` of themselves; the K axis and the order in which a category's
  images are concatenated follow the sorted ids.
* Ground truth: ``bbox`` (x, y, w, h) and the record's own ``area`` as float64; ``ignore`` is overwritten by ``iscrowd``;
  grouped by (image, category) in annotation order.
* Detections, from a float32 row ``b`` = (x1, y1, x2, y2, score): box ``[float(b0), float(b1), float(b2) - float(b0),
  float(b3) - float(b1)]`` (the subtraction in float64, after the conversion), ``area = w * h``.
* ``maxDets`` is sorted by ``evaluate()``, so ``maxDets[-1]`` is the largest.
* Per problem: detections by descending score, stable, the first ``maxDets[-1]`` kept.  IoU in float64: ``w =
  min(dx+dw, gx+gw) - max(dx, gx)``, 0 when ``w <= 0``; ``h`` likewise; ``inter = w*h``; ``union = da`` for a crowd gt,
  else ``da + ga - inter`` with ``da = dw*dh``, ``ga = gw*gh``.
* Per (problem, area range [lo, hi]): gt ``_ignore = ignore or area < lo or area > hi``; gts stably sorted by ``_ignore``.
  Per threshold t, per detection in rank order: ``best = min(t, 1 - 1e-10)``; walk the gts: skip one already matched at
  t unless it is crowd; stop when the current match is not ignored and this gt is; skip when ``iou < best``; else take
  it (equality passes, the later gt wins).  A matched detection inherits its gt's ``_ignore``; an unmatched one whose own
  area is outside [lo, hi] is ignored.
* Per (k, a, m): the category's problems in image order, the first ``maxDets[m]`` detections of each, concatenated and
  ordered by descending score, stable.  ``npig`` = gts with ``_ignore == 0``; ``npig == 0`` leaves -1.  Per t: ``tp`` /
  ``fp`` cumulative counts of matched / unmatched non-ignored detections, ``rc = tp / npig``, ``pr = tp / (fp + tp +
  np.spacing(1))``, ``recall = rc[-1]`` (0 without detections), ``pr`` made non-increasing from the right, ``inds =
  np.searchsorted(rc, recThrs, side='left')``, ``precision[r] = pr[inds[r]]`` and ``scores[r]`` the score there while
  ``inds[r] < nd``, 0 afterwards.
* ``summarize``: the mean of the entries > -1 of a slice (-1 if none); ``stats[0]`` uses pycocotools' literal default
  ``maxDets == 100``, the others ``maxDets[2]`` (AP, AR small / medium / large) and ``maxDets[0..2]`` (AR).
"""
import json
import logging
import time
from collections import OrderedDict

import numpy as np
import torch

from . import _eval_common, _lib
from ._eval_common import _dev, _is_flat, _log, _offsets, _ptr
from ._lib import check
from .ops import stream_ptr

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_RNG_LBL = ['all', 'small', 'medium', 'large']
METRIC_NAMES = {'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5, 'AR@100': 6, 'AR@300': 7,
                'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10, 'AR_l@1000': 11}


def _device():
    return _eval_common._device('coco_eval', 'coco_eval')


class CocoGt:
    """A COCO annotation file without pycocotools: ``dataset`` is the parsed dict or a path to the json.  The flat
    ground-truth tables (one row per annotation, in annotation order): ``ann_img`` / ``ann_cat`` int64 ids, ``ann_box``
    (n, 4) float64 x y w h, ``ann_area`` float64 (the record's own field), ``ann_crowd`` and ``ann_ignore`` bytes --
    ``ignore`` is overwritten by ``iscrowd``, as ``COCOeval._prepare`` does."""

    def __init__(self, dataset):
        if not isinstance(dataset, dict):
            with open(dataset) as f:
                dataset = json.load(f)
        self.dataset = dataset
        self.imgs = OrderedDict((im['id'], im) for im in dataset.get('images', []))
        self.cats = OrderedDict((c['id'], c) for c in dataset.get('categories', []))
        anns = dataset.get('annotations', [])
        self.ann_img = np.array([a['image_id'] for a in anns], dtype=np.int64)
        self.ann_cat = np.array([a['category_id'] for a in anns], dtype=np.int64)
        self.ann_box = np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(-1, 4)
        self.ann_area = np.array([a['area'] for a in anns], dtype=np.float64)
        self.ann_crowd = np.array([1 if a.get('iscrowd', 0) else 0 for a in anns], dtype=np.uint8)
        self.ann_ignore = self.ann_crowd.copy()          # gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']

    def get_img_ids(self):
        return list(self.imgs)

    def get_cat_ids(self, cat_names=()):
        cat_names = [cat_names] if isinstance(cat_names, str) else list(cat_names)
        return [c['id'] for c in self.cats.values() if not cat_names or c['name'] in cat_names]

    def load_cats(self, ids=()):
        ids = list(ids) if isinstance(ids, (list, tuple, np.ndarray)) else [ids]
        return [self.cats[int(i)] for i in ids]

    def cat_group(self):
        """``{category id: supercategory group}``, the groups numbered in the order ``categories`` first names them.  A
        category without a ``supercategory`` key forms a group of its own (``getCatIds(supNms=...)`` of the reference
        raises ``KeyError`` there)."""
        groups, out = {}, {}
        for cid, c in self.cats.items():
            key = ('name', c['supercategory']) if 'supercategory' in c else ('alone', cid)
            out[cid] = groups.setdefault(key, len(groups))
        return out


class Params:
    """``pycocotools.cocoeval.Params`` for ``iouType='bbox'``."""

    def __init__(self, iou_type='bbox'):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [list(r) for r in AREA_RNG]
        self.areaRngLbl = list(AREA_RNG_LBL)
        self.useCats = 1
        self.iouType = iou_type


def flatten_results(results):
    """The reference's result form -- per image a per-class list of (n, 5) float32 arrays -- as the flat form
    ``(dets (D, 5) float32, labels (D,) int64, img_index (D,) int64)``, rows in ``_det2json``'s order (image, class,
    row).  One concatenation per image."""
    C = len(results[0]) if len(results) else 0
    parts, lens = [np.zeros((0, 5), np.float32)], np.zeros((len(results), C), np.int64)
    for i, res in enumerate(results):
        if len(res) != C:
            raise ValueError(f'image {i} has {len(res)} class lists, image 0 has {C}')
        lens[i] = np.fromiter(map(len, res), np.int64, C)
        if lens[i].any():
            parts.append(np.concatenate(res, axis=0))
    dets = np.concatenate(parts, axis=0)
    if dets.dtype != np.float32 or dets.ndim != 2 or dets.shape[1] != 5:
        dets = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    labels = np.repeat(np.tile(np.arange(C, dtype=np.int64), len(results)), lens.reshape(-1))
    img_index = np.repeat(np.arange(len(results), dtype=np.int64), lens.sum(axis=1))
    return dets, labels, img_index


class COCOeval:
    """``COCOeval(coco_gt, results, 'bbox')`` with ``evaluate()``, ``accumulate()`` and ``summarize()``.

    ``results``: the reference's form (per image a per-class list of (n, 5) float32 arrays, images in ``img_ids``
    order), or the flat tuple ``(dets (D, 5), labels (D,), img_index (D,))`` of numpy arrays or GPU tensors -- the
    detector's output before ``bbox2result``; GPU tensors never visit the host.  ``cat_ids[label]`` is a detection's
    category id and ``img_ids[img_index]`` its image id (defaults: the annotation file's order).  ``params.catIds`` /
    ``params.imgIds`` start as those lists.  After ``accumulate()``: ``eval['precision' | 'scores']`` (T, R, K, A, M),
    ``eval['recall']`` (T, K, A, M), ``eval['counts']`` (K, A); after ``summarize()``: ``stats`` (12 float64).
    ``phases``: seconds per phase of the last run (each closed by a device synchronise) when ``timing=True``."""

    def __init__(self, coco_gt, results, iou_type='bbox', cat_ids=None, img_ids=None, timing=False):
        if iou_type != 'bbox':
            raise NotImplementedError(f"iou_type={iou_type!r} is not built: no detector of this package produces masks or "
                                      'keypoints; only iou_type=\'bbox\' is')
        self.cocoGt = coco_gt
        self.results = results
        self.cat_ids = list(coco_gt.get_cat_ids() if cat_ids is None else cat_ids)
        self.img_ids = list(coco_gt.get_img_ids() if img_ids is None else img_ids)
        self.params = Params(iou_type)
        self.params.catIds = list(self.cat_ids)
        self.params.imgIds = list(self.img_ids)
        self.eval = {}
        self.stats = []
        self.timing = timing
        self.phases = {}
        self._dev = None

    # ---- host tables --------------------------------------------------------------------------------------------------
    def tables(self):
        """The problem tables (host, vectorised numpy): sorted ids, the gts grouped by problem ``image * K + category``
        in annotation order, and the maps from a detection's label / image index to its K / image axis position (-1:
        takes no part)."""
        p = self.params
        if not p.useCats:
            raise NotImplementedError('useCats=0 (category-agnostic evaluation: the proposal metrics, which the reference '
                                      "computes from a detector's own boxes, datasets/coco.py:288,574) is not built")
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        img_sorted, cat_sorted = np.asarray(p.imgIds, np.int64), np.asarray(p.catIds, np.int64)
        N, K = len(img_sorted), len(cat_sorted)
        if N == 0 or K == 0:
            raise ValueError('params.imgIds and params.catIds must not be empty')
        if N * K >= 2 ** 31 - 1:
            raise ValueError(f'{N} images x {K} categories: the problem index does not fit 31 bits')

        def position(sorted_ids, ids):
            ids = np.asarray(ids, np.int64).reshape(-1)
            pos = np.searchsorted(sorted_ids, ids)
            pos[pos == len(sorted_ids)] = 0
            return np.where(sorted_ids[pos] == ids, pos, -1)
        g = self.cocoGt
        gi, gk = position(img_sorted, g.ann_img), position(cat_sorted, g.ann_cat)
        keep = np.flatnonzero((gi >= 0) & (gk >= 0))
        prob = gi[keep] * K + gk[keep]
        by = keep[np.argsort(prob, kind='stable')]         # annotation order inside a problem
        flag = (g.ann_crowd[by] != 0).astype(np.uint8) | ((g.ann_ignore[by] != 0).astype(np.uint8) << 1)
        return dict(N=N, K=K, P=N * K, img_ids=img_sorted, cat_ids=cat_sorted,
                    gt_box=np.ascontiguousarray(g.ann_box[by]), gt_area=np.ascontiguousarray(g.ann_area[by]), gt_flag=flag,
                    gt_off=_offsets(np.bincount(prob, minlength=N * K)),
                    kmap=position(cat_sorted, self.cat_ids), imap=position(img_sorted, self.img_ids))

    def flat_results(self):
        """(dets, labels, img_index): numpy arrays, or GPU tensors when the flat form was given as tensors."""
        r = self.results
        if not _is_flat(r):
            return flatten_results(r)
        dets, labels, img_index = r
        if isinstance(dets, torch.Tensor):
            return dets, labels, img_index
        return (np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 5), np.asarray(labels, np.int64).reshape(-1),
                np.asarray(img_index, np.int64).reshape(-1))

    # ---- device ----------------------------------------------------------------------------------------------------------
    def _tick(self):
        if not self.timing:
            return 0.0
        if self._dev is not None:
            torch.cuda.synchronize(self._dev)
        return time.perf_counter()

    def evaluate(self):
        """Ordering and matching.  Leaves the per-detection flags and the gt counts on the device."""
        t0 = self._tick()
        tab = self.tables()
        dets, labels, img_index = self.flat_results()
        t1 = self._tick()
        dev = self._dev = _device()
        p = self.params
        K, P = tab['K'], tab['P']
        thrs = np.ascontiguousarray(p.iouThrs, dtype=np.float64).reshape(-1)
        area = np.ascontiguousarray(p.areaRng, dtype=np.float64).reshape(-1, 2)
        T, A = len(thrs), len(area)
        if T == 0 or A == 0 or len(p.maxDets) == 0:
            raise ValueError('params.iouThrs, params.areaRng and params.maxDets must not be empty')
        max_last = int(p.maxDets[-1])
        dets = dets.to(dev, torch.float32).contiguous() if isinstance(dets, torch.Tensor) else _dev(dets, np.float32, dev)
        labels = labels.to(dev) if isinstance(labels, torch.Tensor) else _dev(labels, np.int64, dev)
        img_index = img_index.to(dev) if isinstance(img_index, torch.Tensor) else _dev(img_index, np.int64, dev)
        D = int(dets.shape[0])
        if dets.dim() != 2 or dets.shape[1] != 5 or labels.numel() != D or img_index.numel() != D:
            raise ValueError('flat results: dets (D, 5), labels (D,), img_index (D,)')
        kmap, imap = _dev(tab['kmap'], np.int64, dev), _dev(tab['imap'], np.int64, dev)
        labels, img_index = labels.reshape(-1).long(), img_index.reshape(-1).long()
        ok = (labels >= 0) & (labels < len(kmap)) & (img_index >= 0) & (img_index < len(imap))
        k = kmap[labels.clamp(0, len(kmap) - 1)]
        i = imap[img_index.clamp(0, len(imap) - 1)]
        prob = torch.where(ok & (k >= 0) & (i >= 0), i * K + k, torch.full_like(k, -1)).to(torch.int32)
        gt_box, gt_area = _dev(tab['gt_box'].reshape(-1), np.float64, dev), _dev(tab['gt_area'], np.float64, dev)
        gt_flag, gt_off = _dev(tab['gt_flag'], np.uint8, dev), _dev(tab['gt_off'], np.int64, dev)
        t_thr, t_area = _dev(thrs, np.float64, dev), _dev(area.reshape(-1), np.float64, dev)
        t2 = self._tick()

        lib = _lib.lib()
        n1 = max(D, 1)
        order = torch.empty(n1, dtype=torch.int32, device=dev)
        sprob = torch.empty(n1, dtype=torch.int32, device=dev)
        det_off = torch.empty(P + 1, dtype=torch.int64, device=dev)
        need = torch.zeros(1, dtype=torch.int64, device=dev)
        work = torch.empty(int(lib.yv4_coco_rank_work(D)) // 8 + 1, dtype=torch.int64, device=dev)
        check(lib.yv4_coco_rank(dets.data_ptr() if D else None, prob.data_ptr() if D else None, D, P, max_last, A * T,
                                gt_off.data_ptr(), work.data_ptr(), order.data_ptr(), sprob.data_ptr(), det_off.data_ptr(),
                                need.data_ptr(), stream_ptr()), 'yv4_coco_rank')
        need = int(need.item())
        del work
        t3 = self._tick()
        mwork = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)
        flags = torch.empty(n1 * A * T, dtype=torch.uint8, device=dev)
        counts = torch.empty(K * A, dtype=torch.int32, device=dev)
        check(lib.yv4_coco_match(_ptr(dets), order.data_ptr(), det_off.data_ptr(), _ptr(gt_box), _ptr(gt_area), _ptr(gt_flag),
                                 gt_off.data_ptr(), P, K, D, max_last, t_thr.data_ptr(), T, t_area.data_ptr(), A,
                                 mwork.data_ptr(), need, state.data_ptr(), flags.data_ptr(), counts.data_ptr(),
                                 stream_ptr()), 'yv4_coco_match')
        t4 = self._tick()
        self._state = dict(tab=tab, dets=dets, order=order, sprob=sprob, det_off=det_off, flags=flags, counts=counts,
                           state=state, D=D, T=T, A=A, thrs=thrs, max_last=max_last)
        if self.timing:
            self.phases.update(table_build=t1 - t0, upload=t2 - t1, ordering=t3 - t2, matching=t4 - t3)

    def det_bits(self):
        """``evalImgs``-style detail of ``evaluate()``: for the detections that take part (rank < maxDets[-1]), in
        (problem, rank) order: ``index`` (row of the flat detection table), ``problem``, ``rank`` and the ``matched`` /
        ``ignored`` bits (A, T, n)."""
        s = self._state
        D, A, T = s['D'], s['A'], s['T']
        det_off = s['det_off'].cpu().numpy()
        n = int(det_off[-1])
        order, sprob = s['order'].cpu().numpy()[:n].astype(np.int64), s['sprob'].cpu().numpy()[:n].astype(np.int64)
        rank = np.arange(n, dtype=np.int64) - det_off[sprob]
        keep = rank < s['max_last']
        f = s['flags'].cpu().numpy()[:D * A * T].reshape(D, A, T)[:n][keep].transpose(1, 2, 0)
        return dict(index=order[keep], problem=sprob[keep], rank=rank[keep], matched=(f & 1) != 0, ignored=(f & 2) != 0)

    def accumulate(self):
        """The per-category ordering, the scans and the 101-point sampling; downloads the result arrays."""
        if not getattr(self, '_state', None):
            raise RuntimeError('Please run evaluate() first')
        s, p = self._state, self.params
        dev, tab = self._dev, s['tab']
        K, P, D, T, A = tab['K'], tab['P'], s['D'], s['T'], s['A']
        t0 = self._tick()
        rec = np.ascontiguousarray(p.recThrs, dtype=np.float64).reshape(-1)
        md = np.ascontiguousarray(p.maxDets, dtype=np.int32).reshape(-1)
        R, M = len(rec), len(md)
        lib = _lib.lib()
        t_rec = torch.from_numpy(rec).to(dev)
        work = torch.empty(int(lib.yv4_coco_accumulate_work(D, K, A * T)) // 8 + 1, dtype=torch.int64, device=dev)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        check(lib.yv4_coco_accumulate(s['dets'].data_ptr() if D else None, s['order'].data_ptr(), s['sprob'].data_ptr(),
                                      s['det_off'].data_ptr(), s['flags'].data_ptr(), s['counts'].data_ptr(), P, K, D,
                                      md.ctypes.data, M, T, A, t_rec.data_ptr(), R, work.data_ptr(), precision.data_ptr(),
                                      recall.data_ptr(), scores.data_ptr(), stream_ptr()), 'yv4_coco_accumulate')
        t1 = self._tick()
        state = s['state'].cpu().numpy()
        if state[1]:
            raise RuntimeError('yv4_coco_match ran out of workspace (internal error: the size came from yv4_coco_rank)')
        self.eval = dict(params=p, shape=[T, R, K, A, M], precision=precision.cpu().numpy(), recall=recall.cpu().numpy(),
                         scores=scores.cpu().numpy())
        self.eval['counts'] = s['counts'].cpu().numpy().reshape(K, A)
        t2 = self._tick()
        if self.timing:
            self.phases.update(accumulation=t1 - t0, download=t2 - t1)

    # ---- host: twelve means ---------------------------------------------------------------------------------------------
    def _summarize(self, ap=1, iouThr=None, areaRng='all', maxDets=100, out=print):
        p = self.params
        iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
        typeStr = '(AP)' if ap == 1 else '(AR)'
        iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        s = self.eval['precision'] if ap == 1 else self.eval['recall']
        if iouThr is not None:
            s = s[np.where(iouThr == np.asarray(p.iouThrs))[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        out(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    def summarize(self, out=print):
        """The twelve numbers, printed in pycocotools' format."""
        if not self.eval:
            raise RuntimeError('Please run accumulate() first')
        t0 = time.perf_counter()
        md = self.params.maxDets
        if len(md) < 3:
            raise ValueError('summarize reads maxDets[0], [1] and [2]')
        S = self._summarize
        stats = np.zeros((12,))
        stats[0] = S(1, out=out)
        stats[1] = S(1, iouThr=.5, maxDets=md[2], out=out)
        stats[2] = S(1, iouThr=.75, maxDets=md[2], out=out)
        stats[3] = S(1, areaRng='small', maxDets=md[2], out=out)
        stats[4] = S(1, areaRng='medium', maxDets=md[2], out=out)
        stats[5] = S(1, areaRng='large', maxDets=md[2], out=out)
        stats[6] = S(0, maxDets=md[0], out=out)
        stats[7] = S(0, maxDets=md[1], out=out)
        stats[8] = S(0, maxDets=md[2], out=out)
        stats[9] = S(0, areaRng='small', maxDets=md[2], out=out)
        stats[10] = S(0, areaRng='medium', maxDets=md[2], out=out)
        stats[11] = S(0, areaRng='large', maxDets=md[2], out=out)
        self.stats = stats
        if self.timing:
            self.phases['summarize'] = time.perf_counter() - t0

    def __str__(self):
        self.summarize()
        return ''


def evaluate_bbox(results, coco_gt, classes=None, cat_ids=None, img_ids=None, logger=None, classwise=False,
                  proposal_nums=(100, 300, 1000), iou_thrs=None, metric_items=None, metric='bbox'):
    """``dataset.evaluate(results, metric='bbox')`` (datasets/coco.py:451-643): ``bbox_mAP``, ``bbox_mAP_50``, ... rounded
    with ``float(f'{v:.3f}')``, and ``bbox_mAP_copypaste``.  ``coco_gt``: a ``CocoGt``, a parsed annotation dict or a
    path.  ``classes`` selects ``cat_ids = coco_gt.get_cat_ids(cat_names=classes)`` as ``CocoDataset.load_annotations``
    does; ``cat_ids`` / ``img_ids`` give the label -> category and index -> image maps directly.  ``classwise`` reads
    ``precisions[:, :, idx, 0, -1]`` with ``idx`` running over ``cat_ids`` as given, literally as the reference indexes
    it; the table is plain text of this package's own.

    ``metric='proposal_fast'`` is scored by ``CocoBBoxDataset.evaluate`` itself (``fast_eval_recall`` on
    ``recall_eval.eval_recalls``), before anything reaches this function, which keeps refusing the name together with
    ``'proposal'`` (COCOeval with ``useCats = 0``, not built)."""
    metrics = metric if isinstance(metric, list) else [metric]
    for m in metrics:
        if m not in ('bbox', 'segm', 'proposal', 'proposal_fast'):
            raise KeyError(f'metric {m} is not supported')
    for m in metrics:
        if m in ('proposal', 'proposal_fast'):
            # (the reference scores a detector's own boxes under this name, category-agnostically: the proposal
            # file IS the bbox file, datasets/coco.py:288, and useCats = 0, :574)
            raise NotImplementedError(f"metric='{m}' is not built: the reference scores the detector's own boxes under "
                                      'this name, category-agnostically (datasets/coco.py:288,574), so no detector of '
                                      'this package is excluded by what it produces; the scoring itself is missing')
        if m == 'segm':
            raise NotImplementedError("metric='segm' is not built: it scores masks, which no detector of this package "
                                      'produces')
    if not isinstance(coco_gt, CocoGt):
        coco_gt = CocoGt(coco_gt)
    if iou_thrs is None:
        iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    if metric_items is not None and not isinstance(metric_items, list):
        metric_items = [metric_items]
    if cat_ids is None:
        cat_ids = coco_gt.get_cat_ids(cat_names=classes or ())
    if img_ids is None:
        img_ids = coco_gt.get_img_ids()
    eval_results = OrderedDict()
    for m in metrics:
        msg = f'Evaluating {m}...'
        _log('\n' + msg if logger is None else msg, logger)
        if not _is_flat(results):
            results = flatten_results(results)             # once: the emptiness test and COCOeval share it
        if int(results[0].shape[0]) == 0:
            _log('The testing results of the whole dataset is empty.', logger, logging.ERROR)
            break
        coco_eval = COCOeval(coco_gt, results, m, cat_ids=cat_ids, img_ids=img_ids)
        coco_eval.params.catIds = list(cat_ids)
        coco_eval.params.imgIds = list(img_ids)
        coco_eval.params.maxDets = list(proposal_nums)
        coco_eval.params.iouThrs = iou_thrs
        if metric_items is not None:
            for item in metric_items:
                if item not in METRIC_NAMES:
                    raise KeyError(f'metric item {item} is not supported')
        coco_eval.evaluate()
        coco_eval.accumulate()
        coco_eval.summarize()
        if classwise:
            precisions = coco_eval.eval['precision']
            assert len(cat_ids) == precisions.shape[2]
            rows = []
            for idx, cat_id in enumerate(cat_ids):
                nm = coco_gt.load_cats(cat_id)[0]
                precision = precisions[:, :, idx, 0, -1]
                precision = precision[precision > -1]
                ap = np.mean(precision) if precision.size else float('nan')
                rows.append((f'{nm["name"]}', f'{float(ap):0.3f}'))
            _log('\n' + _classwise_table(rows), logger)
        items = metric_items if metric_items is not None else ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
        for item in items:
            eval_results[f'{m}_{item}'] = float(f'{coco_eval.stats[METRIC_NAMES[item]]:.3f}')
        ap = coco_eval.stats[:6]
        eval_results[f'{m}_mAP_copypaste'] = (f'{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} '
                                              f'{ap[4]:.3f} {ap[5]:.3f}')
    return eval_results


def _classwise_table(rows):
    """category / AP pairs, up to three pairs per line (plain text; terminaltables is not used and no parity is claimed)."""
    per_line = min(3, max(len(rows), 1))
    cells = [('category', 'AP')] * per_line
    lines = [cells] + [rows[i:i + per_line] for i in range(0, len(rows), per_line)]
    lines = [list(ln) + [('', '')] * (per_line - len(ln)) for ln in lines]
    w0 = max(len(c[0]) for ln in lines for c in ln)
    w1 = max(len(c[1]) for ln in lines for c in ln)
    rule = '+' + '+'.join('-' * (w0 + 2) + '+' + '-' * (w1 + 2) for _ in range(per_line)) + '+'
    out = [rule]
    for n, ln in enumerate(lines):
        out.append('| ' + ' | '.join(f'{a.ljust(w0)} | {b.ljust(w1)}' for a, b in ln) + ' |')
        if n == 0:
            out.append(rule)
    out.append(rule)
    return '\n'.join(out)
