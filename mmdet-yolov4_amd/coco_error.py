"""COCO error analysis, ``tools/analysis_tools/coco_error_analysis.py`` of the reference (after Hoiem et al.): the seven
precision curves C75 / C50 / Loc / Sim / Oth / BG / FN per category and area range, in one pass on the device.

The reference runs ``COCOeval`` 1 + 2 K times.  Here ``yv4_coco_rank`` orders the detections once,
``yv4_coco_error_match`` (csrc/coco_error.hip) computes every (image, category) problem's IoU block against ALL ground
truths of the image once and runs the base, "Sim" and "Oth" walks on it side by side, and ``yv4_coco_accumulate``,
unchanged, turns the ``T + 2`` flag columns into ``precision (T + 2, R, K, A, 1)``: rows 0..4 of the tool's ``ps``.  There
is no CPU implementation: without a GPU, or with a library that lacks the entry points, the call raises.

Parity: **bit-exact against the definition below; parity unpinned against pycocotools itself** (absent from the build
image, as for ``metric='bbox'``; the ``COCOeval`` definition is the one of ``coco_eval.py``).

Definition (``coco_error_analysis.py:173-304``, ``iou_type='bbox'``):

1. Base: ``COCOeval`` with ``iouThrs = [0.75, 0.5, 0.1]`` in this order, ``maxDets = [100]``, ``areaRng = [[0, a2], [0, a0],
   [a0, a1], [a1, a2]]`` for ``--areas a0 a1 a2`` (default 1024 9216 1e10).  ``precision`` gives ``ps[0..2]``.
2. Sim, per category c: only the detections of c; every annotation whose category shares c's ``supercategory`` and is
   not c becomes ``category_id = c, ignore = 1, iscrowd = 1``; ``COCOeval`` at ``iouThrs = [0.1]``; ``precision[0, :, k]``
   gives ``ps[3, :, k]``.
3. Oth, per category c: the same with every annotation whose category is not c -- one of a category that
   ``categories`` does not list included.  ``ps[4, :, k]``.
4. ``ps[ps == -1] = 0``; ``ps[5] = ps[4] > 0``; ``ps[6] = 1.0``.
5. The numbers of the figures: per area range ``ps[type, :, k, a, 0].mean()``; for "allclass" the mean runs over K too,
   the zero rows of empty categories included.

What makes one pass possible:

* A relabelled ground truth is always ignored, so ``npig`` (``counts[k][a]``) is the same in all three runs.
* A relabelled ground truth is crowd: its IoU with a detection is ``inter / det_area``, it may be matched again and again,
  and a detection matched to it is ignored, neither tp nor fp.
* The detections of problem (image, c) are the same in all three runs: one rank order, one ``det_off``, one ``flags``
  table with more columns.
* Inside a problem the ground truths are walked "not ignored first, stable", in the order of the annotations of the
  image: the relabelled ones sit among c's own ignored ones in annotation order, not after them, and with equal IoUs
  the later one wins.
* Ground truths of c keep their own ``iscrowd`` / ``ignore`` and the ordinary IoU.

Stated differences: the K axis is the sorted category ids, as ``COCOeval``'s is -- the reference's tool indexes it by
``enumerate(cocoGt.getCatIds())``, file order, which is the same only for files sorted by id; here each class is labelled
by its own name.  A category without a ``supercategory`` key forms a group of its own (the reference raises
``KeyError``).  With ``cat_ids`` a subset of the file's categories, an annotation of a category outside it takes part in
the Oth walks only.
"""
import json
import pickle
import time
import warnings

import numpy as np
import torch

from . import _eval_common, _lib
from ._eval_common import _dev, _flat_to_device, _is_flat, _offsets, _ptr
from ._lib import check
from .coco_eval import CocoGt, flatten_results
from .ops import stream_ptr

TYPES = ('C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN')
AREA_NAMES = ('allarea', 'small', 'medium', 'large')
DEFAULT_AREAS = (1024, 9216, 10000000000)
PHASES = ('table_build', 'upload', 'ordering', 'matching', 'accumulation', 'download', 'post')


def area_ranges(areas=None):
    """``--areas a0 a1 a2`` as the tool's four ranges (A, 2) float64."""
    a = DEFAULT_AREAS if areas is None else tuple(areas)
    if len(a) != 3:
        raise ValueError('3 integers should be specified as areas, representing 3 area regions')
    return np.array([[0 ** 2, a[2]], [0 ** 2, a[0]], [a[0], a[1]], [a[1], a[2]]], dtype=np.float64)


def _position(sorted_ids, ids):
    ids = np.asarray(ids, np.int64).reshape(-1)
    if len(sorted_ids) == 0:
        return np.full(len(ids), -1, np.int64)
    pos = np.searchsorted(sorted_ids, ids)
    pos[pos == len(sorted_ids)] = 0
    return np.where(sorted_ids[pos] == ids, pos, -1)


def tables(coco_gt, cat_ids=None, img_ids=None):
    """The host tables (vectorised numpy): the sorted ids, the ground truths image-major in annotation order with the
    K-axis position of their category (-1: outside the K axis), the supercategory group of each K-axis position, and
    the maps from a detection's label / image index to its K / image axis position (-1: takes no part)."""
    cat_ids = list(coco_gt.get_cat_ids() if cat_ids is None else cat_ids)
    img_ids = list(coco_gt.get_img_ids() if img_ids is None else img_ids)
    img_sorted, cat_sorted = np.unique(np.asarray(img_ids, np.int64)), np.unique(np.asarray(cat_ids, np.int64))
    N, K = len(img_sorted), len(cat_sorted)
    if N == 0 or K == 0:
        raise ValueError('img_ids and cat_ids must not be empty')
    if N * K >= 2 ** 31 - 1:
        raise ValueError(f'{N} images x {K} categories: the problem index does not fit 31 bits')
    g = coco_gt
    gi = _position(img_sorted, g.ann_img)
    keep = np.flatnonzero(gi >= 0)
    by = keep[np.argsort(gi[keep], kind='stable')]          # annotation order inside an image
    flag = (g.ann_crowd[by] != 0).astype(np.uint8) | ((g.ann_ignore[by] != 0).astype(np.uint8) << 1)
    groups = coco_gt.cat_group()
    spare = max(groups.values(), default=-1) + 1            # a category the file does not list: a group of its own
    cat_group = np.array([groups.get(int(c), spare + k) for k, c in enumerate(cat_sorted)], dtype=np.int32)
    return dict(N=N, K=K, P=N * K, img_ids=img_sorted, cat_ids=cat_sorted,
                gt_box=np.ascontiguousarray(g.ann_box[by]), gt_area=np.ascontiguousarray(g.ann_area[by]), gt_flag=flag,
                gt_cat=_position(cat_sorted, g.ann_cat[by]).astype(np.int32),
                gt_img_off=_offsets(np.bincount(gi[keep], minlength=N)), cat_group=cat_group,
                kmap=_position(cat_sorted, cat_ids), imap=_position(img_sorted, img_ids))


def read_json_results(path_or_list, cat_ids, img_ids):
    """A bbox result ``.json`` as ``results2json`` writes it (a list of ``{image_id, bbox: [x, y, w, h], score,
    category_id}``) -> the flat form.  A row is rebuilt as float32 ``x, y, x + w, y + h, score``; the rows that this does
    not give back exactly (the evaluation reads ``float(b0), float(b1), float(b2) - float(b0), float(b3) - float(b1)``) are
    counted in one warning and evaluated as rounded.  A row of an unknown image or category takes no part."""
    rows = path_or_list
    if not isinstance(rows, list):
        with open(rows) as f:
            rows = json.load(f)
    n = len(rows)
    box = np.array([r['bbox'] for r in rows], dtype=np.float64).reshape(n, 4)
    score = np.array([r['score'] for r in rows], dtype=np.float64).reshape(n)
    x, y, w, h = box.T
    dets = np.stack([x, y, x + w, y + h, score], axis=1).astype(np.float32)
    back = dets.astype(np.float64)
    ok = ((back[:, 0] == x) & (back[:, 1] == y) & (back[:, 2] - back[:, 0] == w) & (back[:, 3] - back[:, 1] == h)
          & (back[:, 4] == score))
    if not ok.all():
        warnings.warn(f'{int((~ok).sum())} of {n} json rows are not float32 x1 y1 x2 y2 score rows written as x y w h: '
                      'they are evaluated as rounded to float32')

    def index(ids, key):
        ids = np.asarray(list(ids), np.int64)
        order = np.argsort(ids, kind='stable')
        pos = _position(ids[order], np.array([r[key] for r in rows], dtype=np.int64))
        return np.where(pos >= 0, order[np.maximum(pos, 0)], -1).astype(np.int64) if len(ids) else pos
    return dets, index(cat_ids, 'category_id'), index(img_ids, 'image_id')


def load_results(results, cat_ids, img_ids):
    """Per-image per-class lists, the flat tuple, the path of a ``.pkl`` (either of the two) or of a bbox ``.json`` ->
    the flat form (numpy arrays, or GPU tensors when they were given)."""
    if isinstance(results, (str, bytes)) or hasattr(results, '__fspath__'):
        path = str(results)
        if path.endswith('.json'):
            return read_json_results(path, cat_ids, img_ids)
        if not path.endswith(('.pkl', '.pickle')):
            raise ValueError(f'{path}: a result file is a .pkl (the test loop\'s) or a bbox .json (results2json\'s)')
        with open(path, 'rb') as f:
            results = pickle.load(f)
    if _is_flat(results):
        return results
    return flatten_results(results)


class ErrorAnalysis:
    """The result of ``error_analysis``: ``ps`` (7, R, K, A, 1) float64 as the tool's, ``rec_thrs`` (R), ``cat_ids`` (K,
    sorted), ``names`` (K), ``counts`` (K, A) the ground truths that count, ``area_rng`` (A, 2), ``iou_thrs``,
    ``conf_thr``, ``phases`` (seconds per phase when ``timing=True``; ``*_dev``: between device events)."""

    def __init__(self, ps, rec_thrs, cat_ids, names, counts, area_rng, iou_thrs, conf_thr, phases, state):
        self.ps, self.rec_thrs, self.cat_ids, self.names, self.counts = ps, rec_thrs, cat_ids, names, counts
        self.area_rng, self.iou_thrs, self.conf_thr, self.phases = area_rng, iou_thrs, conf_thr, phases
        self._state = state

    def det_bits(self):
        """As ``COCOeval.det_bits``, with ``T + 2`` on the threshold axis (``T``: Sim, ``T + 1``: Oth): for the
        detections that take part, in (problem, rank) order, ``index``, ``problem``, ``rank`` and the ``matched`` /
        ``ignored`` bits (A, T + 2, n)."""
        s = self._state
        D, A, TW = s['D'], s['A'], s['TW']
        det_off = s['det_off'].cpu().numpy()
        n = int(det_off[-1])
        order, sprob = s['order'].cpu().numpy()[:n].astype(np.int64), s['sprob'].cpu().numpy()[:n].astype(np.int64)
        rank = np.arange(n, dtype=np.int64) - det_off[sprob]
        keep = rank < s['max_det']
        f = s['flags'].cpu().numpy()[:D * A * TW].reshape(D, A, TW)[:n][keep].transpose(1, 2, 0)
        return dict(index=order[keep], problem=sprob[keep], rank=rank[keep], matched=(f & 1) != 0, ignored=(f & 2) != 0)

    def aps(self, k=None):
        """(7, A): the numbers in the legends of the tool's figures, ``ps[type, :, k, a, 0].mean()`` for class ``k`` (a
        K-axis position) or, ``k=None``, "allclass": the mean over R and K."""
        ps = self.ps if k is None else self.ps[:, :, k]
        return np.array([[ps_.mean() for ps_ in ps[..., a, 0]] for a in range(ps.shape[-2])], dtype=np.float64).T

    def table(self, k=None):
        """The (7, A) numbers as a plain-text table (this package's own form)."""
        aps = self.aps(k)
        A = aps.shape[1]
        head = [AREA_NAMES[a] if A == len(AREA_NAMES) else f'area{a}' for a in range(A)]
        title = 'allclass' if k is None else str(self.names[k])
        types = [f'C{int(round(t * 100))}' for t in self.iou_thrs[:-1]] + list(TYPES[2:])
        lines = [f'bbox-{title}', 'type  ' + ' '.join(f'{h:>8}' for h in head)]
        lines += [f'{types[i]:<5} ' + ' '.join(f'{v:8.3f}' for v in aps[i]) for i in range(len(types))]
        return '\n'.join(lines)


def stack_ps(precision):
    """Step 4 of the definition on ``precision (T + 2, R, K, A, M)`` (base rows, Sim, Oth) -> ``ps (T + 4, R, K, A, M)``."""
    n = precision.shape[0]
    ps = np.vstack([precision, np.zeros((2, *precision.shape[1:]))])
    ps[ps == -1] = 0
    ps[n] = ps[n - 1] > 0
    ps[n + 1] = 1.0
    return ps


def error_analysis(coco_gt, results, cat_ids=None, img_ids=None, areas=None, iou_thrs=(0.75, 0.5, 0.1), conf_thr=0.1,
                   max_det=100, timing=False, iou_type='bbox'):
    """The tool's analysis of ``results`` against ``coco_gt`` (a ``CocoGt``, a parsed annotation dict or a path) ->
    ``ErrorAnalysis``.  ``results``: per-image per-class lists (images in ``img_ids`` order), the flat tuple ``(dets (D,
    5), labels (D,), img_index (D,))`` of numpy arrays or GPU tensors (which never visit the host), the path of a ``.pkl``
    of either, or the path of a bbox ``.json``.  ``cat_ids[label]`` is a detection's category id and
    ``img_ids[img_index]`` its image id (defaults: the annotation file's order).  ``areas``: the tool's ``--areas``.
    The reference's figures need ``iou_thrs`` of three entries (C75, C50, Loc); any ``T >= 1`` gives ``ps`` of ``T + 4``
    rows with Sim, Oth, BG and FN last."""
    if iou_type != 'bbox':
        raise NotImplementedError(f"iou_type={iou_type!r} is not built: no detector of this package produces masks; only "
                                  "iou_type='bbox' is")
    if not isinstance(coco_gt, CocoGt):
        coco_gt = CocoGt(coco_gt)
    cat_ids = list(coco_gt.get_cat_ids() if cat_ids is None else cat_ids)
    img_ids = list(coco_gt.get_img_ids() if img_ids is None else img_ids)
    phases = {} if timing else None
    t0 = time.perf_counter()
    tab = tables(coco_gt, cat_ids, img_ids)
    flat = load_results(results, cat_ids, img_ids)
    thrs = np.ascontiguousarray(iou_thrs, dtype=np.float64).reshape(-1)
    area = area_ranges(areas)
    rec = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    T, A, R = len(thrs), len(area), len(rec)
    max_det = int(max_det)
    if T == 0 or max_det <= 0:
        raise ValueError('iou_thrs must not be empty and max_det must be positive')
    if timing:
        phases['table_build'] = time.perf_counter() - t0

    dev = _eval_common._device('coco_error', 'coco_eval')
    lib = _lib.lib()
    timer = _eval_common.PhaseTimer(phases, dev)
    K, P, N = tab['K'], tab['P'], tab['N']
    TW = T + 2
    dets, labels, img_index = _flat_to_device(flat, dev)
    D = int(dets.shape[0])
    kmap, imap = _dev(tab['kmap'], np.int64, dev), _dev(tab['imap'], np.int64, dev)
    ok = (labels >= 0) & (labels < len(kmap)) & (img_index >= 0) & (img_index < len(imap))
    k = kmap[labels.clamp(0, len(kmap) - 1)]
    i = imap[img_index.clamp(0, len(imap) - 1)]
    prob = torch.where(ok & (k >= 0) & (i >= 0), i * K + k, torch.full_like(k, -1)).to(torch.int32)
    G = len(tab['gt_area'])
    gt_box, gt_area = _dev(tab['gt_box'].reshape(-1), np.float64, dev), _dev(tab['gt_area'], np.float64, dev)
    gt_flag, gt_cat = _dev(tab['gt_flag'], np.uint8, dev), _dev(tab['gt_cat'], np.int32, dev)
    gt_img_off, cat_group = _dev(tab['gt_img_off'], np.int64, dev), _dev(tab['cat_group'], np.int32, dev)
    t_thr, t_area, t_rec = _dev(thrs, np.float64, dev), _dev(area.reshape(-1), np.float64, dev), _dev(rec, np.float64, dev)
    # (yv4_coco_rank sizes yv4_coco_match's workspace from a per-problem gt table; this path sizes its own below)
    no_gt = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    timer.mark('upload')

    events = []

    def device_phase(key, fn):
        if timing:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events.append((key, e0, e1))
        else:
            fn()
    n1 = max(D, 1)
    order = torch.empty(n1, dtype=torch.int32, device=dev)
    sprob = torch.empty(n1, dtype=torch.int32, device=dev)
    det_off = torch.empty(P + 1, dtype=torch.int64, device=dev)
    need = torch.zeros(2, dtype=torch.int64, device=dev)
    rwork = torch.empty(int(lib.yv4_coco_rank_work(D)) // 8 + 1, dtype=torch.int64, device=dev)

    def ordering():
        check(lib.yv4_coco_rank(_ptr(dets), prob.data_ptr() if D else None, D, P, max_det, A * TW, no_gt.data_ptr(),
                                rwork.data_ptr(), order.data_ptr(), sprob.data_ptr(), det_off.data_ptr(),
                                need[:1].data_ptr(), stream_ptr()), 'yv4_coco_rank')
        check(lib.yv4_coco_error_need(det_off.data_ptr(), gt_img_off.data_ptr(), P, K, max_det, A * TW,
                                      need[1:].data_ptr(), stream_ptr()), 'yv4_coco_error_need')
    device_phase('ordering', ordering)
    need = int(need.cpu()[1])                                # the one read-back between the device calls
    timer.mark('ordering')
    del rwork
    mwork = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    flags = torch.empty(n1 * A * TW, dtype=torch.uint8, device=dev)
    counts = torch.empty(K * A, dtype=torch.int32, device=dev)
    device_phase('matching', lambda: check(lib.yv4_coco_error_match(
        _ptr(dets), order.data_ptr(), det_off.data_ptr(), _ptr(gt_box), _ptr(gt_area), _ptr(gt_flag), _ptr(gt_cat),
        gt_img_off.data_ptr(), cat_group.data_ptr(), P, K, D, G, max_det, t_thr.data_ptr(), T, float(conf_thr),
        t_area.data_ptr(), A, mwork.data_ptr(), need, state.data_ptr(), flags.data_ptr(), counts.data_ptr(),
        stream_ptr()), 'yv4_coco_error_match'))
    timer.mark('matching')
    md = np.array([max_det], dtype=np.int32)
    awork = torch.empty(int(lib.yv4_coco_accumulate_work(D, K, A * TW)) // 8 + 1, dtype=torch.int64, device=dev)
    precision = torch.empty((TW, R, K, A, 1), dtype=torch.float64, device=dev)
    scores = torch.empty((TW, R, K, A, 1), dtype=torch.float64, device=dev)
    recall = torch.empty((TW, K, A, 1), dtype=torch.float64, device=dev)
    device_phase('accumulation', lambda: check(lib.yv4_coco_accumulate(
        _ptr(dets), order.data_ptr(), sprob.data_ptr(), det_off.data_ptr(), flags.data_ptr(), counts.data_ptr(), P, K, D,
        md.ctypes.data, 1, TW, A, t_rec.data_ptr(), R, awork.data_ptr(), precision.data_ptr(), recall.data_ptr(),
        scores.data_ptr(), stream_ptr()), 'yv4_coco_accumulate'))
    timer.mark('accumulation')
    if int(state.cpu()[1]):
        raise RuntimeError('yv4_coco_error_match ran out of workspace (internal error: the size came from '
                           'yv4_coco_error_need)')
    precision_h = precision.cpu().numpy()
    counts_h = counts.cpu().numpy().reshape(K, A).astype(np.int64)
    timer.mark('download')
    ps = stack_ps(precision_h)
    names = [str(coco_gt.cats[int(c)].get('name', int(c))) if int(c) in coco_gt.cats else str(int(c)) for c in tab['cat_ids']]
    if timing:
        phases['post'] = time.perf_counter() - timer.last
        for key, e0, e1 in events:
            phases[key + '_dev'] = e0.elapsed_time(e1) * 1e-3
    return ErrorAnalysis(ps, rec, [int(c) for c in tab['cat_ids']], names, counts_h, area, thrs, float(conf_thr), phases,
                         dict(D=D, A=A, TW=TW, max_det=max_det, order=order, sprob=sprob, det_off=det_off, flags=flags,
                              workspace=need, tab=tab))
