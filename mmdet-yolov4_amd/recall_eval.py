"""Proposal recall: ``eval_recalls`` / ``set_recall_param`` / ``print_recall_summary`` under the reference's names
(``mmdet/core/evaluation/recall.py``), scored on the GPU by ONE ``yv4_recall_match`` launch over every (image, proposal
number) pair (csrc/recall.hip).  It answers "do the detector's boxes find the objects at all, whatever class they give
them": a detector's results are scored with their labels dropped.

Definition (restated in plain numpy in tests/_recall_ref.py, held there against what the reference produced):

* Ordering.  An ``(n, 5)`` array is visited by descending score, STABLE: equal scores (``+0`` and ``-0`` are equal) keep
  the input order -- the package's rule everywhere, and the one stated difference from the reference, whose
  ``np.argsort(scores)[::-1]`` is an unstable sort, reversed.  An ``(n, 4)`` array keeps its order.  Scores and boxes are
  expected finite.  The flat form is ordered by ``yv4_map_rank`` (one class, a zero label column), unchanged.
* Per image ``cols = min(n, proposal_nums[-1])`` -- the LAST entry, not the maximum, as ``recall.py:96`` has it -- and
  the IoU block is ``bbox_overlaps(gts, proposals[:cols, :4])``: fp32, the reference's operation order, ``eps = 1e-6``.
* Per proposal number ``pn`` and image, on the block's first ``min(cols, pn)`` columns, the ``G`` steps of
  ``recall.py:24-31``: every row's maximum with its first-occurrence argmax, the first row holding the largest maximum,
  that value recorded, its row and column set to -1.  More gts than columns: the surplus steps record -1.  Gts and no
  columns: ``G`` zeros.  No gts: nothing.
* ``counts[k, t]`` = the recorded float32 values of proposal number k that, widened, reach the float64 threshold t;
  ``recalls = counts / float(total_gt)`` in numpy on the host (zero gts: ``nan`` and numpy's warning, as the reference).

Inputs beyond the reference's per-image ``(n, 4)`` / ``(n, 5)`` arrays: the detector's result form (per image a
per-class list, concatenated in class order -- the reference raises ``AttributeError`` on it) and the flat tuple
``(dets (D, 5), labels (D,), img_index (D,))`` of numpy arrays or GPU tensors (labels are ignored; GPU tensors never
visit the host).  Images of unequal shapes are fine: nothing here depends on ``np.array`` of a ragged list, which
numpy 2 refuses in the reference.  There is no CPU implementation: without a GPU the calls raise.
``plot_num_recall`` / ``plot_iou_recall`` are not built.
"""
from collections.abc import Sequence

import numpy as np
import torch

from . import _eval_common, _lib
from ._eval_common import PhaseTimer, _dev, _flat_to_device, _is_flat, _log, _offsets, _ptr
from ._lib import check
from .ops import stream_ptr

_EPS = float(np.float32(1e-6))


def _device():
    return _eval_common._device('recall_eval', 'recall')


def set_recall_param(proposal_nums, iou_thrs):
    """recall.py:43: check ``proposal_nums`` and ``iou_thrs`` and bring them into array form."""
    if isinstance(proposal_nums, Sequence):
        _proposal_nums = np.array(proposal_nums)
    elif isinstance(proposal_nums, int):
        _proposal_nums = np.array([proposal_nums])
    else:
        _proposal_nums = proposal_nums
    if iou_thrs is None:
        _iou_thrs = np.array([0.5])
    elif isinstance(iou_thrs, Sequence):
        _iou_thrs = np.array(iou_thrs)
    elif isinstance(iou_thrs, float):
        _iou_thrs = np.array([iou_thrs])
    else:
        _iou_thrs = iou_thrs
    return _proposal_nums, _iou_thrs


class RecallGt:
    """The ground truth of a dataset as one flat table, built once: ``gt`` (G, 4) float32 image-major, ``gt_off``
    (N + 1,) int64, ``ng`` (N,); the device copies are kept per device, as ``MapGt`` keeps its.  ``gts``: per image a
    ``(g, 4)`` array, or ``None`` for an image without gts."""

    def __init__(self, gts):
        self.num_imgs = len(gts)
        parts = [np.zeros((0, 4), np.float32)]
        ng = np.zeros(self.num_imgs, np.int64)
        for i, g in enumerate(gts):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float32)
            if g.size == 0:
                continue
            if g.ndim != 2 or g.shape[1] < 4:
                raise ValueError(f'gts[{i}] has shape {g.shape}, (g, 4) is expected')
            parts.append(g[:, :4])
            ng[i] = len(g)
        self.gt = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32).reshape(-1, 4)
        self.ng = ng
        self.gt_off = _offsets(ng)
        self._device = {}

    @property
    def total_gt(self):
        return int(self.gt.shape[0])

    def device(self, dev):
        d = self._device.setdefault((dev.type, dev.index), {})
        if 'gt' not in d:
            d.update(gt=_dev(self.gt, np.float32, dev), gt_off=_dev(self.gt_off, np.int64, dev))
        return d


def _params(proposal_nums, iou_thrs):
    nums = np.asarray(proposal_nums).reshape(-1)
    thrs = np.ascontiguousarray(np.asarray(iou_thrs).reshape(-1), dtype=np.float64)
    if len(nums) == 0 or len(nums) > _lib.RECALL_MAX_NUMS:
        raise ValueError(f'{len(nums)} proposal numbers: 1 .. {_lib.RECALL_MAX_NUMS} are taken')
    if len(thrs) == 0 or len(thrs) > _lib.RECALL_MAX_THRS:
        raise ValueError(f'{len(thrs)} IoU thresholds: 1 .. {_lib.RECALL_MAX_THRS} are taken')
    if (nums < 0).any():
        raise ValueError(f'proposal numbers must not be negative, got {nums.tolist()}')
    return np.ascontiguousarray(nums, dtype=np.int32), thrs


def _match(det4, det_off, total_det, gt, dev, nums, thrs, return_ious, lds_cap, timer):
    """``yv4_recall_match`` on device tables and the one read-back.  Returns (recalls (M, T) float64, gt_ious or None)."""
    N, G, M, T = gt.num_imgs, gt.total_gt, len(nums), len(thrs)
    if N == 0 or G == 0:                                    # nothing records a value: 0 / 0.0 below
        counts = np.zeros((M, T), np.int64)
        ious = np.zeros((M, 0), np.float32) if return_ious else None
    else:
        g = gt.device(dev)
        lib = _lib.lib()
        t_thr = _dev(thrs, np.float64, dev)
        need = int(lib.yv4_recall_work(total_det, G, N, M))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        t_counts = torch.empty((M, T), dtype=torch.int64, device=dev)
        t_ious = torch.empty((M, G), dtype=torch.float32, device=dev) if return_ious else None
        check(lib.yv4_recall_match(_ptr(det4), det_off.data_ptr(), g['gt'].data_ptr(), g['gt_off'].data_ptr(), N + 1, N,
                                   total_det, G, nums.ctypes.data, M, t_thr.data_ptr(), T, _EPS, int(lds_cap),
                                   work.data_ptr(), need, _ptr(t_ious), M * G, t_counts.data_ptr(), M * T, stream_ptr()),
              'yv4_recall_match')
        timer.mark('match')
        counts = t_counts.cpu().numpy()                     # the one read-back
        ious = t_ious.cpu().numpy() if return_ious else None
        timer.mark('download')
    return counts / float(G), ious


def recall_device(flat, gt, proposal_nums, iou_thrs, phases=None, return_ious=False, lds_cap=0):
    """The device path: ``yv4_map_rank`` (one class) orders the flat table ``(dets (D, 5), labels, img_index)`` -- numpy
    arrays or GPU tensors, labels ignored, a row whose image index is outside ``[0, N)`` takes no part -- then ONE
    ``yv4_recall_match`` launch, then one read-back of the ``(M, T)`` counts (plus ``gt_ious`` on request).  ``gt``: a
    ``RecallGt``.  Returns the ``(M, T)`` float64 recalls, or ``(recalls, gt_ious (M, total_gt) float32)`` whose row k
    holds, image by image, the values the G steps recorded (unsorted: the reference sorts them, which changes no
    count).  ``phases``: an optional dict that receives seconds per phase (each closed by a synchronise).  ``lds_cap``:
    ``yv4_recall_match``'s (0: the built-in cap; both forms give the same bytes)."""
    dev = _device()
    nums, thrs = _params(proposal_nums, iou_thrs)
    timer = PhaseTimer(phases, dev)
    N = gt.num_imgs
    dets, _, img_index = _flat_to_device(flat, dev)
    D = int(dets.shape[0])
    det4 = det_off = None
    if N > 0 and gt.total_gt > 0:
        g = gt.device(dev)
        timer.mark('upload')
        lib = _lib.lib()
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)            # noqa: E731
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)            # noqa: E731
        labels = torch.zeros(max(D, 1), dtype=torch.int64, device=dev)
        det4 = torch.empty((max(D, 1), 4), dtype=torch.float32, device=dev)
        det_off, iou_off, info = i64(N + 1), i64(N + 1), i64(3)
        order, rank, cls_order = i32(max(D, 1)), i32(max(D, 1)), i32(max(D, 1))
        work = torch.empty(max(int(lib.yv4_map_rank_work(D)), 8), dtype=torch.uint8, device=dev)
        check(lib.yv4_map_rank(_ptr(dets), labels.data_ptr() if D else None, _ptr(img_index), D, N, 1, g['gt_off'].data_ptr(),
                               work.data_ptr(), det4.data_ptr(), det_off.data_ptr(), order.data_ptr(), rank.data_ptr(),
                               iou_off.data_ptr(), cls_order.data_ptr(), info.data_ptr(), stream_ptr()), 'yv4_map_rank')
        timer.mark('rank')
    recalls, ious = _match(det4, det_off, D, gt, dev, nums, thrs, return_ious, lds_cap, timer)
    return (recalls, ious) if return_ious else recalls


def _recall_tables(gt, det4, nd, proposal_nums, iou_thrs, return_ious=False, lds_cap=0):
    """Boxes already in visiting order on the host (``det4`` (D, 4) image-major, ``nd`` per image): the two tables are
    built here and uploaded; then the same ``yv4_recall_match``."""
    dev = _device()
    nums, thrs = _params(proposal_nums, iou_thrs)
    timer = PhaseTimer(None, dev)
    t4 = t_off = None
    if gt.num_imgs > 0 and gt.total_gt > 0:
        t4 = _dev(det4.reshape(-1, 4) if len(det4) else np.zeros((1, 4), np.float32), np.float32, dev)
        t_off = _dev(_offsets(nd), np.int64, dev)
    recalls, ious = _match(t4, t_off, int(len(det4)), gt, dev, nums, thrs, return_ious, lds_cap, timer)
    return (recalls, ious) if return_ious else recalls


def _as_recall_gt(gts):
    return gts if isinstance(gts, RecallGt) else RecallGt(gts)


def _image_array(p, i):
    """One image's proposals as a 2-D float32 array of 4 or 5 columns; a per-class list is concatenated in class order."""
    if isinstance(p, (list, tuple)):
        parts = [np.asarray(c, dtype=np.float32) for c in p]
        parts = [c for c in parts if c.size]
        p = np.concatenate(parts, axis=0) if parts else np.zeros((0, 5), np.float32)
    p = np.asarray(p, dtype=np.float32)
    if p.size == 0:
        return np.zeros((0, 4), np.float32)
    if p.ndim != 2 or p.shape[1] not in (4, 5):
        raise ValueError(f'proposals[{i}] has shape {p.shape}, (n, 4) or (n, 5) is expected')
    return p


def _score(gt, proposals, proposal_nums, iou_thrs, return_ious=False, lds_cap=0):
    if _is_flat(proposals):
        return recall_device(proposals, gt, proposal_nums, iou_thrs, return_ious=return_ious, lds_cap=lds_cap)
    if len(proposals) != gt.num_imgs:
        raise AssertionError(f'{gt.num_imgs} images of gts, {len(proposals)} of proposals')
    imgs = [_image_array(p, i) for i, p in enumerate(proposals)]
    nd = np.fromiter((len(p) for p in imgs), np.int64, len(imgs))
    if all(p.shape[1] == 5 for p in imgs if len(p)):       # every image scored: the device orders them
        dets = np.concatenate([np.zeros((0, 5), np.float32)] + [p for p in imgs if len(p)], axis=0)
        idx = np.repeat(np.arange(len(imgs), dtype=np.int64), nd)
        return recall_device((dets, np.zeros(len(dets), np.int64), idx), gt, proposal_nums, iou_thrs,
                             return_ious=return_ious, lds_cap=lds_cap)
    # (n, 4) images keep their order; an (n, 5) image among them is ordered here by the same stable rule
    imgs = [p[np.argsort(-p[:, 4], kind='stable'), :4] if p.shape[1] == 5 else p for p in imgs]
    det4 = np.concatenate([np.zeros((0, 4), np.float32)] + imgs, axis=0)
    return _recall_tables(gt, det4, nd, proposal_nums, iou_thrs, return_ious=return_ious, lds_cap=lds_cap)


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=0.5, logger=None):
    """recall.py:64: the ``(M, T)`` float64 recalls of ``M`` proposal numbers and ``T`` IoU thresholds, and the summary.

    ``gts``: per image a ``(g, 4)`` array (``None`` for none), or a ``RecallGt``.  ``proposals``: per image an ``(n, 4)``
    or ``(n, 5)`` array; per image a per-class list of such arrays (a detector's results); or the flat tuple ``(dets
    (D, 5), labels (D,), img_index (D,))`` of numpy arrays or GPU tensors (see the module docstring)."""
    gt = _as_recall_gt(gts)
    proposal_nums, iou_thrs = set_recall_param(proposal_nums, iou_thrs)
    recalls = _score(gt, proposals, proposal_nums, iou_thrs)
    print_recall_summary(recalls, proposal_nums, iou_thrs, logger=logger)
    return recalls


# ---- the summary table (the project's own text; terminaltables is not used and no parity is claimed) -----------------
def print_recall_summary(recalls, proposal_nums, iou_thrs, row_idxs=None, col_idxs=None, logger=None):
    """Recalls, three decimals, one row per proposal number and one column per IoU threshold; ``row_idxs`` /
    ``col_idxs`` select rows and columns.  ``logger='silent'`` prints nothing."""
    if logger == 'silent':
        return
    proposal_nums = np.array(proposal_nums, dtype=np.int32).reshape(-1)
    iou_thrs = np.array(iou_thrs).reshape(-1)
    recalls = np.asarray(recalls)
    if row_idxs is None:
        row_idxs = np.arange(proposal_nums.size)
    if col_idxs is None:
        col_idxs = np.arange(iou_thrs.size)
    rows = [[''] + [str(v) for v in iou_thrs[col_idxs].tolist()]]
    for i, num in enumerate(proposal_nums[row_idxs]):
        rows.append([str(num)] + [f'{val:.3f}' for val in recalls[row_idxs[i], col_idxs].tolist()])
    width = [max(len(r[j]) for r in rows) for j in range(len(rows[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    lines = [rule]
    for n, r in enumerate(rows):
        lines.append('| ' + ' | '.join(c.ljust(w) for c, w in zip(r, width)) + ' |')
        if n == 0:
            lines.append(rule)
    lines.append(rule)
    _log('\n' + '\n'.join(lines), logger)
