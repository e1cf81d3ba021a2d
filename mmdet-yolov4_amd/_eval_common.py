"""Host helpers shared by the evaluation modules (``coco_eval``, ``map_eval``, ``eval_utils``): the upload and offset
helpers, the device / library check, the logger, the per-phase timer, and ``rank_flat``, the common start of the two
flat-table paths (``map_flat_device``, ``flex_flat_device``)."""
import logging
import time

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import stream_ptr


def _device(what, feature=None):
    """The current GPU; raises without one, or when the loaded library lacks ``feature`` (``_lib.FEATURES``)."""
    if not torch.cuda.is_available():
        raise RuntimeError(f'{what} runs on the GPU through libyv4_hip.so; no GPU is visible '
                           '(there is no CPU fallback for this path)')
    if feature is not None:
        _lib.require(feature)
    return torch.device('cuda', torch.cuda.current_device())


def _dev(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev, non_blocking=False)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def _is_flat(results):
    return isinstance(results, tuple) and len(results) == 3 and not isinstance(results[0], (list, tuple))


def _log(msg, logger, level=logging.INFO):
    if logger is None:
        print(msg)
    elif isinstance(logger, logging.Logger):
        logger.log(level, msg)
    elif logger != 'silent':
        logging.getLogger(logger).log(level, msg)


class PhaseTimer:
    """Seconds per phase into the dict ``phases``: ``mark(key)`` closes a phase with a device synchronise.  Does nothing
    when ``phases is None``."""

    def __init__(self, phases, dev):
        self.phases, self.dev = phases, dev
        self.last = self._now()

    def _now(self):
        if self.phases is None:
            return 0
        torch.cuda.synchronize(self.dev)
        return time.perf_counter()

    def mark(self, key):
        if self.phases is not None:
            now = self._now()
            self.phases[key] = now - self.last
            self.last = now


def _flat_to_device(flat, dev):
    dets, labels, img_index = flat

    def put(x, np_dtype, t_dtype):
        if isinstance(x, torch.Tensor):
            return x.to(dev, t_dtype).contiguous()
        return _dev(np.asarray(x), np_dtype, dev)
    dets = put(dets, np.float32, torch.float32).reshape(-1, 5)
    labels, img_index = put(labels, np.int64, torch.int64).reshape(-1), put(img_index, np.int64, torch.int64).reshape(-1)
    if labels.numel() != dets.shape[0] or img_index.numel() != dets.shape[0]:
        raise ValueError(f'flat results: {dets.shape[0]} detections, {labels.numel()} labels, {img_index.numel()} image indices')
    return dets, labels, img_index


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def rank_flat(flat, gt_off, N, C, dev):
    """``yv4_map_rank`` over the flat table ``(dets, labels, img_index)`` already on ``dev`` (``_flat_to_device``) and the
    one read-back between the device calls.  ``gt_off``: the device table of the P = N * C problems' gts.  Returns the
    device tensors det4 (D, 4), det_off / iou_off (P + 1), order / rank / cls_order (D), and from the host the pair
    total, the number of detections inside a problem and the per-class counts (each below 2**24, or it raises)."""
    dets, labels, img_index = flat
    D, P = int(dets.shape[0]), N * C
    lib = _lib.lib()
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)            # noqa: E731
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)            # noqa: E731
    det4 = torch.empty((max(D, 1), 4), dtype=torch.float32, device=dev)
    det_off, iou_off, info = i64(P + 1), i64(P + 1), i64(C + 2)
    order, rank, cls_order = i32(max(D, 1)), i32(max(D, 1)), i32(max(D, 1))
    work = torch.empty(max(int(lib.yv4_map_rank_work(D)), 8), dtype=torch.uint8, device=dev)
    check(lib.yv4_map_rank(_ptr(dets), _ptr(labels), _ptr(img_index), D, N, C, gt_off.data_ptr(), work.data_ptr(),
                           det4.data_ptr(), det_off.data_ptr(), order.data_ptr(), rank.data_ptr(), iou_off.data_ptr(),
                           cls_order.data_ptr(), info.data_ptr(), stream_ptr()), 'yv4_map_rank')
    info_h = info.cpu().numpy()                                 # the one read-back between the device calls
    pairs, Dv, counts = int(info_h[0]), int(info_h[1]), info_h[2:]
    for c in np.flatnonzero(counts >= 2 ** 24):
        raise ValueError(f'class {c} has {counts[c]} detections: the cumulative counts are kept exact only below 2**24')
    return det4, det_off, iou_off, order, rank, cls_order, pairs, Dv, counts
