"""The flat result table of a test loop, kept on the GPU, and the dataset object an evaluation hook scores it against.

The reference's test loop returns, per image, a per-class list of numpy arrays (``bbox2result``,
``mmdet/apis/test.py:16-68``): every batch's ``(N, max_per_img, 5)`` block is downloaded, cut into ``N x num_classes``
arrays, and ``CocoDataset.evaluate`` walks them again (``_det2json``, ``datasets/coco.py:179-199``).  ``COCOeval`` of this
package takes the flat form ``(dets (D, 5), labels (D,), img_index (D,))`` as GPU tensors; ``DeviceResults`` produces
it: ``yv4_results_append`` (csrc/results.hip) copies a batch's rows from the plan's own buffers into the table in
``_det2json`` order -- image, class, the row order NMS left -- so the table equals
``flatten_results([bbox2result(...)])`` bit for bit and nothing but the ``(N,)`` counts visits the host.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._eval_common import _log
from ._lib import check
from .coco_eval import CocoGt, evaluate_bbox, flatten_results
from .eval_utils import FAST_BBOX_SCALE_RANGES, FlexGt, coco_test_annotation, evaluate_fast_bbox
from .map_eval import MapGt, evaluate_map
from .ops import stream_ptr
from .recall_eval import RecallGt, eval_recalls


def _host_index(img_index, n):
    idx = np.asarray(img_index, dtype=np.int64).reshape(-1)
    if idx.shape[0] != n:
        raise ValueError(f'img_index holds {idx.shape[0]} positions for {n} images')
    return idx


class DeviceResults:
    """``(dets (D, 5) float32, labels (D,) int64, img_index (D,) int64)`` on ``device``, grown geometrically; the cursor
    ``D`` lives on the host (it is the sum of counts the test loop reads back anyway).  ``num_images`` counts the images
    appended so far: the default position of the next batch's images."""

    def __init__(self, num_classes, device, capacity=4096):
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        if self.num_classes <= 0:
            raise ValueError('num_classes must be positive')
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceResults lives on the GPU (yv4_results_append); there is no CPU fallback for this path')
        _lib.require('results_append')
        self.D = 0
        self.num_images = 0
        self._alloc(max(int(capacity), 1))

    def _alloc(self, capacity):
        self.capacity = capacity
        self.dets = torch.empty((capacity, 5), dtype=torch.float32, device=self.device)
        self.labels = torch.empty((capacity,), dtype=torch.int64, device=self.device)
        self.img_index = torch.empty((capacity,), dtype=torch.int64, device=self.device)

    def _reserve(self, rows):
        need = self.D + rows
        if need <= self.capacity:
            return
        old = (self.dets, self.labels, self.img_index)
        self._alloc(max(need, 2 * self.capacity))
        for new, prev in zip((self.dets, self.labels, self.img_index), old):
            new[:self.D].copy_(prev[:self.D])

    def next_positions(self, n):
        return np.arange(self.num_images, self.num_images + n, dtype=np.int64)

    def append(self, post, img_index=None, counts=None):
        """One batch from a plan's post-processing buffers (``Plan.postprocess``: ``dets``, ``labels``, ``count``).
        ``img_index``: the N dataset positions (default: the next N), -1 skips an image.  ``counts``: the host copy of
        ``post['count']`` when the caller has it already; every count must be final (the split path has run).  The
        counts are checked here; the labels are the plan's own (its NMS writes class indices below ``num_classes``) and
        are trusted: they stay on the device, and reading them back to check would be the detour this class removes."""
        N, M = int(post['N']), int(post['max_per_img'])
        idx = self.next_positions(N) if img_index is None else _host_index(img_index, N)
        counts = (post['count'].cpu() if counts is None else counts).numpy().astype(np.int64).reshape(-1)
        if counts.shape[0] != N or (counts < 0).any() or (counts > M).any():
            raise ValueError(f'counts must be {N} values in [0, {M}] (run the split path first), got {counts.tolist()}')
        if M > _lib.RESULTS_MAX_PER_IMG:
            raise NotImplementedError(f'max_per_img={M}: yv4_results_append holds at most {_lib.RESULTS_MAX_PER_IMG} '
                                      'rows per image')
        total = int(counts[idx >= 0].sum())
        self._reserve(total)
        dets, labels, count = post['dets'], post['labels'], post['count']
        assert dets.dtype == torch.float32 and labels.dtype == torch.int32 and count.dtype == torch.int32
        assert dets.is_contiguous() and labels.is_contiguous() and tuple(dets.shape) == (N, M, 5)
        from .yolocsp_head import _upload
        idx_dev = _upload(torch.from_numpy(idx), self.device)
        check(_lib.lib().yv4_results_append(dets.data_ptr(), labels.data_ptr(), count.data_ptr(), idx_dev.data_ptr(), N, M,
                                            self.num_classes, self.D, self.capacity, self.dets.data_ptr(),
                                            self.labels.data_ptr(), self.img_index.data_ptr(), stream_ptr()),
              'yv4_results_append')
        self.D += total
        self.num_images += N
        return total

    def append_lists(self, results, img_index=None):
        """Images in the reference's form (per image a per-class list of (n, 5) arrays: what ``aug_test`` returns):
        one ``flatten_results``, one upload."""
        n = len(results)
        idx = self.next_positions(n) if img_index is None else _host_index(img_index, n)
        if n and len(results[0]) != self.num_classes:
            raise ValueError(f'results hold {len(results[0])} class lists, the table {self.num_classes}')
        dets, labels, local = flatten_results(results)
        pos = idx[local]
        keep = pos >= 0
        if not keep.all():
            dets, labels, pos = dets[keep], labels[keep], pos[keep]
        rows = int(dets.shape[0])
        self._reserve(rows)
        if rows:
            from .yolocsp_head import _upload
            lo, hi = self.D, self.D + rows
            self.dets[lo:hi].copy_(_upload(torch.from_numpy(np.ascontiguousarray(dets)), self.device))
            self.labels[lo:hi].copy_(_upload(torch.from_numpy(np.ascontiguousarray(labels)), self.device))
            self.img_index[lo:hi].copy_(_upload(torch.from_numpy(np.ascontiguousarray(pos)), self.device))
        self.D += rows
        self.num_images += n
        return rows

    def tensors(self):
        return self.dets[:self.D], self.labels[:self.D], self.img_index[:self.D]


class CocoBBoxDataset:
    """The ``.dataset`` a validation loader carries: the annotation file and ``evaluate``.  It loads no images (the
    loader yields them).  ``accepts_flat``: ``evaluate`` takes the flat GPU table as well as the list form, which is
    what makes an evaluation hook choose the flat test loop.  ``classes`` selects the categories by name as
    ``CocoDataset.load_annotations`` does (``datasets/coco.py:57-77``)."""

    accepts_flat = True

    def __init__(self, ann_file, classes=None):
        self.coco = ann_file if isinstance(ann_file, CocoGt) else CocoGt(ann_file)
        self.CLASSES = tuple(classes) if classes is not None else tuple(c['name'] for c in self.coco.cats.values())
        self.cat_ids = self.coco.get_cat_ids(cat_names=self.CLASSES)
        self.img_ids = self.coco.get_img_ids()
        self._flex_gt = None
        self._recall_gt = None

    def __len__(self):
        return len(self.img_ids)

    def recall_gt(self):
        """The ground truth of ``fast_eval_recall`` (``datasets/coco.py:305-322``): per image of ``img_ids`` every
        annotation, of any category, that is neither ``ignore`` nor ``iscrowd``, in the file's order; ``x1, y1, x1 + w,
        y1 + h`` formed in float64, then cast to float32.  One ``RecallGt``, built on first use and kept."""
        if self._recall_gt is None:
            per_img = {i: [] for i in self.img_ids}
            for ann in self.coco.dataset.get('annotations', []):
                if ann['image_id'] in per_img and not (ann.get('ignore', False) or ann.get('iscrowd', 0)):
                    x1, y1, w, h = ann['bbox']
                    per_img[ann['image_id']].append([x1, y1, x1 + w, y1 + h])
            self._recall_gt = RecallGt([np.array(per_img[i], dtype=np.float32).reshape(-1, 4) for i in self.img_ids])
        return self._recall_gt

    def fast_eval_recall(self, results, proposal_nums, iou_thrs, logger=None):
        """``datasets/coco.py:305-327``: ``eval_recalls`` of the results, labels dropped, against ``recall_gt()``;
        returns the average recall per proposal number, ``recalls.mean(axis=1)``.  ``results``: the per-image lists or
        the flat tuple."""
        return eval_recalls(self.recall_gt(), results, proposal_nums, iou_thrs, logger=logger).mean(axis=1)

    def flex_gt(self):
        """The ground truth of ``metric='fast-bbox'``: per image of ``img_ids`` what ``CocoDataset.get_ann_info_test``
        returns (``coco_test_annotation``; a box of an unlisted category keeps label -1, which no class owns), as one
        ``FlexGt`` with the metric's three scale ranges.  Built on first use and kept."""
        if self._flex_gt is None:
            per_img = {i: [] for i in self.img_ids}
            for ann in self.coco.dataset.get('annotations', []):
                if ann['image_id'] in per_img:
                    per_img[ann['image_id']].append(ann)
            cat2label = {c['id']: -1 for c in self.coco.cats.values()}
            cat2label.update({cat_id: i for i, cat_id in enumerate(self.cat_ids)})
            annotations = [coco_test_annotation(per_img[i], self.cat_ids, cat2label) for i in self.img_ids]
            self._flex_gt = FlexGt(annotations, len(self.CLASSES), FAST_BBOX_SCALE_RANGES)
        return self._flex_gt

    def _det2json(self, results):
        """``datasets/coco.py:210-225``: one record per detection -- image, class, row order -- with ``bbox`` as
        ``[x1, y1, x2 - x1, y2 - y1]`` formed from the Python floats of the float32 values (``xyxy2xywh``).
        ``results``: the per-image lists or the flat tuple (tensors or arrays); the flat rows are in that order
        already."""
        if isinstance(results, tuple) and len(results) == 3 and not isinstance(results[0], (list, tuple)):
            dets, labels, img_index = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in results)
        else:
            if len(results) != len(self):
                raise AssertionError(f'The length of results is not equal to the dataset len: {len(results)} != '
                                     f'{len(self)}')
            dets, labels, img_index = flatten_results(results)
        if dets.shape[0] and (int(labels.max()) >= len(self.cat_ids) or int(img_index.max()) >= len(self.img_ids)):
            raise ValueError('results name a class or an image the dataset does not have')
        rows = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 5).tolist()
        return [dict(image_id=self.img_ids[i], bbox=[r[0], r[1], r[2] - r[0], r[3] - r[1]], score=r[4],
                     category_id=self.cat_ids[c]) for r, c, i in zip(rows, labels.tolist(), img_index.tolist())]

    def results2json(self, results, outfile_prefix):
        """``datasets/coco.py:265-303`` for box results: ``<outfile_prefix>.bbox.json`` (what ``json.dump`` writes with
        its defaults, as ``mmcv.dump`` does); returns ``dict(bbox=..., proposal=...)``, both that file."""
        import json
        path = f'{outfile_prefix}.bbox.json'
        with open(path, 'w') as f:
            json.dump(self._det2json(results), f)
        return dict(bbox=path, proposal=path)

    def format_results(self, results, jsonfile_prefix=None, **kwargs):
        """``datasets/coco.py:329-355``: the results as a COCO result file (the form a test server takes).  Returns
        ``(result_files, tmp_dir)``; without ``jsonfile_prefix`` the file goes into a ``tempfile.TemporaryDirectory``,
        returned as ``tmp_dir`` (the caller cleans it up), else ``tmp_dir`` is None.  The per-image lists and the flat
        tuple (``DeviceResults``) give the same bytes."""
        import os
        import tempfile
        if not isinstance(results, (list, tuple)):
            raise AssertionError('results must be a list')
        if jsonfile_prefix is None:
            tmp_dir = tempfile.TemporaryDirectory()
            jsonfile_prefix = os.path.join(tmp_dir.name, 'results')
        else:
            tmp_dir = None
        return self.results2json(results, jsonfile_prefix), tmp_dir

    def evaluate(self, results, metric='bbox', logger=None, **kwargs):
        """``CocoDataset.evaluate`` (``datasets/coco.py:451-643``): ``metric='bbox'`` through ``evaluate_bbox``,
        ``metric='fast-bbox'`` (alone, as in the reference) through ``evaluate_fast_bbox`` against ``flex_gt()``,
        ``metric='proposal_fast'`` through ``fast_eval_recall`` (``AR@{num}`` keys; ``proposal_nums`` and ``iou_thrs``
        are the keywords ``evaluate_bbox`` takes, with its defaults).  In a list the metrics keep their order and
        merge into one ``OrderedDict``.  ``results``: the per-image lists or the flat tuple, ``img_index`` being
        positions in ``img_ids``."""
        metrics = list(metric) if isinstance(metric, (list, tuple)) else [metric]
        if 'fast-bbox' in metrics:
            assert len(metrics) == 1, 'fast-bbox evaluation can only be used alone!'
            if kwargs:                # (the reference ignores them: its thresholds, ranges and report are fixed)
                raise TypeError(f"metric='fast-bbox' takes no further arguments (its thresholds, scale ranges and report "
                                f'are fixed), got {sorted(kwargs)}')
            return evaluate_fast_bbox(results, self.flex_gt(), self.CLASSES, logger=logger)
        if 'proposal_fast' not in metrics:
            return evaluate_bbox(results, self.coco, cat_ids=self.cat_ids, img_ids=self.img_ids, logger=logger,
                                 metric=metric, **kwargs)
        for m in metrics:             # (as the reference: before anything is scored)
            if m not in ('bbox', 'segm', 'proposal', 'proposal_fast'):
                raise KeyError(f'metric {m} is not supported')
        proposal_nums = kwargs.get('proposal_nums', (100, 300, 1000))
        iou_thrs = kwargs.get('iou_thrs', None)
        if iou_thrs is None:
            iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        eval_results = OrderedDict()
        for m in metrics:
            if m != 'proposal_fast':
                eval_results.update(evaluate_bbox(results, self.coco, cat_ids=self.cat_ids, img_ids=self.img_ids,
                                                  logger=logger, metric=m, **kwargs))
                continue
            msg = f'Evaluating {m}...'
            _log('\n' + msg if logger is None else msg, logger)
            ar = self.fast_eval_recall(results, proposal_nums, iou_thrs, logger='silent')
            log_msg = []
            for i, num in enumerate(proposal_nums):
                eval_results[f'AR@{num}'] = ar[i]
                log_msg.append(f'\nAR@{num}\t{ar[i]:.4f}')
            _log(''.join(log_msg), logger)
        return eval_results

    def error_analysis(self, results, **kw):
        """``coco_error.error_analysis`` of ``results`` (any form it takes) against the annotation file held here, with
        this dataset's label -> category and index -> image maps: the C75 / C50 / Loc / Sim / Oth / BG / FN breakdown of
        the reference's ``tools/analysis_tools/coco_error_analysis.py``."""
        from .coco_error import error_analysis
        return error_analysis(self.coco, results, cat_ids=self.cat_ids, img_ids=self.img_ids, **kw)


class CustomBBoxDataset:
    """The ``.dataset`` of a validation loader that scores ``metric='mAP'``, as ``CustomDataset.evaluate`` and
    ``VOCDataset.evaluate`` do by default (``datasets/custom.py:280-337``).  ``annotations``: per image the dict that
    ``get_ann_info`` returns (``bboxes`` (n, 4), ``labels`` (n,), optionally ``bboxes_ignore`` / ``labels_ignore``);
    ``classes``: the class names.  It loads no images.  ``accepts_flat``: ``evaluate`` takes the flat GPU table as well
    as the list form; the ground-truth tables are built once (``MapGt``) and their device copies kept."""

    # the flat loop plus device scoring against the list loop plus list scoring: DESIGN 18's table
    accepts_flat = True

    def __init__(self, annotations, classes):
        self.CLASSES = tuple(classes)
        self.annotations = list(annotations)
        self.map_gt = MapGt(self.annotations, len(self.CLASSES))
        self._recall_gt = None

    def __len__(self):
        return len(self.annotations)

    def get_ann_info(self, idx):
        return self.annotations[idx]

    def evaluate(self, results, metric='mAP', logger=None, iou_thr=0.5, scale_ranges=None):
        """``evaluate_map``: ``AP50``-style keys and ``mAP``; ``results``: the per-image lists or the flat tuple,
        ``img_index`` being positions in ``annotations``.  Unknown metrics raise ``KeyError``; ``'recall'`` raises what
        ``evaluate_map`` raises."""
        return evaluate_map(results, self.map_gt, classes=list(self.CLASSES), iou_thr=iou_thr, scale_ranges=scale_ranges,
                            logger=logger, metric=metric)

    def eval_recalls(self, results, proposal_nums=(100, 300, 1000), iou_thr=0.5, logger=None):
        """The ``metric='recall'`` branch of ``CustomDataset.evaluate`` (``datasets/custom.py:326-336``) as a method of
        its own (``evaluate(metric='recall')`` keeps raising): the results, labels dropped, against the annotations'
        ``bboxes``.  ``recall@{num}@{iou}`` per proposal number and threshold, and ``AR@{num}`` when there is more than
        one threshold.  ``results``: the per-image lists or the flat tuple."""
        if self._recall_gt is None:
            self._recall_gt = RecallGt([a['bboxes'] for a in self.annotations])
        iou_thrs = [iou_thr] if isinstance(iou_thr, float) else iou_thr
        recalls = eval_recalls(self._recall_gt, results, proposal_nums, iou_thr, logger=logger)
        eval_results = OrderedDict()
        for i, num in enumerate(proposal_nums):
            for j, iou in enumerate(iou_thrs):
                eval_results[f'recall@{num}@{iou}'] = recalls[i, j]
        if recalls.shape[1] > 1:
            ar = recalls.mean(axis=1)
            for i, num in enumerate(proposal_nums):
                eval_results[f'AR@{num}'] = ar[i]
        return eval_results
