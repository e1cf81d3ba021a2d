"""The reference's dataset wrappers (``mmdet/datasets/dataset_wrappers.py``) and its ``build_dataset``
(``builder.py:26-73``): ``ConcatDataset``, ``RepeatDataset``, ``ClassBalancedDataset``, lists of blocks, nested wrappers,
and an ``ann_file`` list with per-entry prefixes.

A wrapper holds no images and no tables of its own.  It exposes ``flag``, ``CLASSES``, ``__len__``, ``get_cat_ids`` and
``resolve(idx) -> (innermost dataset, its index)``; the loaders (``datasets.TrainLoader`` / ``TestLoader``) go through
``resolve`` for everything a sample needs -- its file, its annotation, and its mosaic partners, which are drawn from the
dataset that owns the sample (the reference hands ``results['dataset'] = self`` of the inner dataset to
``MosaicPipeline``).  ``pipeline`` is the innermost (first) dataset's block.
"""
import bisect
import copy
import math
from collections import defaultdict

import numpy as np
import torch

from ._eval_common import _is_flat, _log
from .registry import DATASETS, build_from_cfg


class _Wrapper:
    """What the three wrappers share: the way down to the datasets that own the samples."""

    def _children(self):
        return [self.dataset]

    def leaves(self):
        """The innermost datasets, in order."""
        out = []
        for d in self._children():
            out += d.leaves() if isinstance(d, _Wrapper) else [d]
        return out

    @property
    def pipeline(self):
        return self.leaves()[0].pipeline

    def resolve(self, idx):
        """``(innermost dataset, index in it)`` of sample ``idx``."""
        d, i = self._inner(int(idx))
        return d.resolve(i) if isinstance(d, _Wrapper) else (d, i)


@DATASETS.register_module()
class ConcatDataset(_Wrapper):
    """``dataset_wrappers.py:13-124`` (on ``torch.utils.data.ConcatDataset``'s ``cumulative_sizes``): the datasets one
    after another, their group flags concatenated.  ``separate_eval``: as a validation dataset, score every dataset on
    its own slice of the results, with ``{i}_`` key prefixes; ``False`` scores the whole as ``datasets[0]`` with every
    dataset's ``data_infos``, which is refused for ``CocoDataset`` and for datasets of different types."""

    def __init__(self, datasets, separate_eval=True):
        self.datasets = list(datasets)
        assert len(self.datasets) > 0, 'datasets should not be an empty iterable'
        self.cumulative_sizes = np.cumsum([len(d) for d in self.datasets]).tolist()
        self.CLASSES = self.datasets[0].CLASSES
        self.separate_eval = separate_eval
        if not separate_eval:
            self._refuse_joint()
        if hasattr(self.datasets[0], 'flag'):
            self.flag = np.concatenate([d.flag for d in self.datasets])

    def _refuse_joint(self):
        from .datasets import CocoDataset
        if any(isinstance(ds, CocoDataset) for ds in self.datasets):
            raise NotImplementedError('Evaluating concatenated CocoDataset as a whole is not supported! Please set '
                                      '"separate_eval=True"')
        if len(set(type(ds) for ds in self.datasets)) != 1:
            raise NotImplementedError('All the datasets should have same types')

    def _children(self):
        return self.datasets

    def __len__(self):
        return self.cumulative_sizes[-1]

    def _inner(self, idx):
        if idx < 0:
            if -idx > len(self):
                raise ValueError('absolute value of index should not exceed dataset length')
            idx = len(self) + idx
        k = bisect.bisect_right(self.cumulative_sizes, idx)
        return self.datasets[k], idx if k == 0 else idx - self.cumulative_sizes[k - 1]

    def get_cat_ids(self, idx):
        d, i = self._inner(int(idx))
        return d.get_cat_ids(i)

    @property
    def accepts_flat(self):
        return all(getattr(d, 'accepts_flat', False) for d in self.datasets)

    @staticmethod
    def _slice(results, lo, hi):
        """The results of images ``[lo, hi)``.  Flat form: the rows whose ``img_index`` lies in the range, in table
        order, re-based to the slice -- three masked selects where the table lives (on the device for a
        ``DeviceResults`` table), no per-image lists."""
        if not _is_flat(results):
            return results[lo:hi]
        dets, labels, img_index = results
        if isinstance(img_index, torch.Tensor):
            keep = (img_index >= lo) & (img_index < hi)
            return dets[keep], labels[keep], img_index[keep] - lo
        img_index = np.asarray(img_index)
        keep = (img_index >= lo) & (img_index < hi)
        return np.asarray(dets)[keep], np.asarray(labels)[keep], img_index[keep] - lo

    def evaluate(self, results, logger=None, **kwargs):
        """``dataset_wrappers.py:68-124``.  ``results``: the per-image lists or the flat tuple."""
        if not _is_flat(results):
            assert len(results) == self.cumulative_sizes[-1], \
                f'Dataset and results have different sizes: {self.cumulative_sizes[-1]} v.s. {len(results)}'
        for dataset in self.datasets:
            assert hasattr(dataset, 'evaluate'), f'{type(dataset)} does not implement evaluate function'
        if self.separate_eval:
            total = dict()
            for k, dataset in enumerate(self.datasets):
                lo, hi = (0 if k == 0 else self.cumulative_sizes[k - 1]), self.cumulative_sizes[k]
                _log(f'\nEvaluateing {dataset.ann_file} with {hi - lo} images now', logger)
                for key, v in dataset.evaluate(self._slice(results, lo, hi), logger=logger, **kwargs).items():
                    total[f'{k}_{key}'] = v
            return total
        self._refuse_joint()
        first = self.datasets[0]
        original = first.data_infos
        first.data_infos = sum([d.data_infos for d in self.datasets], [])
        first._reset_gt()
        try:
            return first.evaluate(results, logger=logger, **kwargs)
        finally:
            first.data_infos = original
            first._reset_gt()


@DATASETS.register_module()
class RepeatDataset(_Wrapper):
    """``dataset_wrappers.py:127-167``: ``times`` passes over ``dataset`` as one epoch."""

    def __init__(self, dataset, times):
        self.dataset, self.times = dataset, times
        self.CLASSES = dataset.CLASSES
        if hasattr(dataset, 'flag'):
            self.flag = np.tile(dataset.flag, times)
        self._ori_len = len(dataset)

    def _inner(self, idx):
        return self.dataset, idx % self._ori_len

    def get_cat_ids(self, idx):
        return self.dataset.get_cat_ids(idx % self._ori_len)

    def __len__(self):
        return self.times * self._ori_len


@DATASETS.register_module()
class ClassBalancedDataset(_Wrapper):
    """``dataset_wrappers.py:171-282``: image ``i`` appears ``ceil(r(i))`` times, ``r(i) = max over its categories of
    max(1, sqrt(oversample_thr / f(c)))``, ``f(c)`` being the fraction of images that hold category ``c``.
    ``filter_empty_gt=False`` counts an image without boxes as the background category."""

    def __init__(self, dataset, oversample_thr, filter_empty_gt=True):
        self.dataset, self.oversample_thr, self.filter_empty_gt = dataset, oversample_thr, filter_empty_gt
        self.CLASSES = dataset.CLASSES
        repeat_factors = self._get_repeat_factors(dataset, oversample_thr)
        repeat_indices = []
        for dataset_idx, repeat_factor in enumerate(repeat_factors):
            repeat_indices.extend([dataset_idx] * math.ceil(repeat_factor))
        self.repeat_indices = repeat_indices
        flags = []
        if hasattr(dataset, 'flag'):
            for flag, repeat_factor in zip(dataset.flag, repeat_factors):
                flags.extend([flag] * int(math.ceil(repeat_factor)))
            assert len(flags) == len(repeat_indices)
        self.flag = np.asarray(flags, dtype=np.uint8)

    def _get_repeat_factors(self, dataset, repeat_thr):
        category_freq = defaultdict(int)
        num_images = len(dataset)
        cat_ids_of = []
        for idx in range(num_images):
            cat_ids = set(dataset.get_cat_ids(idx))
            if len(cat_ids) == 0 and not self.filter_empty_gt:
                cat_ids = set([len(self.CLASSES)])
            cat_ids_of.append(cat_ids)
            for cat_id in cat_ids:
                category_freq[cat_id] += 1
        for k, v in category_freq.items():
            category_freq[k] = v / num_images
        category_repeat = {cat_id: max(1.0, math.sqrt(repeat_thr / cat_freq)) for cat_id, cat_freq in category_freq.items()}
        repeat_factors = []
        for cat_ids in cat_ids_of:
            repeat_factor = 1
            if len(cat_ids) > 0:
                repeat_factor = max({category_repeat[cat_id] for cat_id in cat_ids})
            repeat_factors.append(repeat_factor)
        return repeat_factors

    def _inner(self, idx):
        return self.dataset, self.repeat_indices[idx]

    def get_cat_ids(self, idx):
        return self.dataset.get_cat_ids(self.repeat_indices[int(idx)])

    def __len__(self):
        return len(self.repeat_indices)


def _concat_dataset(cfg, default_args=None):
    """``builder.py:26-50``: one dataset per entry of the ``ann_file`` list, with its own prefix where those are lists."""
    ann_files = cfg['ann_file']
    img_prefixes = cfg.get('img_prefix', None)
    seg_prefixes = cfg.get('seg_prefix', None)
    proposal_files = cfg.get('proposal_file', None)
    separate_eval = cfg.get('separate_eval', True)
    datasets = []
    for i in range(len(ann_files)):
        data_cfg = copy.deepcopy(dict(cfg))
        data_cfg.pop('separate_eval', None)
        data_cfg['ann_file'] = ann_files[i]
        if isinstance(img_prefixes, (list, tuple)):
            data_cfg['img_prefix'] = img_prefixes[i]
        if isinstance(seg_prefixes, (list, tuple)):
            data_cfg['seg_prefix'] = seg_prefixes[i]
        if isinstance(proposal_files, (list, tuple)):
            data_cfg['proposal_file'] = proposal_files[i]
        datasets.append(build_dataset(data_cfg, default_args))
    return ConcatDataset(datasets, separate_eval)


def build_dataset(cfg, default_args=None):
    """``builder.py:53-73``.  ``default_args`` (``dict(test_mode=True)`` of a validation loader, say) reach every plain
    dataset block, whose own keys win."""
    if isinstance(cfg, (list, tuple)):
        return ConcatDataset([build_dataset(c, default_args) for c in cfg])
    if cfg['type'] == 'ConcatDataset':
        return ConcatDataset([build_dataset(c, default_args) for c in cfg['datasets']], cfg.get('separate_eval', True))
    if cfg['type'] == 'RepeatDataset':
        return RepeatDataset(build_dataset(cfg['dataset'], default_args), cfg['times'])
    if cfg['type'] == 'ClassBalancedDataset':
        return ClassBalancedDataset(build_dataset(cfg['dataset'], default_args), cfg['oversample_thr'])
    if isinstance(cfg.get('ann_file'), (list, tuple)):
        return _concat_dataset(cfg, default_args)
    return build_from_cfg(cfg, DATASETS, default_args)
