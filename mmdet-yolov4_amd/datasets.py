"""Training from image files: the COCO dataset in train mode, the group samplers and a loader that decodes and augments
on the GPU.

``cfg.data.train`` of a reference config (``configs/yolov4/*.py``: ``dict(type='CocoDataset', ann_file=...,
img_prefix=..., pipeline=train_pipeline)``) goes through ``build_train_loader`` and yields ``train_step`` data dicts:

* ``CocoDataset`` restates ``mmdet/datasets/coco.py`` and ``custom.py`` on ``coco_eval.CocoGt`` (no pycocotools): which
  images survive, their aspect-ratio groups, each image's boxes, and the random partner draws of the mosaic.
* ``GroupSampler`` / ``DistributedGroupSampler`` restate ``mmdet/datasets/samplers/group_sampler.py``.
* ``TrainLoader`` takes the sampler's indices, reads the files on a thread pool, decodes the whole batch with ONE
  ``image_io.decode_into`` call and hands the device views to the fused pipeline (``build_train_pipeline``).  No pixel
  crosses back to the host.
* ``TestLoader`` (``build_test_loader`` over ``cfg.data.val`` / ``cfg.data.test``) is the test side's counterpart: the
  order of ``DistributedSampler(shuffle=False)``, the same reads and ONE decode per batch, then the test pipeline
  (``FusedTestPipeline``), in the nested form ``single_gpu_test`` / ``EvalHook`` take.

What the loaders ask of a dataset, and nothing else: ``data_infos[i]['filename']``, ``img_prefix``, ``flag``,
``get_ann_info``, ``batch_rand_others`` / ``_rand_another``, ``pipeline``, ``CLASSES`` and, on the test side, ``evaluate``
-- so ``custom_datasets`` (the middle-format pickle, VOC XML, the traffic-sign folders, whose ``data_infos`` carry no
size) serve as ``CocoDataset`` does.  Under a wrapper (``dataset_wrappers``: ``RepeatDataset``, ``ConcatDataset``,
``ClassBalancedDataset``) the sampler works on the wrapper's ``flag`` and length, and every sample is resolved to
``(innermost dataset, index)``: its file, its annotation and its mosaic partners come from the dataset that owns it;
``draws['sources']`` then names samples as ``(owner's number, index)``.

What is pinned draw for draw against the reference (tests/golden/coco_train_set.npz): ``CocoDataset._rand_another`` /
``batch_rand_others`` and both samplers' orders, given the same generator state.  What is this loader's own: the ORDER
in which the samples of a batch take their draws.  The reference spreads them over its worker processes, each with its
own ``np.random`` state, so its stream cannot be replayed; here one ``RandomState`` per (seed, epoch, rank) serves, in
this order per batch: ``batch_rand_others`` for each sample in sample order (mosaic only), a ``_rand_another`` for each
refused file (``on_unsupported='resample'``), then the pipeline's draws for each sample in sample order.
"""
import logging
import math
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import image_io
from .augment import FusedTrainPipeline
from .augment_v3 import build_train_pipeline
from .dataset_wrappers import build_dataset  # noqa: F401  (builder.py:53-73: plain blocks, wrappers, lists of blocks)
from .registry import DATASETS
from .results import CocoBBoxDataset

#: the files of a batch are read on at most this many threads (never sized from the machine's CPU count)
MAX_READ_THREADS = 16

COCO_CLASSES = ('person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat', 'traffic light',
                'fire hydrant', 'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow',
                'elephant', 'bear', 'zebra', 'giraffe', 'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee',
                'skis', 'snowboard', 'sports ball', 'kite', 'baseball bat', 'baseball glove', 'skateboard', 'surfboard',
                'tennis racket', 'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl', 'banana', 'apple',
                'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair', 'couch',
                'potted plant', 'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote', 'keyboard',
                'cell phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'book', 'clock', 'vase', 'scissors',
                'teddy bear', 'hair drier', 'toothbrush')


@DATASETS.register_module()
class CocoDataset(CocoBBoxDataset):
    """``CocoDataset`` of the reference (``mmdet/datasets/coco.py:19-173`` on ``custom.py:56-191``) for ``bbox`` work:
    the annotation tables of training, and ``evaluate`` from ``CocoBBoxDataset``.  ``pipeline`` is kept as the config
    block (``build_train_loader`` builds the fused pipeline from it); ``classes``: a sequence of names, or ``None`` for
    the 80 COCO names (``coco.py:21-34``; a file of names is not built).  With ``test_mode`` nothing is filtered and no
    group flag is set (``custom.py:96-102``).  Parity with pycocotools itself is unpinned (it is absent here): ``CocoGt``
    stands in for its ``COCO`` class -- image, category and annotation ids in file order."""

    CLASSES = COCO_CLASSES

    def __init__(self, ann_file, pipeline=None, classes=None, data_root=None, img_prefix='', test_mode=False,
                 filter_empty_gt=True):
        if isinstance(classes, str):
            raise NotImplementedError('CocoDataset(classes=<file name>) is not built: pass the names')
        self.data_root, self.img_prefix = data_root, img_prefix
        if data_root is not None:                                          # custom.py:76-80
            if isinstance(ann_file, str) and not os.path.isabs(ann_file):
                ann_file = os.path.join(data_root, ann_file)
            if not (img_prefix is None or os.path.isabs(img_prefix)):
                self.img_prefix = os.path.join(data_root, img_prefix)
        super().__init__(ann_file, classes=self.CLASSES if classes is None else classes)
        self.ann_file = ann_file
        self.pipeline = pipeline
        self.test_mode, self.filter_empty_gt = test_mode, filter_empty_gt
        self.data_infos = self.load_annotations()
        if not test_mode:
            valid_inds = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid_inds]
            self.valid_inds = valid_inds
            self._set_group_flag()

    def __len__(self):
        return len(self.data_infos)

    def load_annotations(self):
        """``coco.py:36-60``: ``data_infos`` in ``get_img_ids()`` order with ``filename = file_name``; each image's
        annotation records in file order (``COCO.get_ann_ids(img_ids=[i])``); annotation ids must be unique."""
        self.cat2label = {cat_id: i for i, cat_id in enumerate(self.cat_ids)}
        self.img_ids = self.coco.get_img_ids()
        self._img_anns = {i: [] for i in self.img_ids}
        for ann in self.coco.dataset.get('annotations', []):
            if ann['image_id'] in self._img_anns:
                self._img_anns[ann['image_id']].append(ann)
        data_infos, total_ann_ids = [], []
        for i in self.img_ids:
            info = self.coco.imgs[i]
            info['filename'] = info['file_name']
            data_infos.append(info)
            total_ann_ids.extend(a['id'] for a in self._img_anns[i])
        assert len(set(total_ann_ids)) == len(total_ann_ids), f"Annotation ids in '{self.ann_file}' are not unique!"
        return data_infos

    def _filter_imgs(self, min_size=32):
        """``coco.py:92-114``: with ``filter_empty_gt`` only images that hold an annotation of a listed category stay;
        images whose shorter side is below ``min_size`` go; ``img_ids`` becomes the survivors'."""
        valid_inds, valid_img_ids = [], []
        anns = self.coco.dataset.get('annotations', [])
        ids_with_ann = set(a['image_id'] for a in anns)
        cat_ids = set(self.cat_ids)
        ids_in_cat = set(a['image_id'] for a in anns if a['category_id'] in cat_ids) & ids_with_ann
        for i, img_info in enumerate(self.data_infos):
            img_id = self.img_ids[i]
            if self.filter_empty_gt and img_id not in ids_in_cat:
                continue
            if min(img_info['width'], img_info['height']) >= min_size:
                valid_inds.append(i)
                valid_img_ids.append(img_id)
        self.img_ids = valid_img_ids
        return valid_inds

    def _set_group_flag(self):
        """``custom.py:164-174``: aspect ratio ``width / height > 1`` is group 1, the rest group 0."""
        self.flag = np.zeros(len(self), dtype=np.uint8)
        for i in range(len(self)):
            img_info = self.data_infos[i]
            if img_info['width'] / img_info['height'] > 1:
                self.flag[i] = 1

    def get_ann_info(self, idx):
        """``coco.py:62-75``."""
        info = self.data_infos[idx]
        return self._parse_ann_info(info, self._img_anns[info['id']])

    def get_cat_ids(self, idx):
        """``coco.py:77-90``."""
        return [ann['category_id'] for ann in self._img_anns[self.data_infos[idx]['id']]]

    def _parse_ann_info(self, img_info, ann_info):
        """``coco.py:116-173`` without the masks: ``ignore`` records, boxes that do not meet the image, boxes with
        ``area <= 0 or w < 1 or h < 1`` and boxes of unlisted categories are skipped; crowd boxes go to
        ``bboxes_ignore``; x y w h becomes x1 y1 x2 y2; float32 boxes, int64 labels, (0, 4) / (0,) when empty."""
        gt_bboxes, gt_labels, gt_bboxes_ignore = [], [], []
        for ann in ann_info:
            if ann.get('ignore', False):
                continue
            x1, y1, w, h = ann['bbox']
            inter_w = max(0, min(x1 + w, img_info['width']) - max(x1, 0))
            inter_h = max(0, min(y1 + h, img_info['height']) - max(y1, 0))
            if inter_w * inter_h == 0:
                continue
            if ann['area'] <= 0 or w < 1 or h < 1:
                continue
            if ann['category_id'] not in self.cat_ids:
                continue
            bbox = [x1, y1, x1 + w, y1 + h]
            if ann.get('iscrowd', False):
                gt_bboxes_ignore.append(bbox)
            else:
                gt_bboxes.append(bbox)
                gt_labels.append(self.cat2label[ann['category_id']])
        if gt_bboxes:
            gt_bboxes = np.array(gt_bboxes, dtype=np.float32)
            gt_labels = np.array(gt_labels, dtype=np.int64)
        else:
            gt_bboxes = np.zeros((0, 4), dtype=np.float32)
            gt_labels = np.array([], dtype=np.int64)
        if gt_bboxes_ignore:
            gt_bboxes_ignore = np.array(gt_bboxes_ignore, dtype=np.float32)
        else:
            gt_bboxes_ignore = np.zeros((0, 4), dtype=np.float32)
        return dict(bboxes=gt_bboxes, labels=gt_labels, bboxes_ignore=gt_bboxes_ignore,
                    seg_map=img_info['filename'].replace('jpg', 'png'))

    def _rand_another(self, idx, rng=np.random):
        """``custom.py:176-179``, drawing from ``rng`` (a ``RandomState``; default: the module-level ``np.random``)."""
        pool = np.where(self.flag == self.flag[idx])[0]
        return rng.choice(pool)

    def batch_rand_others(self, idx, batch, rng=np.random):
        """``custom.py:181-191``, draw for draw: ``batch`` other indices of ``idx``'s group -- ``[idx] * batch`` when
        there is no other, with replacement when there are fewer than ``batch``, without otherwise."""
        mask = (self.flag == self.flag[idx])
        mask[idx] = False
        pool = np.where(mask)[0]
        if len(pool) == 0:
            return np.array([idx] * batch)
        if len(pool) < batch:
            return rng.choice(pool, size=batch, replace=True)
        return rng.choice(pool, size=batch, replace=False)


class GroupSampler:
    """``group_sampler.py:10-48``: every group shuffled, padded to a multiple of ``samples_per_gpu`` with
    ``choice(indice, num_extra)``, then whole batches permuted -- the same three calls on ``rng`` (a ``RandomState``;
    default: the module-level ``np.random``).  With ``seed``, ``set_epoch(e)`` replaces ``rng`` by
    ``RandomState([seed, e])`` (the reference's class has no epoch: its order comes from the process's global state)."""

    def __init__(self, dataset, samples_per_gpu=1, rng=None, seed=None):
        assert hasattr(dataset, 'flag')
        self.dataset = dataset
        self.samples_per_gpu = samples_per_gpu
        self.flag = dataset.flag.astype(np.int64)
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = 0
        for i, size in enumerate(self.group_sizes):
            self.num_samples += int(np.ceil(size / self.samples_per_gpu)) * self.samples_per_gpu
        self.seed, self.epoch = seed, 0
        self.rng = rng if rng is not None else np.random
        if seed is not None:
            self.set_epoch(0)

    def set_epoch(self, epoch):
        self.epoch = epoch
        if self.seed is not None:
            self.rng = np.random.RandomState([int(self.seed), int(epoch)])

    def __iter__(self):
        rng = self.rng
        indices = []
        for i, size in enumerate(self.group_sizes):
            if size == 0:
                continue
            indice = np.where(self.flag == i)[0]
            assert len(indice) == size
            rng.shuffle(indice)
            num_extra = int(np.ceil(size / self.samples_per_gpu)) * self.samples_per_gpu - len(indice)
            indice = np.concatenate([indice, rng.choice(indice, num_extra)])
            indices.append(indice)
        indices = np.concatenate(indices)
        indices = [indices[i * self.samples_per_gpu:(i + 1) * self.samples_per_gpu]
                   for i in rng.permutation(range(len(indices) // self.samples_per_gpu))]
        indices = np.concatenate(indices)
        indices = indices.astype(np.int64).tolist()
        assert len(indices) == self.num_samples
        return iter(indices)

    def __len__(self):
        return self.num_samples


class DistributedGroupSampler:
    """``group_sampler.py:51-148``: one ``torch.Generator`` seeded ``epoch + seed`` permutes every group
    (``torch.randperm``) and then the whole batches; groups are padded by repetition to a multiple of
    ``samples_per_gpu * num_replicas``; rank ``r`` takes the ``r``-th contiguous run of ``num_samples``."""

    def __init__(self, dataset, samples_per_gpu=1, num_replicas=1, rank=0, seed=0):
        self.dataset = dataset
        self.samples_per_gpu = samples_per_gpu
        self.num_replicas = num_replicas
        self.rank = rank
        self.epoch = 0
        self.seed = seed if seed is not None else 0
        assert hasattr(self.dataset, 'flag')
        self.flag = self.dataset.flag
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = 0
        for i, j in enumerate(self.group_sizes):
            self.num_samples += int(math.ceil(self.group_sizes[i] * 1.0 / self.samples_per_gpu /
                                              self.num_replicas)) * self.samples_per_gpu
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.epoch + self.seed)
        indices = []
        for i, size in enumerate(self.group_sizes):
            if size > 0:
                indice = np.where(self.flag == i)[0]
                assert len(indice) == size
                indice = indice[list(torch.randperm(int(size), generator=g).numpy())].tolist()
                extra = int(math.ceil(size * 1.0 / self.samples_per_gpu / self.num_replicas)
                            ) * self.samples_per_gpu * self.num_replicas - len(indice)
                tmp = indice.copy()
                for _ in range(extra // size):
                    indice.extend(tmp)
                indice.extend(tmp[:extra % size])
                indices.extend(indice)
        assert len(indices) == self.total_size
        indices = [indices[j] for i in list(torch.randperm(len(indices) // self.samples_per_gpu, generator=g))
                   for j in range(i * self.samples_per_gpu, (i + 1) * self.samples_per_gpu)]
        offset = self.num_samples * self.rank
        indices = indices[offset:offset + self.num_samples]
        assert len(indices) == self.num_samples
        return iter(indices)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


class _FileLoader:
    """What ``TrainLoader`` and ``TestLoader`` share: the files' paths, the reader pool, the host work of one batch
    (reads, header parses, ``image_io.HostHalf``), the naming of a damaged file, and the ``prefetch`` worker that does the
    next batch's host work while the caller uses this one.  A subclass gives ``_start(batch)`` -- whatever must happen on
    the caller's thread before the host work, ending in ``_submit(sources)`` -- and ``_finish(started)``."""

    def __init__(self, dataset, rank, world, device, entropy, prefetch, orientation):
        if prefetch not in (0, 1):
            raise ValueError(f'prefetch {prefetch!r} is not 0 or 1')
        if not 0 <= rank < world:
            raise ValueError(f'rank {rank} of world {world}')
        self.dataset = dataset
        self.rank, self.world = int(rank), int(world)
        self.device = torch.device(device) if device is not None else None
        self.entropy = image_io._entropy_mode(entropy)
        self.prefetch, self.orientation = prefetch, bool(orientation)
        # under a wrapper (dataset_wrappers) a sample is named by (number of the innermost dataset that owns it, its index there)
        self._leaves = dataset.leaves() if hasattr(dataset, 'resolve') else None
        self._leaf_no = {id(d): k for k, d in enumerate(self._leaves)} if self._leaves is not None else None
        self._readers = ThreadPoolExecutor(max_workers=MAX_READ_THREADS, thread_name_prefix='yv4-read')
        self._worker = ThreadPoolExecutor(max_workers=1, thread_name_prefix='yv4-prefetch') if prefetch else None

    def close(self):
        """Ends the loader's threads (they are idle between batches; an interpreter exit ends them as well)."""
        self._readers.shutdown(wait=True)
        if self._worker is not None:
            self._worker.shutdown(wait=True)

    def _dev(self):
        return self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())

    def _own(self, idx):
        """The name of the loader's sample ``idx`` from here on: ``idx`` itself for a plain dataset, under a wrapper
        ``(owner's number, index in the owner)``."""
        if self._leaves is None:
            return idx
        ds, i = self.dataset.resolve(idx)
        return self._leaf_no[id(ds)], int(i)

    def _at(self, j):
        """``(the dataset that owns sample j, j's index in it)``."""
        return (self._leaves[j[0]], j[1]) if isinstance(j, tuple) else (self.dataset, j)

    @staticmethod
    def _sibling(j, i):
        """Index ``i`` of the dataset that owns ``j``, named as ``j`` is."""
        return (j[0], int(i)) if isinstance(j, tuple) else int(i)

    def _filename(self, j):
        ds, i = self._at(j)
        return ds.data_infos[i]['filename']

    def _path(self, j):
        ds, i = self._at(j)
        name = ds.data_infos[i]['filename']
        return os.path.join(ds.img_prefix, name) if ds.img_prefix is not None else name

    # ---- host work of one batch: no HIP call, no torch call, no draw (may run on the worker thread) -----------------------
    def _host(self, sources):
        """Reads and parses the files of ``sources`` (a flat list of dataset indices) -> ``(bufs, refused, host,
        (read seconds, parse seconds))``: ``refused`` maps positions to the decoder's refusal; ``host`` is the batch's
        ``HostHalf`` when none was."""
        t0 = time.perf_counter()
        bufs = list(self._readers.map(_read, [self._path(j) for j in sources]))
        t1 = time.perf_counter()
        refused = image_io.refusals(bufs)
        host = None
        if not refused:
            host = self._host_half(bufs, sources)
        t2 = time.perf_counter()
        return bufs, refused, host, (t1 - t0, t2 - t1)

    def _named(self, e, sources):
        """The decoder's ``ValueError`` about "image n" of a batch, naming the file."""
        m = re.search(r'image (\d+)', str(e))
        where = self._path(sources[int(m.group(1))]) if m else f'batch of {[self._path(j) for j in sources]}'
        return ValueError(f'{type(self).__name__}: {where}: {e}')

    def _host_half(self, bufs, sources):
        try:
            return image_io.HostHalf(bufs, self.entropy, what=type(self).__name__)
        except ValueError as e:      # a damaged scan found by the host Huffman decode or the segment walk
            raise self._named(e, sources) from None

    def _submit(self, sources):
        """The host work of ``sources``: a future with ``prefetch``, else its result."""
        return self._worker.submit(self._host, list(sources)) if self._worker is not None else self._host(list(sources))

    def _result(self, job):
        return job.result() if self._worker is not None else job

    def _decode(self, bufs, host, sources):
        """ONE ``decode_into`` of the batch -> its (h, w, 3) device views."""
        try:
            out, table = image_io.decode_into(bufs, 'bgr', self._dev(), orientation=self.orientation, host=host)
        except ValueError as e:      # a damaged scan found by the device decode's status read-back
            raise self._named(e, sources) from None
        return image_io.image_views(out, table)

    def _pipelined(self, batches):
        """``_finish(_start(batch))`` per batch; with ``prefetch`` the next batch is started before this one is yielded."""
        started = self._start(batches[0]) if batches else None
        for k in range(len(batches)):
            if self.prefetch:
                data = self._finish(started)
                started = self._start(batches[k + 1]) if k + 1 < len(batches) else None
            else:
                data = self._finish(started if k == 0 else self._start(batches[k]))
            yield data


class TrainLoader(_FileLoader):
    """What ``Runner.data_loader`` and the hooks expect of a loader (``hooks.BatchSource``), fed from image files:
    iterable over ``train_step`` data dicts (``img`` (N, 3, H, W) float32 on the device, ``img_metas``, ``gt_bboxes``,
    ``gt_labels``), with ``__len__`` (batches an epoch), ``.dataset`` and ``.sampler`` (``samples_per_gpu``,
    ``set_epoch``).  An iteration is one epoch; the sampler's epoch then advances by one, and ``set_epoch`` (a resume,
    ``DistSamplerSeedHook``) overrides it.  The same ``(seed, epoch, rank, world)`` gives the same batches bit for bit.

    Per batch: the sampler's indices; for a mosaic pipeline ``dataset.batch_rand_others(idx, 3)`` per sample from the
    epoch's ``RandomState``; the files read on at most ``MAX_READ_THREADS`` threads; every header through
    ``jpeg_parse``; ONE ``image_io.decode_into`` of the whole batch in the ``entropy`` mode asked for; the device views
    into the fused pipeline with the same ``RandomState``.  ``draws`` records the last batch: ``indices``, ``sources``
    (per sample the dataset indices whose files were decoded, after any resampling) and the pipeline's ``params``.

    ``prefetch=1``: one worker thread reads the next batch's files and does the host half of their decode
    (``image_io.HostHalf``: the parses, and with ``entropy='host'`` the Huffman decodes) while the caller runs the step.
    Every HIP and torch call stays on the caller's thread and stream, and every draw on the caller's thread in the
    order above, so the batches equal ``prefetch=0``'s bit for bit.

    ``on_unsupported``: ``'raise'`` -- a file the decoder refuses (progressive, CMYK, another format ...) raises
    ``NotImplementedError`` naming the file; ``'resample'`` -- it is replaced by ``dataset._rand_another(idx)``, the
    rule of the reference's ``__getitem__`` retry (``custom.py:206-211``), logged once per file and counted in
    ``resampled``.  A damaged scan is a ``ValueError`` either way."""

    def __init__(self, dataset, pipeline, samples_per_gpu, seed=0, rank=0, world=1, device=None, entropy=None, prefetch=0,
                 on_unsupported='raise', orientation=True):
        if on_unsupported not in ('raise', 'resample'):
            raise ValueError(f"on_unsupported {on_unsupported!r} is not 'raise' or 'resample'")
        super().__init__(dataset, rank, world, device, entropy, prefetch, orientation)
        self.pipeline = pipeline
        self.mosaic = isinstance(pipeline, FusedTrainPipeline)
        self.seed, self.on_unsupported = int(seed), on_unsupported
        if world == 1:
            self.sampler = GroupSampler(dataset, samples_per_gpu, seed=self.seed)
        else:
            self.sampler = DistributedGroupSampler(dataset, samples_per_gpu, world, rank, seed=self.seed)
        self.resampled = 0
        self._logged = set()
        self.draws = None
        self._rng = None
        #: host seconds of the last epoch by phase (tools/loader_bench.py): index draws, file reads, header parse and
        #: host half, the decode call, the pipeline call
        self.times = dict(draws=0.0, read=0.0, host=0.0, decode=0.0, pipeline=0.0)

    def __len__(self):
        return len(self.sampler) // self.sampler.samples_per_gpu

    def set_epoch(self, epoch):
        self.sampler.set_epoch(epoch)

    def _settle(self, sources, job, rng):
        """The refusals of a batch, on the caller's thread: raise, or draw replacements until every file is accepted."""
        bufs, refused, host, (t_read, t_host) = job
        self.times['read'] += t_read
        self.times['host'] += t_host
        while refused:
            t0 = time.perf_counter()
            for k in sorted(refused):
                path = self._path(sources[k])
                if self.on_unsupported == 'raise':
                    raise NotImplementedError(f'TrainLoader: {path}: {refused[k]}')
                if path not in self._logged:
                    self._logged.add(path)
                    logging.getLogger(__name__).warning('TrainLoader: %s is refused (%s): another image of its group is '
                                                        'drawn in its place', path, refused[k])
                self.resampled += 1
                ds, i = self._at(sources[k])
                sources[k] = self._sibling(sources[k], ds._rand_another(i, rng))
                bufs[k] = _read(self._path(sources[k]))
            drawn = sorted(refused)
            refused = {drawn[i]: e for i, e in image_io.refusals([bufs[k] for k in drawn]).items()}
            if not refused:
                host = self._host_half(bufs, sources)
            self.times['host'] += time.perf_counter() - t0
        return bufs, host

    def _start(self, indices):
        """The draws of a batch's sources (caller's thread), then its host work: a future with ``prefetch``."""
        t0 = time.perf_counter()
        if self.mosaic:
            sources = []
            for idx in indices:
                own = self._own(idx)
                ds, i = self._at(own)          # the partners come from the dataset that owns the sample
                sources += [own] + [self._sibling(own, j) for j in ds.batch_rand_others(i, 3, self._rng)]
        else:
            sources = [self._own(idx) for idx in indices]
        self.times['draws'] += time.perf_counter() - t0
        return indices, sources, self._submit(sources)

    def _finish(self, started):
        indices, sources, job = started
        rng = self._rng
        bufs, host = self._settle(sources, self._result(job), rng)
        t0 = time.perf_counter()
        imgs = self._decode(bufs, host, sources)
        t1 = time.perf_counter()
        anns = [ds.get_ann_info(i) for ds, i in map(self._at, sources)]
        triples = [(im, a['bboxes'], a['labels']) for im, a in zip(imgs, anns)]
        if self.mosaic:
            samples = [tuple(triples[4 * n:4 * n + 4]) for n in range(len(indices))]
        else:
            samples = triples
        res = self.pipeline(samples, rng=rng)
        t2 = time.perf_counter()
        self.times['decode'] += t1 - t0
        self.times['pipeline'] += t2 - t1
        per = 4 if self.mosaic else 1
        groups = [sources[per * n:per * n + per] for n in range(len(indices))]
        self.draws = dict(indices=list(indices), sources=groups, params=res['params'])
        metas = res.get('img_metas')
        if metas is None:
            shape = tuple(res['img'].shape[2:]) + (3,)
            metas = [dict(img_shape=shape, pad_shape=shape, scale_factor=1.0, flip=False) for _ in indices]
        for m, g in zip(metas, groups):
            m['ori_filename'] = self._filename(g[0])
            m['filename'] = self._path(g[0])
        return dict(img=res['img'], img_metas=metas, gt_bboxes=res['gt_bboxes'], gt_labels=res['gt_labels'])

    def __iter__(self):
        epoch = self.sampler.epoch
        self._rng = np.random.RandomState([self.seed, int(epoch), self.rank, 1])
        for k in self.times:
            self.times[k] = 0.0
        order = list(iter(self.sampler))
        n = self.sampler.samples_per_gpu
        yield from self._pipelined([order[i:i + n] for i in range(0, len(order), n)])
        self.sampler.set_epoch(epoch + 1)


#: ``build_test_loader``'s pipeline form: the one-launch batched letterbox (``FusedTestPipeline(batched=True)``), which
#: DESIGN 22 measured as not slower than the per-image path at batch 32
TEST_LOADER_BATCHED = True


class TestLoader(_FileLoader):
    """The test side's loader, what ``single_gpu_test`` / ``multi_gpu_test`` / ``EvalHook`` / ``DistEvalHook`` take, fed
    from image files: iterable over ``dict(img=[batch per augmentation], img_metas=[[meta per image] per augmentation])``
    (the nested form of the reference's test collate), with ``__len__`` (batches) and ``.dataset`` (a dataset in test
    mode -- ``CocoDataset``, one of ``custom_datasets``, a ``ConcatDataset`` of them --, which ``accepts_flat``).

    Order: ``dist.sampler_indices(len(dataset), rank, world)`` -- ``DistributedSampler(shuffle=False)``, for one rank
    ``range(len(dataset))`` -- in consecutive batches of ``samples_per_gpu``, the last one ragged.  Per batch: the files
    read on at most ``MAX_READ_THREADS`` threads, every header parsed, ONE ``image_io.decode_into`` in the ``entropy`` mode
    asked for, the device views into ``pipeline`` (a ``FusedTestPipeline``; with ``batched=True`` ONE launch).  Each meta
    gains ``filename`` and ``ori_filename``.  ``prefetch=1`` as in ``TrainLoader``: the next batch's reads and host half on a
    worker thread, every HIP and torch call on the caller's.

    A file the decoder refuses (progressive, CMYK, another format ...) cannot be replaced by another in a test run: it
    raises ``NotImplementedError`` naming the file, unless ``fallback`` is given -- a callable ``path -> (h, w, 3) uint8
    BGR array`` (``cv2.imread``, say), whose array is uploaded by the pipeline and joins the batch's launch.  A damaged
    scan is a ``ValueError`` naming the file."""

    __test__ = False      # (not a test class, whatever its name says to a collector)

    def __init__(self, dataset, pipeline, samples_per_gpu=1, rank=0, world=1, device=None, entropy=None, prefetch=0,
                 fallback=None, orientation=True):
        if int(samples_per_gpu) < 1:
            raise ValueError(f'samples_per_gpu {samples_per_gpu!r} is not positive')
        if fallback is not None and not callable(fallback):
            raise ValueError('fallback is not callable')
        super().__init__(dataset, rank, world, device, entropy, prefetch, orientation)
        from .dist import sampler_indices
        self.pipeline, self.samples_per_gpu, self.fallback = pipeline, int(samples_per_gpu), fallback
        self.indices = sampler_indices(len(dataset), self.rank, self.world)
        n = self.samples_per_gpu
        self.batches = [self.indices[i:i + n] for i in range(0, len(self.indices), n)]
        #: host seconds of the last pass by phase (tools/test_loader_bench.py): file reads, header parse and host half,
        #: the decode call, the pipeline call
        self.times = dict(read=0.0, host=0.0, decode=0.0, pipeline=0.0)

    def __len__(self):
        return len(self.batches)

    def _start(self, indices):
        sources = [self._own(j) for j in indices]
        return sources, self._submit(sources)

    def _finish(self, started):
        sources, job = started
        bufs, refused, host, (t_read, t_host) = self._result(job)
        self.times['read'] += t_read
        self.times['host'] += t_host
        images = [None] * len(sources)
        if refused:
            t0 = time.perf_counter()
            for k in sorted(refused):
                path = self._path(sources[k])
                if self.fallback is None:
                    raise NotImplementedError(f'TestLoader: {path}: {refused[k]}')
                arr = self.fallback(path)
                if not isinstance(arr, np.ndarray) or arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
                    raise ValueError(f'TestLoader: {path}: fallback must return an (h, w, 3) uint8 array')
                images[k] = arr
            keep = [k for k in range(len(sources)) if k not in refused]
            bufs, sources_dec = [bufs[k] for k in keep], [sources[k] for k in keep]
            host = self._host_half(bufs, sources_dec) if keep else None
            self.times['host'] += time.perf_counter() - t0
        else:
            keep, sources_dec = list(range(len(sources))), sources
        t0 = time.perf_counter()
        if keep:
            for k, im in zip(keep, self._decode(bufs, host, sources_dec)):
                images[k] = im
        t1 = time.perf_counter()
        batch, metas = self.pipeline(images)
        if not isinstance(batch, list):
            batch, metas = [batch], [metas]
        t2 = time.perf_counter()
        self.times['decode'] += t1 - t0
        self.times['pipeline'] += t2 - t1
        for per_aug in metas:
            for m, j in zip(per_aug, sources):
                m['ori_filename'] = self._filename(j)
                m['filename'] = self._path(j)
        return dict(img=list(batch), img_metas=[list(m) for m in metas])

    def __iter__(self):
        for k in self.times:
            self.times[k] = 0.0
        yield from self._pipelined(self.batches)


def _reads_oriented(pipeline):
    """Whether the block's ``LoadImageFromFile`` applies the EXIF orientation, with the reference's meaning:
    ``color_type='color'`` (the default) does, ``'color_ignore_orientation'`` does not; nothing else is built."""
    color_type = 'color'
    stack = list(pipeline)
    while stack:
        t = stack.pop()
        if t['type'] == 'LoadImageFromFile':
            color_type = t.get('color_type', 'color')
        stack += list(t.get('individual_pipeline', ()))
    if color_type not in ('color', 'color_ignore_orientation'):
        raise NotImplementedError(f"LoadImageFromFile(color_type={color_type!r}) is not built ('color' and "
                                  "'color_ignore_orientation' only)")
    return color_type == 'color'


def build_train_loader(cfg, samples_per_gpu, seed=0, rank=0, world=1, device=None, entropy=None, prefetch=0,
                       on_unsupported='raise'):
    """``cfg``: ``cfg.data.train`` of a reference config -- a dataset block with its ``pipeline``, a wrapper around one, or
    a list of blocks (``build_dataset``) -> ``TrainLoader``.  The pipeline block, under a wrapper the innermost dataset's,
    goes through ``build_train_pipeline`` (the mosaic recipes, the YOLOv3 mstrain recipe, the plain ``Resize`` block).  Its
    ``LoadImageFromFile`` says how files are read, with the reference's meaning: ``color_type='color'`` (the default)
    applies the EXIF orientation, ``'color_ignore_orientation'`` does not."""
    dataset = build_dataset(cfg)
    if dataset.pipeline is None:
        raise ValueError('build_train_loader: the dataset block has no pipeline')
    orientation = _reads_oriented(dataset.pipeline)
    pipeline = build_train_pipeline(dataset.pipeline, device=device)
    return TrainLoader(dataset, pipeline, samples_per_gpu, seed=seed, rank=rank, world=world, device=device,
                       entropy=entropy, prefetch=prefetch, on_unsupported=on_unsupported,
                       orientation=orientation)


def build_test_loader(cfg, samples_per_gpu=None, rank=0, world=1, device=None, entropy=None, prefetch=0, fallback=None,
                      batched=None):
    """``cfg``: ``cfg.data.val`` or ``cfg.data.test`` of a reference config, a dataset block with its test ``pipeline``
    (or a wrapper or a list, as ``build_dataset`` takes them) -> ``TestLoader``.  A plain block is built with
    ``test_mode=True`` whatever it says, and the blocks under a wrapper take it as their default (``apis/train.py:140``),
    so no image is filtered.  ``samples_per_gpu``: ``None`` takes the block's own key (the YOLOv4 configs put
    ``samples_per_gpu=8`` into ``val``), else 1; the key never reaches the dataset.  The pipeline block goes through
    ``FusedTestPipeline.from_config`` (a transform it does not build is refused by name), its ``LoadImageFromFile`` decides
    the orientation as in ``build_train_loader``.  ``batched``: the pipeline's form, ``None`` for ``TEST_LOADER_BATCHED``."""
    from .preprocess import FusedTestPipeline
    own = None
    if isinstance(cfg, dict):
        cfg = dict(cfg)
        own = cfg.pop('samples_per_gpu', None)
        if 'ann_file' in cfg:
            cfg['test_mode'] = True
    # under a wrapper or in a list, test_mode reaches every plain block as a default argument (apis/train.py:140)
    dataset = build_dataset(cfg, dict(test_mode=True))
    if samples_per_gpu is None:
        samples_per_gpu = 1 if own is None else own
    if dataset.pipeline is None:
        raise ValueError('build_test_loader: the dataset block has no pipeline')
    orientation = _reads_oriented(dataset.pipeline)
    pipeline = FusedTestPipeline.from_config(dataset.pipeline, device=device,
                                             batched=TEST_LOADER_BATCHED if batched is None else batched)
    return TestLoader(dataset, pipeline, samples_per_gpu, rank=rank, world=world, device=device, entropy=entropy,
                      prefetch=prefetch, fallback=fallback, orientation=orientation)
