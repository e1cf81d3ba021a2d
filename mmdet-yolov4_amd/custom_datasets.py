"""Datasets beyond COCO under the reference's names: ``CustomDataset`` (the middle-format pickle or json), ``XMLDataset``
/ ``VOCDataset`` (VOC XML trees), ``TrafficSignDataset`` (the traffic-sign recipe's ``*.circle`` folders) and
``GarbageDataset``.

Each restates its class of ``mmdet/datasets`` (``custom.py:56-337``, ``xml_style.py``, ``voc.py``,
``tencent_traffic.py``, ``garbage.py``) on top of ``results.CustomBBoxDataset``, so that ``accepts_flat`` and the cached
``MapGt`` / ``RecallGt`` are inherited and an evaluation hook scores the flat GPU table.  The ground-truth tables are
built on first use: a training dataset never pays for them.  ``pipeline`` is kept as the config block
(``build_train_loader`` / ``build_test_loader`` build the fused pipelines from it).

What is pinned against the reference's own classes (tests/golden/custom_sets.npz): the tables per index, the group
flags, the filtered indices, ``_rand_another`` / ``batch_rand_others`` draw for draw, and ``evaluate``.  The stated
difference: ``TrafficSignDataset`` takes the files of its folder in sorted name order (the reference takes ``glob``'s,
which is the file system's), because "same seed, same batches" needs one order.
"""
import copy
import glob
import json
import os.path as osp
import pickle
import warnings
import xml.etree.ElementTree as ET

import numpy as np

from .map_eval import MapGt, evaluate_map
from .registry import DATASETS
from .results import CustomBBoxDataset


def list_from_file(filename):
    """``mmcv.list_from_file`` with its defaults: the lines without their line ends."""
    with open(filename, 'r', encoding='utf-8') as f:
        return [line.rstrip('\n\r') for line in f]


@DATASETS.register_module()
class CustomDataset(CustomBBoxDataset):
    """``CustomDataset`` of the reference (``custom.py:56-337``) for box work.  ``ann_file``: the middle format, a list
    of ``dict(filename, width, height, ann=dict(bboxes, labels[, bboxes_ignore, labels_ignore]))``, as ``.pkl`` or
    ``.json``.  ``classes``: names, a file of names (one a line) or ``None`` for the class's own.  ``proposal_file`` and
    ``seg_prefix`` are accepted as ``None`` only."""

    CLASSES = None

    def __init__(self, ann_file, pipeline=None, classes=None, data_root=None, img_prefix='', seg_prefix=None,
                 proposal_file=None, test_mode=False, filter_empty_gt=True):
        if seg_prefix is not None:
            raise NotImplementedError(f'{type(self).__name__}(seg_prefix={seg_prefix!r}) is not built: box work only')
        if proposal_file is not None:
            raise NotImplementedError(f'{type(self).__name__}(proposal_file={proposal_file!r}) is not built: no detector '
                                      'of this package takes proposals')
        self.ann_file, self.data_root, self.img_prefix = ann_file, data_root, img_prefix
        self.seg_prefix, self.proposal_file, self.proposals = None, None, None
        self.test_mode, self.filter_empty_gt = test_mode, filter_empty_gt
        self.CLASSES = self.get_classes(classes)
        if self.data_root is not None:                                     # custom.py:76-80
            if not osp.isabs(self.ann_file):
                self.ann_file = osp.join(self.data_root, self.ann_file)
            if not (self.img_prefix is None or osp.isabs(self.img_prefix)):
                self.img_prefix = osp.join(self.data_root, self.img_prefix)
        self._reset_gt()
        self.data_infos = self.load_annotations(self.ann_file)
        if not test_mode:
            valid_inds = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid_inds]
            self.valid_inds = valid_inds
            self._set_group_flag()
        self.pipeline = pipeline

    def __len__(self):
        return len(self.data_infos)

    # ---- the ground truth of evaluate, built on first use (CustomBBoxDataset builds its own in __init__) -----------------
    def _reset_gt(self):
        self._annotations, self._map_gt, self._recall_gt = None, None, None

    @property
    def annotations(self):
        if self._annotations is None:
            self._annotations = [self.get_ann_info(i) for i in range(len(self))]
        return self._annotations

    @property
    def map_gt(self):
        if self._map_gt is None:
            self._map_gt = MapGt(self.annotations, len(self.CLASSES))
        return self._map_gt

    def load_annotations(self, ann_file):
        """``custom.py:111-113`` (``mmcv.load``): a pickle or a json by the file's extension."""
        ext = osp.splitext(ann_file)[1].lower()
        if ext in ('.pkl', '.pickle'):
            with open(ann_file, 'rb') as f:
                return pickle.load(f)
        if ext == '.json':
            with open(ann_file) as f:
                return json.load(f)
        raise NotImplementedError(f'{type(self).__name__}: annotation file {ann_file!r}: only .pkl / .pickle and .json '
                                  'are built')

    def get_ann_info(self, idx):
        return self.data_infos[idx]['ann']

    def get_cat_ids(self, idx):
        """``custom.py:131-141`` with ``int`` for the reference's ``np.int`` (gone from numpy)."""
        return np.asarray(self.data_infos[idx]['ann']['labels']).astype(int).tolist()

    def _filter_imgs(self, min_size=32):
        """``custom.py:153-162``: images whose shorter side is below ``min_size`` go; empty images stay, with the
        reference's warning."""
        if self.filter_empty_gt:
            warnings.warn('CustomDataset does not support filtering empty gt images.')
        return [i for i, img_info in enumerate(self.data_infos)
                if min(img_info['width'], img_info['height']) >= min_size]

    def _set_group_flag(self):
        """``custom.py:164-174``."""
        self.flag = np.zeros(len(self), dtype=np.uint8)
        for i in range(len(self)):
            img_info = self.data_infos[i]
            if img_info['width'] / img_info['height'] > 1:
                self.flag[i] = 1

    def _rand_another(self, idx, rng=np.random):
        """``custom.py:176-179``, drawing from ``rng`` (the same call as ``CocoDataset``'s)."""
        pool = np.where(self.flag == self.flag[idx])[0]
        return rng.choice(pool)

    def batch_rand_others(self, idx, batch, rng=np.random):
        """``custom.py:181-191``, draw for draw (the same calls as ``CocoDataset``'s)."""
        mask = (self.flag == self.flag[idx])
        mask[idx] = False
        pool = np.where(mask)[0]
        if len(pool) == 0:
            return np.array([idx] * batch)
        if len(pool) < batch:
            return rng.choice(pool, size=batch, replace=True)
        return rng.choice(pool, size=batch, replace=False)

    @classmethod
    def get_classes(cls, classes=None):
        """``custom.py:250-275``: ``None`` -> the class's names; a string -> the lines of that file; a tuple or list."""
        if classes is None:
            return cls.CLASSES
        if isinstance(classes, str):
            return list_from_file(classes)
        if isinstance(classes, (tuple, list)):
            return classes
        raise ValueError(f'Unsupported type {type(classes)} of classes.')

    def format_results(self, results, **kwargs):
        """Place holder, as the reference's."""

    _ap_dataset = None      # evaluate_map's `classes`: None for the class names, or a dataset name such as 'voc07'

    def evaluate(self, results, metric='mAP', logger=None, proposal_nums=(100, 300, 1000), iou_thr=0.5,
                 scale_ranges=None):
        """``custom.py:280-337``: ``'mAP'`` through ``evaluate_map`` (``AP50``-style keys and ``mAP``), ``'recall'``
        through ``eval_recalls`` (``recall@{num}@{iou}`` and, with several thresholds, ``AR@{num}``).  ``results``:
        the per-image lists or the flat tuple of GPU tensors, ``img_index`` being positions in ``data_infos``."""
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric not in ('mAP', 'recall'):
            raise KeyError(f'metric {metric} is not supported')
        if metric == 'recall':
            return self.eval_recalls(results, proposal_nums=proposal_nums, iou_thr=iou_thr, logger=logger)
        classes = self._ap_dataset if self._ap_dataset is not None else list(self.CLASSES)
        return evaluate_map(results, self.map_gt, classes=classes, iou_thr=iou_thr, scale_ranges=scale_ranges,
                            logger=logger, metric=metric)

    def __repr__(self):
        return (f'\n{self.__class__.__name__} {"Test" if self.test_mode else "Train"} dataset with number of images '
                f'{len(self)}')


@DATASETS.register_module()
class XMLDataset(CustomDataset):
    """``xml_style.py``: ``ann_file`` lists image ids; image ``i`` is ``JPEGImages/<i>.jpg`` and its annotation
    ``Annotations/<i>.xml`` under ``img_prefix``.  ``min_size``: boxes narrower or lower go to the ignore fields.  An
    XML file without ``<size>`` takes the size from the JPEG's header (``yv4_jpeg_parse``, as stored: no EXIF turn,
    like the reference's ``Image.open(...).size``)."""

    def __init__(self, min_size=None, **kwargs):
        assert self.CLASSES or kwargs.get('classes', None), 'CLASSES in `XMLDataset` can not be None.'
        self._xml = {}
        super().__init__(**kwargs)
        self.cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        self.min_size = min_size

    def _root(self, img_id):
        """The parsed ``Annotations/<img_id>.xml`` (kept: the reference parses it again at every use)."""
        if img_id not in self._xml:
            self._xml[img_id] = ET.parse(osp.join(self.img_prefix, 'Annotations', f'{img_id}.xml')).getroot()
        return self._xml[img_id]

    def load_annotations(self, ann_file):
        """``xml_style.py:29-59``."""
        data_infos = []
        for img_id in list_from_file(ann_file):
            size = self._root(img_id).find('size')
            if size is not None:
                width, height = int(size.find('width').text), int(size.find('height').text)
            else:
                from .image_io import jpeg_parse
                with open(osp.join(self.img_prefix, 'JPEGImages', f'{img_id}.jpg'), 'rb') as f:
                    info = jpeg_parse(f.read())
                width, height = int(info.width), int(info.height)
            data_infos.append(dict(id=img_id, filename=f'JPEGImages/{img_id}.jpg', width=width, height=height))
        return data_infos

    def _filter_imgs(self, min_size=32):
        """``xml_style.py:61-80``: too small, or (``filter_empty_gt``) without an object of a listed class."""
        valid_inds = []
        for i, img_info in enumerate(self.data_infos):
            if min(img_info['width'], img_info['height']) < min_size:
                continue
            if self.filter_empty_gt:
                for obj in self._root(img_info['id']).findall('object'):
                    if obj.find('name').text in self.CLASSES:
                        valid_inds.append(i)
                        break
            else:
                valid_inds.append(i)
        return valid_inds

    def get_ann_info(self, idx):
        """``xml_style.py:82-146``: ``int(float(text))`` corners minus one; ``difficult`` objects and, with
        ``min_size``, small ones go to ``bboxes_ignore`` / ``labels_ignore``; float32 boxes and int64 labels."""
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for obj in self._root(self.data_infos[idx]['id']).findall('object'):
            name = obj.find('name').text
            if name not in self.CLASSES:
                continue
            label = self.cat2label[name]
            difficult = obj.find('difficult')
            difficult = 0 if difficult is None else int(difficult.text)
            bnd_box = obj.find('bndbox')
            bbox = [int(float(bnd_box.find(k).text)) for k in ('xmin', 'ymin', 'xmax', 'ymax')]
            ignore = False
            if self.min_size:
                assert not self.test_mode
                if bbox[2] - bbox[0] < self.min_size or bbox[3] - bbox[1] < self.min_size:
                    ignore = True
            if difficult or ignore:
                bboxes_ignore.append(bbox)
                labels_ignore.append(label)
            else:
                bboxes.append(bbox)
                labels.append(label)
        if not bboxes:
            bboxes, labels = np.zeros((0, 4)), np.zeros((0, ))
        else:
            bboxes, labels = np.array(bboxes, ndmin=2) - 1, np.array(labels)
        if not bboxes_ignore:
            bboxes_ignore, labels_ignore = np.zeros((0, 4)), np.zeros((0, ))
        else:
            bboxes_ignore, labels_ignore = np.array(bboxes_ignore, ndmin=2) - 1, np.array(labels_ignore)
        return dict(bboxes=bboxes.astype(np.float32), labels=labels.astype(np.int64),
                    bboxes_ignore=bboxes_ignore.astype(np.float32), labels_ignore=labels_ignore.astype(np.int64))

    def get_cat_ids(self, idx):
        """``xml_style.py:148-170``: the labels of every listed object, difficult ones included."""
        return [self.cat2label[obj.find('name').text] for obj in self._root(self.data_infos[idx]['id']).findall('object')
                if obj.find('name').text in self.CLASSES]


@DATASETS.register_module()
class VOCDataset(XMLDataset):
    """``voc.py``: the twenty VOC names; the year is read from ``img_prefix``; ``evaluate`` scores ``'mAP'`` with the
    11-point form for 2007 and the area form otherwise, always without scale ranges."""

    CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
               'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if 'VOC2007' in self.img_prefix:
            self.year = 2007
        elif 'VOC2012' in self.img_prefix:
            self.year = 2012
        else:
            raise ValueError('Cannot infer dataset year from img_prefix')
        self._ap_dataset = 'voc07' if self.year == 2007 else None

    def evaluate(self, results, metric='mAP', logger=None, proposal_nums=(100, 300, 1000), iou_thr=0.5,
                 scale_ranges=None):
        """``voc.py:27-93`` (``scale_ranges`` is accepted and unused, as there)."""
        return super().evaluate(results, metric=metric, logger=logger, proposal_nums=proposal_nums, iou_thr=iou_thr,
                                scale_ranges=None)


@DATASETS.register_module()
class TrafficSignDataset(CustomDataset):
    """``tencent_traffic.py``: ``ann_file`` is a folder of ``<name>.circle`` files, one box a line as ``a,b,c,d,x,y,w,h``
    (rows with ``w <= 0`` or ``h <= 0`` are dropped); image ``<name>.jpg`` lies under ``img_prefix``.  A folder without
    ``.circle`` files is the test phase's image folder: one pseudo annotation (empty lists) per ``*.jpg``.
    ``difficulty_thresh``: every box has difficulty 0, so a threshold of 0 or less sends all of them to the ignore
    fields.  ``data_infos`` carry no ``width`` / ``height``: every image is group 0, and training keeps the images
    that have a label.  Files are taken in sorted name order (the reference: ``glob``'s order)."""

    CLASSES = ('sign',)

    def __init__(self, *args, **kwargs):
        self.difficulty_thresh = kwargs.pop('difficulty_thresh', 100)
        super().__init__(*args, **kwargs)

    def load_annotations(self, ann_folder):
        """``tencent_traffic.py:19-96``."""
        ann_files = sorted(glob.glob(ann_folder + '/*.circle'))
        data_infos = []
        if not ann_files:
            for ann_file in sorted(glob.glob(ann_folder + '/*.jpg')):
                data_infos.append(dict(filename=osp.split(ann_file)[1][:-4] + '.jpg', ann=dict(bboxes=[], labels=[])))
        for ann_file in ann_files:
            gt_bboxes, gt_labels, gt_bboxes_ignore, gt_labels_ignore = [], [], [], []
            with open(ann_file) as f:
                for line in f.readlines():
                    x, y, w, h = [float(v) for v in line.strip().split(',')[4:]]
                    if w <= 0 or h <= 0:
                        continue
                    bbox, difficulty, label = [x, y, x + w, y + h], 0, 0
                    if difficulty >= self.difficulty_thresh:
                        gt_labels_ignore.append(label)
                        gt_bboxes_ignore.append(bbox)
                    else:
                        gt_labels.append(label)
                        gt_bboxes.append(bbox)
            ann = dict()
            if gt_bboxes:
                ann['bboxes'], ann['labels'] = np.array(gt_bboxes, dtype=np.float32), np.array(gt_labels, dtype=np.int64)
            else:
                ann['bboxes'], ann['labels'] = np.zeros((0, 4), dtype=np.float32), np.array([], dtype=np.int64)
            if gt_bboxes_ignore:
                ann['bboxes_ignore'] = np.array(gt_bboxes_ignore, dtype=np.float32)
                ann['labels_ignore'] = np.array(gt_labels_ignore, dtype=np.int64)
            else:
                ann['bboxes_ignore'] = np.zeros((0, 4), dtype=np.float32)
                ann['labels_ignore'] = np.array([], dtype=np.int64)
            data_infos.append(dict(filename=osp.split(ann_file)[1][:-7] + '.jpg', ann=ann))
        self.img_ids = [d['filename'][:-4] for d in data_infos]
        return data_infos

    def _filter_imgs(self):
        """``tencent_traffic.py:98-104``: images without a label go."""
        return [i for i, d in enumerate(self.data_infos) if d['ann']['labels'].size > 0]

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)


@DATASETS.register_module()
class GarbageDataset(CustomDataset):
    """``garbage.py``: ``CustomDataset`` whose ``get_ann_info`` returns a deep copy; with ``class_agnostic`` the one
    class is ``'x'`` and the copy's ``labels`` / ``labels_ignore`` are zeroed."""

    def __init__(self, ann_file, pipeline=None, classes=None, data_root=None, img_prefix='', seg_prefix=None,
                 proposal_file=None, test_mode=False, filter_empty_gt=True, class_agnostic=False):
        self.class_agnostic = class_agnostic
        if self.class_agnostic:
            classes = ['x']
        super().__init__(ann_file=ann_file, pipeline=pipeline, classes=classes, data_root=data_root,
                         img_prefix=img_prefix, seg_prefix=seg_prefix, proposal_file=proposal_file, test_mode=test_mode,
                         filter_empty_gt=filter_empty_gt)

    def get_ann_info(self, idx):
        ret = copy.deepcopy(self.data_infos[idx]['ann'])
        if self.class_agnostic:
            ret['labels'] *= 0
            ret['labels_ignore'] *= 0
        return ret
