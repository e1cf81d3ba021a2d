"""Writes tests/golden/coco_train_set.json (a hand-made COCO annotation file) and tests/golden/coco_train_set.npz: what
the reference's own ``CocoDataset``, ``GroupSampler`` and ``DistributedGroupSampler`` return for it.

Run in the build container only (``python tests/golden/make_golden_coco_train.py``).  The reference's modules
(``mmdet/datasets/coco.py``, ``custom.py``, ``samplers/group_sampler.py``) are executed from the reference tree behind
stand-in modules, in the manner of ``_ref_import.py``: ``mmcv`` / ``terminaltables`` / ``mmdet.core`` shells that only
have to exist, a ``Compose`` that keeps the block, and ``_COCO`` below for ``mmdet.datasets.api_wrappers.COCO``.
pycocotools is absent: ``_COCO`` restates the part of its ``COCO`` class that ``CocoDataset`` calls (``createIndex``'s
``anns`` / ``imgs`` / ``imgToAnns`` / ``catToImgs`` in file order, ``getCatIds`` by name, ``getImgIds``, ``getAnnIds`` of
one image, ``loadAnns`` / ``loadImgs``), so parity with pycocotools itself is unpinned.

The annotation file (IMAGES / ANNS below; classes ``('cat', 'dog')``, the file also lists ``'bird'``, which the dataset
does not): landscape, portrait and square images; image 4 is below 32 pixels; image 5 has no annotation; image 6 only a
crowd box; image 7 only a box of the unlisted category; a box with w < 1, one with area 0, one wholly outside its image,
one partly outside, an ``ignore`` record; the annotations of image 1 are not adjacent in the file.  After filtering
(12 images stay: 4, 5, 7, 16 and 17 go), group 0 (portrait and square) holds three images and group 1 (landscape) nine.

Contents of the npz: ``valid_inds``, ``img_ids``, ``flag``; per index ``bboxes_<i>``, ``labels_<i>``, ``ignore_<i>``;
``others_<seed>`` (len, 3): ``batch_rand_others(idx, 3)`` for every index in turn from ``np.random.seed(seed)``;
``another_<seed>``: ``_rand_another`` likewise; ``bird_*``: the same for ``classes=('bird',)`` -- groups of three and
two images, pools smaller than the batch (drawn with replacement); ``solo_*``: the file cut down to images 7 and 13 with ``classes=('bird',)`` -- two groups of one image
(the ``[idx] * batch`` case);
``group_<seed>_<spg>``: ``GroupSampler`` orders; ``dist_<world>_<rank>_<epoch>``: ``DistributedGroupSampler`` orders
(seed 7, samples_per_gpu 2).

The image files of the set, for the loader's GPU tests (tests/test_gpu_train_loader.py writes them into a directory):
``jpg_<id>``: a Pillow-written baseline JPEG of each image's size (4:2:0, 4:2:2, grayscale and 4:4:4 in turn, the
4:4:4 ones with restart markers); ``jpg_tagged_2``: image 2 (48 x 64 as displayed) stored as a 64 x 48 picture with EXIF
orientation 6; ``jpg_progressive_10``: image 10 as a progressive file, which the decoder refuses.
"""
import importlib
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))

# (id, width, height)
IMAGES = [(1, 64, 48), (2, 48, 64), (3, 40, 40), (4, 31, 64), (5, 64, 48), (6, 64, 48), (7, 48, 64), (8, 70, 50),
          (9, 50, 70), (10, 64, 40), (11, 80, 48), (12, 33, 32), (13, 96, 64), (14, 66, 60), (15, 72, 40), (16, 40, 72),
          (17, 90, 45)]
# (id, image, category, x, y, w, h, area, iscrowd, extra)
ANNS = [
    (1, 1, 1, 4, 5, 20, 18, 360, 0, {}),
    (2, 2, 2, 3.5, 10.25, 30, 40, 1200, 0, {}),
    (3, 3, 1, 1, 1, 10, 10, 100, 0, {}),
    (4, 1, 2, 30, 20, 25.5, 20.5, 522.75, 0, {}),             # image 1 again, not adjacent to annotation 1
    (5, 4, 1, 2, 2, 20, 20, 400, 0, {}),                      # on the image below 32 pixels
    (6, 6, 1, 5, 5, 40, 30, 1200, 1, {}),                     # image 6: only a crowd box
    (7, 7, 3, 5, 5, 20, 20, 400, 0, {}),                      # image 7: only the unlisted category
    (8, 8, 1, 10, 10, 0.5, 20, 10, 0, {}),                    # w < 1
    (9, 8, 2, 12, 8, 30, 30, 0, 0, {}),                       # area 0
    (10, 8, 1, 100, 100, 10, 10, 100, 0, {}),                 # wholly outside
    (11, 8, 2, 60, 40, 30, 30, 900, 0, {}),                   # partly outside: kept as it is
    (12, 8, 1, 5, 5, 20, 20, 400, 0, {'ignore': True}),       # an ignore record
    (13, 8, 1, 20, 15, 22, 18, 396, 1, {}),                   # a crowd box beside kept boxes
    (14, 9, 1, 5, 6, 30, 50, 1500, 0, {}),
    (15, 10, 2, 8, 4, 40, 30, 1200, 0, {}),
    (16, 11, 1, 0, 0, 80, 48, 3840, 0, {}),
    (17, 12, 2, 2, 2, 28, 27, 756, 0, {}),
    (18, 13, 1, 10, 10, 50, 40, 2000, 0, {}),
    (19, 13, 3, 20, 20, 30, 30, 900, 0, {}),                  # the unlisted category beside a listed one
    (20, 1, 1, -3, -2, 10, 10, 100, 0, {}),                   # image 1 a third time; reaches over the corner
    (21, 14, 2, 6, 6, 50, 40, 2000, 0, {}),
    (22, 15, 1, 3, 3, 60, 30, 1800, 0, {}),
    (23, 16, 3, 4, 4, 30, 60, 1800, 0, {}),                   # image 16 and 17: 'bird' only
    (24, 17, 3, 4, 4, 60, 30, 1800, 0, {}),
    (25, 9, 3, 10, 10, 20, 20, 400, 0, {}),                   # with images 7 and 16: three portrait 'bird' images
]


def annotation_file():
    images = [dict(id=i, width=w, height=h, file_name=f'{i:06d}.jpg') for i, w, h in IMAGES]
    anns = []
    for i, img, cat, x, y, w, h, area, crowd, extra in ANNS:
        anns.append(dict(id=i, image_id=img, category_id=cat, bbox=[x, y, w, h], area=area, iscrowd=crowd, **extra))
    cats = [dict(id=1, name='cat'), dict(id=2, name='dog'), dict(id=3, name='bird')]
    return dict(images=images, annotations=anns, categories=cats)


class _COCO:
    """The calls ``CocoDataset`` makes of ``mmdet.datasets.api_wrappers.COCO`` (pycocotools' ``COCO``), restated."""

    def __init__(self, annotation_file=None):
        with open(annotation_file) as f:
            self.dataset = json.load(f)
        self.anns, self.cats, self.imgs = {}, {}, {}
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset['annotations']:
            self.imgToAnns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset['images']:
            self.imgs[img['id']] = img
        for cat in self.dataset['categories']:
            self.cats[cat['id']] = cat
        for ann in self.dataset['annotations']:
            self.catToImgs[ann['category_id']].append(ann['image_id'])
        self.img_ann_map, self.cat_img_map = self.imgToAnns, self.catToImgs

    def get_cat_ids(self, cat_names=[], sup_names=[], cat_ids=[]):
        cats = self.dataset['categories']
        if len(cat_names):
            cats = [c for c in cats if c['name'] in cat_names]
        return [c['id'] for c in cats]

    def get_img_ids(self, img_ids=[], cat_ids=[]):
        return list(self.imgs.keys())

    def get_ann_ids(self, img_ids=[], cat_ids=[], area_rng=[], iscrowd=None):
        return [a['id'] for i in img_ids if i in self.imgToAnns for a in self.imgToAnns[i]]

    def load_anns(self, ids):
        return [self.anns[i] for i in ids]

    def load_imgs(self, ids):
        return [self.imgs[i] for i in ids]


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference():
    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    _mod('mmcv', load=None, list_from_file=None)
    _mod('mmcv.utils', print_log=print)
    _mod('mmcv.runner', get_dist_info=lambda: (0, 1))
    _mod('terminaltables', AsciiTable=None)
    _mod('mmdet').__path__ = [os.path.join(REF, 'mmdet')]
    _mod('mmdet.core', eval_map=None, eval_recalls=None)
    ds = _mod('mmdet.datasets')
    ds.__path__ = [os.path.join(REF, 'mmdet', 'datasets')]
    _mod('mmdet.datasets.builder', DATASETS=_Registry())
    _mod('mmdet.datasets.pipelines', Compose=lambda pipeline: pipeline)
    _mod('mmdet.datasets.api_wrappers', COCO=_COCO, COCOeval=None)
    _mod('mmdet.datasets.samplers').__path__ = [os.path.join(REF, 'mmdet', 'datasets', 'samplers')]
    coco = importlib.import_module('mmdet.datasets.coco')
    samplers = importlib.import_module('mmdet.datasets.samplers.group_sampler')
    return coco.CocoDataset, samplers.GroupSampler, samplers.DistributedGroupSampler


def image_files(out):
    import io
    from PIL import Image, features
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'

    def picture(h, w, seed):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        grad = np.stack([255 * xx / (w - 1), 255 * yy / (h - 1), 255 * (xx + yy) / (h + w - 2)], -1)
        return np.clip(grad + (rng.integers(0, 256, (h, w, 3)) - 128) * 0.3, 0, 255).astype(np.uint8)

    def save(im, **kw):
        buf = io.BytesIO()
        im.save(buf, 'JPEG', quality=90, **kw)
        return np.frombuffer(buf.getvalue(), np.uint8)

    for k, (i, w, h) in enumerate(IMAGES):
        im = Image.fromarray(picture(h, w, 200 + i))
        kw = dict(restart_marker_blocks=2) if k % 4 == 3 else {}
        out[f'jpg_{i}'] = save(im.convert('L'), **kw) if k % 4 == 2 else save(im, subsampling=(2, 1, None, 0)[k % 4], **kw)
    exif = Image.Exif()
    exif[0x0112] = 6
    out['jpg_tagged_2'] = save(Image.fromarray(picture(48, 64, 300)), subsampling=2, exif=exif.tobytes())
    out['jpg_progressive_10'] = save(Image.fromarray(picture(40, 64, 301)), subsampling=2, progressive=True)


def draws(ds, out, prefix):
    for seed in (0, 1, 2):
        np.random.seed(seed)
        out[f'{prefix}others_{seed}'] = np.stack([ds.batch_rand_others(i, 3) for i in range(len(ds))]).astype(np.int64)
        np.random.seed(seed)
        out[f'{prefix}another_{seed}'] = np.array([ds._rand_another(i) for i in range(len(ds))], np.int64)


def main():
    path = os.path.join(HERE, 'coco_train_set.json')
    with open(path, 'w') as f:
        json.dump(annotation_file(), f, indent=1)
    CocoDataset, GroupSampler, DistributedGroupSampler = import_reference()
    out = {}
    ds = CocoDataset(path, pipeline=[], classes=('cat', 'dog'))
    out['valid_inds'] = np.array([i for i, (img, _, _) in enumerate(IMAGES) if img in ds.img_ids], np.int64)
    out['img_ids'] = np.array(ds.img_ids, np.int64)
    out['flag'] = ds.flag
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        out[f'bboxes_{i}'], out[f'labels_{i}'], out[f'ignore_{i}'] = ann['bboxes'], ann['labels'], ann['bboxes_ignore']
    draws(ds, out, '')
    for seed in (3, 4):
        for spg in (2, 3):      # 2 divides neither group (3 and 9 images), 3 both
            np.random.seed(seed)
            out[f'group_{seed}_{spg}'] = np.array(list(GroupSampler(ds, spg)), np.int64)
            assert len(out[f'group_{seed}_{spg}']) == len(GroupSampler(ds, spg))
    for world in (1, 2, 3):
        for rank in range(world):
            s = DistributedGroupSampler(ds, 2, world, rank, seed=7)
            for epoch in (0, 1):
                s.set_epoch(epoch)
                out[f'dist_{world}_{rank}_{epoch}'] = np.array(list(s), np.int64)
                assert len(out[f'dist_{world}_{rank}_{epoch}']) == len(s)
    # no filtering: every image, in file order
    everything = CocoDataset(path, pipeline=[], classes=('cat', 'dog'), filter_empty_gt=False)
    out['unfiltered_img_ids'] = np.array(everything.img_ids, np.int64)
    # classes=('bird',): images 7, 9, 16 (portrait) are group 0, 13 and 17 group 1
    bird = CocoDataset(path, pipeline=[], classes=('bird',))
    out['bird_img_ids'] = np.array(bird.img_ids, np.int64)
    out['bird_flag'] = bird.flag
    draws(bird, out, 'bird_')
    # one-image groups: the file cut down to images 7 and 13 (written beside the fixture for the run, then removed)
    solo = annotation_file()
    solo['images'] = [im for im in solo['images'] if im['id'] in (13, 7)]
    solo['annotations'] = [a for a in solo['annotations'] if a['image_id'] in (13, 7)]
    solo_path = os.path.join(HERE, 'coco_train_solo.json')
    with open(solo_path, 'w') as f:
        json.dump(solo, f, indent=1)
    one = CocoDataset(solo_path, pipeline=[], classes=('bird',))
    out['solo_img_ids'] = np.array(one.img_ids, np.int64)
    out['solo_flag'] = one.flag
    draws(one, out, 'solo_')
    os.remove(solo_path)
    image_files(out)
    np.savez_compressed(os.path.join(HERE, 'coco_train_set.npz'), **out)
    print('img_ids', ds.img_ids, 'flag', ds.flag.tolist())
    print('bird', bird.img_ids, bird.flag.tolist(), 'solo', one.img_ids, one.flag.tolist())
    print(f'{len(out)} arrays -> coco_train_set.npz')


if __name__ == '__main__':
    main()
