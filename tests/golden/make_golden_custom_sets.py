"""Writes the fixtures of the datasets beyond COCO: ``tests/golden/custom_sets.npz`` (what the reference's own classes
return), ``tests/golden/custom_sets_recipe.json`` (the traffic-sign recipe's settings, parsed) and the hand-made sources
under ``tests/golden/custom_sets/`` as data only -- two middle-format pickles, a VOC tree of XML files and id lists, and
a folder of ``.circle`` files.

Run in the build container only (``python tests/golden/make_golden_custom_sets.py``).  The reference's ``custom.py``,
``xml_style.py``, ``voc.py``, ``tencent_traffic.py``, ``garbage.py``, ``dataset_wrappers.py``, ``builder.py`` and
``samplers/group_sampler.py`` are executed from the reference tree behind stand-in modules, in the manner of
``make_golden_coco_train.py``; the offset and label logic of the root ``tencent_image_split.py`` likewise.  The stand-ins
carry no arithmetic: ``mmcv.load`` / ``list_from_file``, a registry, a ``Compose`` that keeps the block, ``np.int = int``
(gone from numpy 2), ``make_golden_coco_train._COCO`` (only so that ``dataset_wrappers`` can import ``CocoDataset``), a
``cv2`` whose ``imread`` returns zeros of the source's shape and whose ``imwrite`` records its calls, and a ``skimage.io``
that reads nothing.  ``mmdet.core.eval_map`` / ``eval_recalls`` are the reference's own, imported as
``make_golden_map.py`` and ``make_golden_recall.py`` import them.  ``TrafficSignDataset`` is run with ``glob.glob``
sorted: the package takes the files in sorted name order (its one stated difference), the reference in the file system's.

The sources (all hand-made here):
* ``middle_a.pkl``: 12 images, classes ``('a', 'b', 'c')``, landscape, portrait and square; image 3 is below 32 pixels,
  image 4 has no boxes, some carry ignored boxes.  ``middle_b.pkl``: 5 images, for the ``ConcatDataset`` cases.
* ``VOC2007`` (5 XML files) and ``VOC2012`` (3): 000003 has no ``<size>`` (its JPEG is 48 x 64), 000002 a difficult
  object and float coordinates, 000004 only an unlisted class, 000005 is 30 pixels wide, 2012_000002 holds the only
  ``cat`` (the rare class of the ``ClassBalancedDataset`` cases) and a box below ``min_size=8``.
* ``circle/``: 8 files; t03 has a ``w <= 0`` row beside a kept one, t05 is empty, t06 holds a ``h <= 0`` row only.

Contents of the npz, per dataset prefix ``P`` (``ca`` / ``cb``: the pickles; ``v07`` / ``v12``: the VOC sets; ``v12m``:
VOC2012 with ``min_size=8``; ``ts``: the circle folder; ``ts0``: ``difficulty_thresh=0``; ``tst``: the test phase over the
image folder; ``ga``: ``GarbageDataset(class_agnostic=True)`` on ``middle_a``): ``P/names`` (the surviving file names),
``P/flag``, per index ``P/bboxes_i`` ``P/labels_i`` ``P/bboxes_ignore_i`` ``P/labels_ignore_i``, ``P/cats_i``
(``get_cat_ids``), ``P/others_<seed>`` and ``P/another_<seed>`` (draws from ``np.random.seed(seed)``); ``v07/wh``.
Wrappers: ``W/len``, ``W/flag``, ``W/cats_i`` for every nesting form ``W`` of ``WRAPPER_FORMS``; ``group_<W>_<seed>``:
``GroupSampler(W, 2)`` orders; ``cbd_<thr>/repeat_indices`` and ``/flag``.  ``det_<P>/dets|labels|img_index``: fixed
detections (distinct scores) and ``eval_<P>/<case>/<key>``: what ``evaluate`` returns for them.  ``split/<source>/...``:
the split tool's tile names, offsets, shapes and label files.  ``jpg/<name>``: Pillow-written baseline JPEGs.
"""
import importlib
import importlib.util
import io
import json
import os
import pickle
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import as R  # noqa: E402
from _custom_sets_data import (CLASSES_ABC, EVAL_CASES, SEEDS, SRC, WRAPPER_FORMS, as_lists, as_proposals,  # noqa: E402
                               circle_block, fill, plain_blocks, write_tree)

# ---- the hand-made sources ---------------------------------------------------------------------------------------------
# (width, height) of the images of middle_a.pkl
SIZES_A = [(64, 48), (48, 64), (40, 40), (31, 64), (64, 48), (70, 50), (50, 70), (80, 48), (33, 32), (96, 64), (66, 60),
           (72, 40)]
SIZES_B = [(64, 48), (48, 64), (80, 48), (50, 70), (40, 40)]

VOC = {
    'VOC2007': {
        '000001': dict(size=(64, 48), objects=[('person', 0, 5, 6, 30, 40), ('dog', 0, 20, 10, 60, 44)]),
        '000002': dict(size=(48, 64), objects=[('person', 1, 4, 4, 20, 30), ('person', 0, '10.7', '12.2', '40.9', '60.5'),
                                               ('unicorn', 0, 1, 1, 9, 9)]),
        '000003': dict(size=None, jpeg=(48, 64), objects=[('dog', 0, 3, 3, 40, 50)]),
        '000004': dict(size=(64, 48), objects=[('unicorn', 0, 5, 5, 30, 30)]),
        '000005': dict(size=(30, 50), objects=[('person', 0, 2, 2, 20, 40)]),
    },
    'VOC2012': {
        '2012_000001': dict(size=(80, 48), objects=[('person', 0, 10, 5, 50, 40), ('person', 0, 40, 10, 76, 44)]),
        '2012_000002': dict(size=(64, 64), objects=[('cat', 0, 8, 8, 50, 50), ('person', 0, 30, 30, 36, 60),
                                                    ('person', None, 2, 2, 30, 30)]),
        '2012_000003': dict(size=(40, 60), objects=[('person', 1, 5, 5, 30, 50), ('dog', 0, 6, 20, 36, 58)]),
    },
}

CIRCLE = {
    't00': (64, 64, ['0,s,x,1,10,12,20,18\n', '1,s,x,1,30.5,28.25,16,22\n']),
    't01': (64, 64, ['0,s,y,0,5,5,40,40\n']),
    't02': (80, 64, ['0,s,x,1,50,10,24,30\n', '1,s,z,1,4,30,20,20\n', '2,s,z,0,30,2,12,12\n']),
    't03': (64, 64, ['0,s,x,1,12,12,0,9\n', '1,s,x,1,20,22,30,28\n']),
    't04': (64, 80, ['0,s,x,1,8,40,44,30\n']),
    't05': (64, 64, []),
    't06': (64, 64, ['0,s,x,1,12,12,10,-1\n']),
    't07': (64, 64, ['0,s,q,2,2,3,58,56\n', '1,s,q,2,24,24,14,14\n']),
}

# (name, width, height, label rows) of the split tool's sources; tile (64, 48), overlap (16, 16)
SPLIT_SOURCES = [
    ('big', 100, 70, ['0,s,x,1,5,5,10,10\n', '1,s,y,0,60.9,40.2,20,20\n', '2,s,z,1,90,60,8,8\n', '3,s,z,1,47,30,2,2\n']),
    ('fit', 64, 48, ['0,s,x,1,10,10,20,20\n', '1,s,x,1,62,46,2,2\n']),
    ('small', 40, 30, ['0,s,x,1,4,4,10,10\n']),
]
SPLIT_TILE, SPLIT_OVERLAP = (64, 48), (16, 16)


def _boxes(rng, n, w, h):
    x1, y1 = rng.uniform(0, w * 0.6, n), rng.uniform(0, h * 0.6, n)
    bw, bh = rng.uniform(6, w * 0.4, n), rng.uniform(6, h * 0.4, n)
    return np.round(np.stack([x1, y1, x1 + bw, y1 + bh], 1) * 4).astype(np.float32) / 4


def middle_format(sizes, seed, prefix):
    rng = np.random.default_rng(seed)
    infos = []
    for i, (w, h) in enumerate(sizes):
        n = 0 if (prefix == 'a' and i == 4) else int(rng.integers(1, 4))
        k = int(rng.integers(0, 2)) if i % 3 == 0 else 0
        ann = dict(bboxes=_boxes(rng, n, w, h).reshape(-1, 4), labels=rng.integers(0, 3, n).astype(np.int64),
                   bboxes_ignore=_boxes(rng, k, w, h).reshape(-1, 4), labels_ignore=rng.integers(0, 3, k).astype(np.int64))
        infos.append(dict(filename=f'{prefix}{i:02d}.jpg', width=w, height=h, ann=ann))
    return infos


def write_sources():
    if os.path.isdir(SRC):
        shutil.rmtree(SRC)
    os.makedirs(SRC)
    for name, sizes, seed in (('a', SIZES_A, 11), ('b', SIZES_B, 12)):
        with open(os.path.join(SRC, f'middle_{name}.pkl'), 'wb') as f:
            pickle.dump(middle_format(sizes, seed, name), f, protocol=4)
    with open(os.path.join(SRC, 'classes_abc.txt'), 'w') as f:
        f.write('\n'.join(CLASSES_ABC) + '\n')
    for year, files in VOC.items():
        os.makedirs(os.path.join(SRC, year, 'Annotations'))
        os.makedirs(os.path.join(SRC, year, 'ImageSets', 'Main'))
        with open(os.path.join(SRC, year, 'ImageSets', 'Main', 'trainval.txt'), 'w') as f:
            f.write('\n'.join(files) + '\n')
        for img_id, d in files.items():
            xml = ['<annotation>', f'  <filename>{img_id}.jpg</filename>']
            if d['size'] is not None:
                xml.append(f'  <size><width>{d["size"][0]}</width><height>{d["size"][1]}</height><depth>3</depth></size>')
            for name, difficult, x1, y1, x2, y2 in d['objects']:
                diff = '' if difficult is None else f'<difficult>{difficult}</difficult>'
                xml.append(f'  <object><name>{name}</name>{diff}<bndbox><xmin>{x1}</xmin><ymin>{y1}</ymin><xmax>{x2}</xmax>'
                           f'<ymax>{y2}</ymax></bndbox></object>')
            xml.append('</annotation>')
            with open(os.path.join(SRC, year, 'Annotations', f'{img_id}.xml'), 'w') as f:
                f.write('\n'.join(xml) + '\n')
    os.makedirs(os.path.join(SRC, 'circle'))
    for name, (_, _, rows) in CIRCLE.items():
        with open(os.path.join(SRC, 'circle', f'{name}.circle'), 'w') as f:
            f.writelines(rows)


def image_files(out):
    """``jpg/<name>``: every source image as a Pillow-written baseline JPEG of its size (samplings in turn)."""
    from PIL import Image, features
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'

    def picture(h, w, seed):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        grad = np.stack([255 * xx / (w - 1), 255 * yy / (h - 1), 255 * (xx + yy) / (h + w - 2)], -1)
        return np.clip(grad + (rng.integers(0, 256, (h, w, 3)) - 128) * 0.3, 0, 255).astype(np.uint8)

    todo = [(f'a{i:02d}', w, h) for i, (w, h) in enumerate(SIZES_A)] + [(f'b{i:02d}', w, h) for i, (w, h) in enumerate(SIZES_B)]
    for files in VOC.values():
        todo += [(img_id,) + tuple(d['size'] or d['jpeg']) for img_id, d in files.items()]
    todo += [(name, w, h) for name, (w, h, _) in CIRCLE.items()]
    todo += [(f'split_{name}', w, h) for name, w, h, _ in SPLIT_SOURCES]
    for k, (name, w, h) in enumerate(todo):
        buf = io.BytesIO()
        Image.fromarray(picture(h, w, 500 + k)).save(buf, 'JPEG', quality=90, subsampling=(2, 1, 0)[k % 3])
        out[f'jpg/{name}'] = np.frombuffer(buf.getvalue(), np.uint8)
    return {name: (w, h) for name, w, h in todo}


# ---- the reference behind stand-ins ------------------------------------------------------------------------------------
def _load(path):
    if path.endswith('.json'):
        with open(path) as f:
            return json.load(f)
    with open(path, 'rb') as f:
        return pickle.load(f)


def _list_from_file(path):
    with open(path) as f:
        return [line.rstrip('\n\r') for line in f]


def import_reference():
    from make_golden_coco_train import _COCO
    from make_golden_map import import_reference_map
    from make_golden_recall import import_reference_recall
    mean_ap, _ = import_reference_map()
    recall = import_reference_recall()
    np.int = int
    R._mod('mmcv', load=_load, list_from_file=_list_from_file)
    R._mod('mmcv.utils', print_log=lambda *a, **k: None, Registry=R._Registry, build_from_cfg=R._build_from_cfg)
    R._mod('mmcv.parallel', collate=None)
    R._mod('mmcv.runner', get_dist_info=lambda: (0, 1))
    R._pkg('mmdet', os.path.join(R.REF, 'mmdet'))
    R._mod('mmdet.core', eval_map=mean_ap.eval_map, eval_recalls=recall.eval_recalls)
    ds = R._pkg('mmdet.datasets', os.path.join(R.REF, 'mmdet', 'datasets'))
    R._mod('mmdet.datasets.pipelines', Compose=lambda pipeline: pipeline)
    R._mod('mmdet.datasets.api_wrappers', COCO=_COCO, COCOeval=None)
    samplers = R._pkg('mmdet.datasets.samplers', os.path.join(R.REF, 'mmdet', 'datasets', 'samplers'))
    group = importlib.import_module('mmdet.datasets.samplers.group_sampler')
    samplers.GroupSampler, samplers.DistributedGroupSampler = group.GroupSampler, group.DistributedGroupSampler
    samplers.DistributedSampler = None
    builder = importlib.import_module('mmdet.datasets.builder')
    ds.CustomDataset = importlib.import_module('mmdet.datasets.custom').CustomDataset
    for name in ('coco', 'xml_style', 'voc', 'garbage', 'dataset_wrappers'):
        importlib.import_module(f'mmdet.datasets.{name}')
    traffic = importlib.import_module('mmdet.datasets.tencent_traffic')
    import glob as real_glob
    traffic.glob = types.SimpleNamespace(glob=lambda pattern: sorted(real_glob.glob(pattern)))
    return builder, group.GroupSampler


def import_split_tool(shapes, writes):
    """The root ``tencent_image_split.py`` with a ``cv2`` that reads zeros of ``shapes[image id]`` and records writes."""
    def imread(path):
        w, h = shapes[os.path.splitext(os.path.basename(path))[0]]
        return np.zeros((h, w, 3), np.uint8)

    def imwrite(path, img):
        writes.append((os.path.basename(path), img.shape))
        return True
    R._mod('cv2', imread=imread, imwrite=imwrite)
    sk = R._mod('skimage')
    sk.io = R._mod('skimage.io', imread=lambda path: None)
    spec = importlib.util.spec_from_file_location('ref_tencent_image_split', os.path.join(R.REF, 'tencent_image_split.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TencentImageSplitTool


# ---- recording ---------------------------------------------------------------------------------------------------------
def tables(ds, out, prefix, draws=True):
    out[f'{prefix}/names'] = np.array([d['filename'] for d in ds.data_infos])
    if hasattr(ds, 'flag'):
        out[f'{prefix}/flag'] = ds.flag
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        for key in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            if key in ann:
                out[f'{prefix}/{key}_{i}'] = np.asarray(ann[key])
        out[f'{prefix}/cats_{i}'] = np.asarray(ds.get_cat_ids(i), np.int64)
    if draws and hasattr(ds, 'flag'):
        for seed in SEEDS:
            np.random.seed(seed)
            out[f'{prefix}/others_{seed}'] = np.stack([ds.batch_rand_others(i, 3) for i in range(len(ds))]).astype(np.int64)
            np.random.seed(seed)
            out[f'{prefix}/another_{seed}'] = np.array([ds._rand_another(i) for i in range(len(ds))], np.int64)


def detections(rng, annotations, num_classes):
    """Fixed detections for ``annotations``: every ground-truth box jittered, plus false positives; scores distinct.
    -> the flat form ``(dets (D, 5) float32, labels (D,) int64, img_index (D,) int64)`` in image, class, row order."""
    rows = []
    for i, ann in enumerate(annotations):
        per = []
        for b, l in zip(np.asarray(ann['bboxes'], np.float32).reshape(-1, 4), np.asarray(ann['labels']).reshape(-1)):
            if rng.random() < 0.85:
                per.append((int(l), b + rng.normal(0, 2.0, 4).astype(np.float32)))
        for _ in range(int(rng.integers(1, 4))):
            x1, y1 = rng.uniform(0, 30, 2)
            per.append((int(rng.integers(0, num_classes)), np.array([x1, y1, x1 + rng.uniform(5, 30), y1 + rng.uniform(5, 30)],
                                                                    np.float32)))
        per.sort(key=lambda t: t[0])
        rows += [(i, l, b) for l, b in per]
    scores = rng.permutation(len(rows)).astype(np.float32) / np.float32(len(rows)) * np.float32(0.9) + np.float32(0.05)
    dets = np.concatenate([np.stack([b for _, _, b in rows]).astype(np.float32), scores[:, None]], 1).astype(np.float32)
    return dets, np.array([l for _, l, _ in rows], np.int64), np.array([i for i, _, _ in rows], np.int64)


def evaluations(ds, out, prefix, rng, num_imgs=None, annotations=None):
    """``det_<prefix>`` and ``eval_<prefix>/<case>/<key>`` of dataset (or ConcatDataset) ``ds``."""
    n = len(ds) if num_imgs is None else num_imgs
    anns = annotations if annotations is not None else [ds.get_ann_info(i) for i in range(n)]
    flat = detections(rng, anns, len(ds.CLASSES))
    out[f'det_{prefix}/dets'], out[f'det_{prefix}/labels'], out[f'det_{prefix}/img_index'] = flat
    for case, kw in EVAL_CASES.items():
        results = as_proposals(flat, n) if kw['metric'] == 'recall' else as_lists(flat, n, len(ds.CLASSES))
        for key, v in ds.evaluate(results, logger='silent', **kw).items():
            out[f'eval_{prefix}/{case}/{key}'] = np.float64(v)


def split_tool(out, shapes, work):
    writes = []
    Tool = import_split_tool({f'{n}': shapes[f'split_{n}'] for n, _, _, _ in SPLIT_SOURCES}, writes)
    for name, w, h, rows in SPLIT_SOURCES:
        root, dst = os.path.join(work, f'split_in_{name}'), os.path.join(work, f'split_out_{name}')
        os.makedirs(os.path.join(root, 'img'))
        os.makedirs(os.path.join(root, 'label'))
        with open(os.path.join(root, 'img', f'{name}.jpg'), 'wb') as f:
            f.write(out[f'jpg/split_{name}'].tobytes())
        with open(os.path.join(root, 'label', f'{name}.circle'), 'w') as f:
            f.writelines(rows)
        del writes[:]
        Tool(root, dst, tile_overlap=SPLIT_OVERLAP, tile_shape=SPLIT_TILE, num_process=0).split()
        names = [n[:-4] for n, _ in writes]
        out[f'split/{name}/rows'] = np.array(rows)
        out[f'split/{name}/tiles'] = np.array(names)
        out[f'split/{name}/offsets'] = np.array([[int(v) for v in n.split('_')[-2:]] for n in names], np.int64).reshape(-1, 2)
        out[f'split/{name}/shapes'] = np.array([s[:2] for _, s in writes], np.int64).reshape(-1, 2)
        assert sorted(os.listdir(os.path.join(dst, 'label'))) == sorted(n + '.circle' for n in names)
        for n in names:
            with open(os.path.join(dst, 'label', n + '.circle')) as f:
                out[f'split/{name}/label/{n}'] = np.array(f.read())
        print('split', name, (w, h), out[f'split/{name}/offsets'].tolist(), out[f'split/{name}/shapes'].tolist())


def recipe():
    """The traffic-sign recipe's settings, parsed with this package's ``Config`` (as ``make_golden_configs.py`` does)."""
    import mmdet_yolov4_amd as pkg
    from make_golden_configs import plain
    cfg = pkg.Config.fromfile(os.path.join(R.REF, 'configs', 'tencent', 'tencent_traffic_sign_yolov4l.py'))
    keep = ('model', 'data', 'evaluation', 'checkpoint_config', 'total_epochs', 'optimizer', 'optimizer_config', 'lr_config')
    d = cfg.to_dict()
    with open(os.path.join(HERE, 'custom_sets_recipe.json'), 'w') as f:
        json.dump({k: plain(d[k]) for k in keep if k in d}, f, indent=1, sort_keys=True)


def main():
    import tempfile
    write_sources()
    out = {}
    shapes = image_files(out)
    builder, GroupSampler = import_reference()
    build = builder.build_dataset
    work = tempfile.mkdtemp()
    root = write_tree(os.path.join(work, 'sets'), {k[4:]: v.tobytes() for k, v in out.items() if k.startswith('jpg/')})
    blocks = plain_blocks(root)
    rng = np.random.default_rng(20261021)

    ca, cb = build(blocks['{A}']), build(blocks['{B}'])
    tables(ca, out, 'ca')
    tables(cb, out, 'cb')
    assert set(np.unique(ca.flag)) == {0, 1} and len(ca) == 11
    v07, v12 = build(blocks['{V07}']), build(blocks['{V12}'])
    tables(v07, out, 'v07')
    tables(v12, out, 'v12')
    out['v07/wh'] = np.array([[d['width'], d['height']] for d in build(dict(blocks['{V07}'], test_mode=True)).data_infos])
    assert (v07.year, v12.year) == (2007, 2012)
    tables(build(dict(blocks['{V12}'], min_size=8)), out, 'v12m', draws=False)
    tables(build(dict(blocks['{V07}'], filter_empty_gt=False)), out, 'v07e', draws=False)
    circle = circle_block(root)
    ts = build(circle)
    tables(ts, out, 'ts')
    tables(build(dict(circle, test_mode=True)), out, 'tsv', draws=False)
    tables(build(dict(circle, difficulty_thresh=0, test_mode=True)), out, 'ts0', draws=False)
    tst = build(dict(circle, ann_file=os.path.join(root, 'circle_img'), test_mode=True))
    out['tst/names'] = np.array([d['filename'] for d in tst.data_infos])
    tables(build(dict(blocks['{A}'], type='GarbageDataset', class_agnostic=True)), out, 'ga', draws=False)

    for name, form in WRAPPER_FORMS.items():
        w = build(fill(form, blocks))
        out[f'{name}/len'], out[f'{name}/flag'] = np.int64(len(w)), w.flag
        for i in range(len(w)):
            # (the reference's ClassBalancedDataset has no get_cat_ids of its own: its repeat_indices name the image)
            cats = w.get_cat_ids(i) if hasattr(w, 'get_cat_ids') else w.dataset.get_cat_ids(w.repeat_indices[i])
            out[f'{name}/cats_{i}'] = np.asarray(cats, np.int64)
        if name in ('repeat_v07', 'concat_ab'):
            for seed in (3, 4):
                np.random.seed(seed)
                out[f'group_{name}_{seed}'] = np.array(list(GroupSampler(w, 2)), np.int64)
    for thr in (0.5, 0.9):
        w = build(dict(WRAPPER_FORMS['cbd_v'], oversample_thr=thr, dataset=fill('{VV}', blocks)))
        out[f'cbd_{thr}/repeat_indices'], out[f'cbd_{thr}/flag'] = np.array(w.repeat_indices, np.int64), w.flag

    # evaluate: test-mode datasets (nothing filtered), as a validation loader holds them
    test = dict(test_mode=True)
    evaluations(build(dict(blocks['{A}'], **test)), out, 'ca', rng)
    evaluations(build(dict(blocks['{V07}'], **test)), out, 'v07', rng)
    evaluations(build(dict(blocks['{V12}'], **test)), out, 'v12', rng)
    evaluations(build(dict(circle, **test)), out, 'ts', rng)
    for name, sep in (('concat_sep', True), ('concat_joint', False)):
        w = build(dict(type='ConcatDataset', separate_eval=sep, datasets=[dict(blocks['{A}'], **test), dict(blocks['{B}'], **test)]))
        anns = [d.get_ann_info(i) for d in w.datasets for i in range(len(d))]
        evaluations(w, out, name, rng, num_imgs=len(w), annotations=anns)

    split_tool(out, shapes, work)
    shutil.rmtree(work)
    recipe()
    np.savez_compressed(os.path.join(HERE, 'custom_sets.npz'), **out)
    print('ca', out['ca/names'].tolist(), out['ca/flag'].tolist())
    print('v07', out['v07/names'].tolist(), 'v12', out['v12/names'].tolist(), 'ts', out['ts/names'].tolist())
    print({k: float(v) for k, v in out.items() if k.startswith('eval_')})
    print(f'{len(out)} arrays -> custom_sets.npz')


if __name__ == '__main__':
    main()
