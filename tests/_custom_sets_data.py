"""What the fixture script of the datasets beyond COCO (tests/golden/make_golden_custom_sets.py) and their tests share:
where the hand-made sources lie, the dataset blocks over them, every nesting form ``build_dataset`` takes, the
``evaluate`` cases, and the two list forms of a flat result table.  Data and plumbing only."""
import os
import shutil

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'custom_sets')
CLASSES_ABC = ('a', 'b', 'c')
SEEDS = (0, 1, 2)

EVAL_CASES = {
    'map50': dict(metric='mAP', iou_thr=0.5),
    'map_two': dict(metric='mAP', iou_thr=[0.5, 0.75]),
    'recall': dict(metric='recall', iou_thr=[0.5, 0.75], proposal_nums=(1, 3, 10)),
}

# every nesting form build_dataset takes; {A} {B} {AB} {V07} {V12} {VV} stand for the plain blocks of plain_blocks()
WRAPPER_FORMS = {
    'repeat_v07': dict(type='RepeatDataset', times=3, dataset='{V07}'),
    'concat_ab': dict(type='ConcatDataset', datasets=['{A}', '{B}']),
    'list_ab': ['{A}', '{B}'],
    'ann_list': '{AB}',
    'repeat_concat_voc': dict(type='RepeatDataset', times=2, dataset=dict(type='ConcatDataset', datasets=['{V07}', '{V12}'])),
    'cbd_v': dict(type='ClassBalancedDataset', oversample_thr=0.5, dataset='{VV}'),
    'concat_repeat': dict(type='ConcatDataset', separate_eval=True,
                          datasets=[dict(type='RepeatDataset', times=2, dataset='{B}'), '{A}']),
}


def write_tree(root, jpgs):
    """The sources copied to ``root`` and the images where the datasets look for them.  ``jpgs``: ``{name: bytes}`` --
    the fixture's ``jpg/<name>`` arrays."""
    shutil.copytree(SRC, root)
    for year in ('VOC2007', 'VOC2012'):
        os.makedirs(os.path.join(root, year, 'JPEGImages'))
        for xml in sorted(os.listdir(os.path.join(root, year, 'Annotations'))):
            with open(os.path.join(root, year, 'JPEGImages', xml[:-4] + '.jpg'), 'wb') as f:
                f.write(jpgs[xml[:-4]])
    for folder, names in (('circle_img', [n[:-7] for n in sorted(os.listdir(os.path.join(root, 'circle')))]),
                          ('img_a', sorted(n for n in jpgs if n[0] == 'a' and n[1:].isdigit())),
                          ('img_b', sorted(n for n in jpgs if n[0] == 'b' and n[1:].isdigit()))):
        os.makedirs(os.path.join(root, folder))
        for name in names:
            with open(os.path.join(root, folder, name + '.jpg'), 'wb') as f:
                f.write(jpgs[name])
    return root


def circle_block(root, **kw):
    return dict(type='TrafficSignDataset', ann_file=os.path.join(root, 'circle'), img_prefix=os.path.join(root, 'circle_img'),
                pipeline=[], **kw)


def plain_blocks(root):
    """The plain dataset blocks of ``WRAPPER_FORMS`` over the sources in ``root``."""
    voc = dict(type='VOCDataset', pipeline=[])
    middle = dict(type='CustomDataset', classes=CLASSES_ABC, pipeline=[])
    a, b = os.path.join(root, 'middle_a.pkl'), os.path.join(root, 'middle_b.pkl')
    v07, v12 = os.path.join(root, 'VOC2007/'), os.path.join(root, 'VOC2012/')
    return {
        '{A}': dict(middle, ann_file=a, img_prefix=os.path.join(root, 'img_a/')),
        '{B}': dict(middle, ann_file=b, img_prefix=os.path.join(root, 'img_b/')),
        '{AB}': dict(middle, ann_file=[a, b], img_prefix=[os.path.join(root, 'img_a/'), os.path.join(root, 'img_b/')],
                     separate_eval=False),
        '{V07}': dict(voc, ann_file=v07 + 'ImageSets/Main/trainval.txt', img_prefix=v07),
        '{V12}': dict(voc, ann_file=v12 + 'ImageSets/Main/trainval.txt', img_prefix=v12),
        '{VV}': dict(voc, ann_file=[v07 + 'ImageSets/Main/trainval.txt', v12 + 'ImageSets/Main/trainval.txt'],
                     img_prefix=[v07, v12]),
    }


def fill(form, blocks):
    if isinstance(form, str):
        return dict(blocks[form])
    if isinstance(form, list):
        return [fill(f, blocks) for f in form]
    return {k: fill(v, blocks) if k in ('dataset', 'datasets') else v for k, v in form.items()}


def as_lists(flat, num_imgs, num_classes):
    """The flat table ``(dets, labels, img_index)`` as the test loop's per-image, per-class lists."""
    dets, labels, img_index = flat
    return [[dets[(img_index == i) & (labels == c)] for c in range(num_classes)] for i in range(num_imgs)]


def as_proposals(flat, num_imgs):
    """The flat table as per-image ``(n, 5)`` proposal arrays, labels dropped."""
    dets, _, img_index = flat
    return [dets[img_index == i] for i in range(num_imgs)]


def jpgs_of(npz):
    return {k[4:]: npz[k].tobytes() for k in npz.files if k.startswith('jpg/')}
