"""Generate tests/golden/image_map.npz: the REFERENCE's per-image mAP (``bbox_map_eval`` of
``tools/analysis_tools/analyze_results.py``) on synthetic images.

Run in the build container only:   python tests/golden/make_golden_image_map.py
``mean_ap.py`` is imported as ``make_golden_map.import_reference_map`` does, with the serial pool, and the tool's own
``bbox_map_eval`` is loaded from its file and run as it is under this container's numpy (2.x: a float32 IoU compared
with the ``np.float64`` thresholds of ``np.linspace`` is compared in float64).  What the tool imports and the container
lacks is represented by stand-ins with no arithmetic: ``mmcv.Config`` / ``DictAction``, ``mmdet.core.visualization``,
``mmdet.datasets``.  The fixture is data only: per set the inputs (flat), per image the mAP (float64) and per image and
threshold the ``mean_ap`` of ``eval_map``.

Two sets.  ``main``: 40 synthetic images x 6 classes (``_map_data.synth_dataset`` with its four crafted images, the IoU
== float32(0.7) pair among them) plus hand-built ones -- no gts at all, gts without detections, detections of a class
without gts, ignored gts only, perfect detections.  ``wide``: 300 classes, images with 7, 8, 9, 129 and 300 classes that
have a gt (one box each), whose detections hit at some thresholds only and sit behind 0 to 3 false positives, so that
the per-class APs are 1, 1/2, 1/3, 1/4 or 0 and the order in which float32 adds them shows.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import as R  # noqa: E402
from _image_map_ref import store_set  # noqa: E402
from _map_data import synth_dataset  # noqa: E402
from make_golden_map import import_reference_map  # noqa: E402


def import_reference_tool():
    """(the tool's module, the reference's eval_map)."""
    M, _ = import_reference_map()
    mmcv = sys.modules['mmcv']
    mmcv.Config = mmcv.DictAction = object
    sys.modules['mmdet.core.evaluation'].eval_map = M.eval_map
    R._mod('mmdet.core.visualization', imshow_gt_det_bboxes=None)
    R._mod('mmdet.datasets', build_dataset=None, get_loading_pipeline=None)
    spec = importlib.util.spec_from_file_location(
        'ref_analyze_results', os.path.join(R.REF, 'tools', 'analysis_tools', 'analyze_results.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool, M.eval_map


def _f(rows, cols):
    return np.array(rows, np.float32).reshape(-1, cols)


def hand_built(num_cls):
    """(dets, annos, names): the edge images of the main set; scores distinct inside every (image, class)."""
    dets, annos, names = [], [], []

    def image(name, cls_dets, **anno):
        per_cls = [np.zeros((0, 5), np.float32) for _ in range(num_cls)]
        for c, rows in cls_dets.items():
            per_cls[c] = _f(rows, 5)
        dets.append(per_cls)
        annos.append({k: (_f(v, 4) if k.startswith('bboxes') else np.array(v, np.int64)) for k, v in anno.items()})
        names.append(name)
    image('no_gts', {1: [[10, 10, 50, 50, 0.9], [60, 60, 90, 90, 0.4]]}, bboxes=[], labels=[])
    image('no_dets', {}, bboxes=[[10, 10, 50, 50], [100, 100, 180, 160]], labels=[0, 2])
    image('det_of_class_without_gt', {0: [[10, 10, 50, 56, 0.8]], 3: [[10, 10, 50, 50, 0.95], [200, 200, 240, 240, 0.5]]},
          bboxes=[[10, 10, 50, 50]], labels=[0])
    image('ignore_only', {2: [[100, 100, 200, 200, 0.7], [300, 300, 340, 340, 0.6]]}, bboxes=[], labels=[],
          bboxes_ignore=[[100, 100, 200, 198]], labels_ignore=[2])
    image('perfect', {0: [[10, 10, 50, 50, 0.9], [100, 20, 160, 90, 0.8]], 4: [[200, 200, 300, 260, 0.6]]},
          bboxes=[[10, 10, 50, 50], [100, 20, 160, 90], [200, 200, 300, 260]], labels=[0, 0, 4])
    return dets, annos, names


def wide_set(num_cls=300, counts=(7, 8, 9, 129, 300)):
    """Image k: classes 0 .. counts[k]-1 hold one 40 x 40 gt each.  Class c's good detection is the gt moved right by
    2 * (1 + (c + k) % 7) pixels -- IoU (40 - s) / (40 + s): 0.905, 0.818, 0.739, 0.667, 0.6, 0.538, 0.481 -- with score
    0.3, behind (3 * c + k) % 4 far-away false positives with higher, distinct scores."""
    dets, annos = [], []
    for k, n in enumerate(counts):
        per_cls = [np.zeros((0, 5), np.float32) for _ in range(num_cls)]
        gts = []
        for c in range(n):
            x0, y0 = 50.0 * (c % 20), 50.0 * (c // 20)
            gts.append([x0, y0, x0 + 40, y0 + 40])
            s = 2.0 * (1 + (c + k) % 7)
            rows = [[x0, y0 + 2000 + 60 * j, x0 + 40, y0 + 2040 + 60 * j, 0.9 - 0.1 * j] for j in range((3 * c + k) % 4)]
            rows.append([x0 + s, y0, x0 + 40 + s, y0 + 40, 0.3])
            per_cls[c] = _f(rows, 5)
        dets.append(per_cls)
        annos.append(dict(bboxes=_f(gts, 4), labels=np.arange(n, dtype=np.int64)))
    return dets, annos


def score_set(tool, eval_map, dets, annos):
    """(map (N,) float64, mean_ap (T, N) float32) from the reference: its own bbox_map_eval per image, and the mean_ap
    of its eval_map at each of bbox_map_eval's thresholds."""
    thrs = np.linspace(0.5, 0.95, 10)
    maps = np.array([tool.bbox_map_eval(d, a) for d, a in zip(dets, annos)], np.float64)
    per = np.zeros((len(thrs), len(dets)), np.float64)
    for i, (d, a) in enumerate(zip(dets, annos)):
        for t, thr in enumerate(thrs):
            per[t, i] = eval_map([d], [a], iou_thr=thr, logger='silent')[0]
        assert sum(per[:, i].tolist()) / len(thrs) == maps[i]
    assert (per.astype(np.float32).astype(np.float64) == per).all()          # every mean_ap is a float32 value
    return maps, per.astype(np.float32)


def main():
    tool, eval_map = import_reference_tool()
    rng = np.random.default_rng(20261020)
    out = {}
    dets, annos = synth_dataset(rng, 40, 6, distinct_scores=True, crafted=True)
    iou07 = 40                                                   # the first crafted image: the IoU == float32(0.7) pair
    assert (dets[iou07][0][:, :4] == [0, 0, 10, 7]).all() and (annos[iou07]['bboxes'] == [0, 0, 10, 10]).all()
    hd, ha, names = hand_built(6)
    first_hand = len(dets)
    dets, annos = dets + hd, annos + ha
    wd, wa = wide_set()
    for name, (d, a) in dict(main=(dets, annos), wide=(wd, wa)).items():
        for i, per_cls in enumerate(d):                          # no stored value depends on a tie order
            for c, rows in enumerate(per_cls):
                assert rows.dtype == np.float32 and len(np.unique(rows[:, 4])) == len(rows), (name, i, c)
        maps, per = score_set(tool, eval_map, d, a)
        store_set(out, name, d, a)
        out[f'{name}/map'], out[f'{name}/mean_ap'] = maps, per
        print(name, len(d), 'images', maps.round(4).tolist()[-12:])
    m, per = out['main/map'], out['main/mean_ap']
    # the threshold trap: a miss at 0.7 (float32(0.7) < 0.7 in float64), a hit at 0.65
    assert per[4, iou07] == 0.0 and per[3, iou07] == 1.0 and m[iou07] == 0.4
    hand = {n: first_hand + k for k, n in enumerate(names)}
    assert m[hand['no_gts']] == 0.0 and m[hand['no_dets']] == 0.0 and m[hand['ignore_only']] == 0.0
    assert m[hand['perfect']] == 1.0 and 0.0 < m[hand['det_of_class_without_gt']] < 1.0
    out['main/iou07_image'] = np.int64(iou07)
    for n, k in hand.items():
        out[f'main/hand/{n}'] = np.int64(k)
    # the pairwise mean shows: a left-to-right float32 sum gives another mean somewhere among the wide images
    import _image_map_ref as I
    _, mine = I.image_maps(wd, wa)
    assert (mine == out['wide/mean_ap']).all()
    differs = 0
    for i in (3, 4):
        for t, thr in enumerate(I.IOU_THRS):
            aps = [I.problem_ap(*I.tpfp(wd[i][c], wa[i]['bboxes'][c:c + 1], None, thr), 1) for c in range(len(wa[i]['labels']))]
            seq = np.float32(0)
            for v in aps:
                seq = np.float32(seq + v)
            differs += int(np.float32(seq / np.float32(len(aps))) != out['wide/mean_ap'][t, i])
    assert differs > 0, 'the wide images do not tell the pairwise sum from a left-to-right one'
    print('thresholds at which a left-to-right sum would differ:', differs)
    path = os.path.join(HERE, 'image_map.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
