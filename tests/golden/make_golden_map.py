"""Generate tests/golden/map_eval.npz: outputs of the REFERENCE's VOC-style mAP on a synthetic dataset.

Run in the build container only:   python tests/golden/make_golden_map.py
``mmdet/core/evaluation/mean_ap.py`` and ``bbox_overlaps.py`` are imported from the reference checkout and run as
they are under this container's numpy (2.x: float32 arrays compare with Python floats in float32).  What they import
and the container lacks is represented by stand-ins with no arithmetic: mmcv's ``print_log`` / ``is_str``,
``terminaltables.AsciiTable``, ``class_names.get_classes``, and a serial ``Pool`` (``starmap`` as a list
comprehension), so that nothing forks (``import_reference_map(serial_pool=False)`` keeps the real pool: tools/map_bench.py
times the reference with it).  The fixture is data only: the inputs, per case the reference's per-class
``num_gts`` / ``num_dets`` / ``recall`` / ``precision`` / ``ap`` and ``mean_ap``, per (image, class) the direct
``tpfp_default`` / ``tpfp_imagenet`` flags, and ``bbox_overlaps`` vectors.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import as R  # noqa: E402
from _map_data import (CASES, TPFP_CASES, boxes, class_major_problems, store_dataset, store_result, synth_dataset,  # noqa: E402
                       without_detections)


class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def starmap(self, fn, it):
        return [fn(*args) for args in it]

    def close(self):
        pass


def import_reference_map(serial_pool=True):
    mmcv = R._mod('mmcv', is_str=lambda x: isinstance(x, str))
    mmcv.utils = R._mod('mmcv.utils', print_log=lambda *a, **k: None)
    R._mod('terminaltables', AsciiTable=object)
    m = os.path.join(R.REF, 'mmdet')
    R._pkg('mmdet', m)
    R._pkg('mmdet.core', os.path.join(m, 'core'))
    R._pkg('mmdet.core.evaluation', os.path.join(m, 'core', 'evaluation'))
    R._mod('mmdet.core.evaluation.class_names', get_classes=None)
    M = importlib.import_module('mmdet.core.evaluation.mean_ap')
    if serial_pool:
        M.Pool = _SerialPool
    return M, importlib.import_module('mmdet.core.evaluation.bbox_overlaps').bbox_overlaps


def overlap_vectors(rng, ref_overlaps, out):
    cases = [(7, 13), (13, 7), (1, 1), (40, 3), (6, 6)]
    for k, (n1, n2) in enumerate(cases):
        a, b = boxes(rng, n1), boxes(rng, n2)
        n = min(n1, n2)
        a[:n] = b[:n] + rng.normal(0, 5, (n, 4)).astype(np.float32)
        if k == 4:
            a[0] = b[0] = [50, 50, 50, 50]                      # zero area on both sides: union 0 -> eps
            a[1, 2:] = a[1, :2]                                 # zero-area first box inside a second box
            b[1] = [a[1, 0] - 5, a[1, 1] - 5, a[1, 0] + 5, a[1, 1] + 5]
            a[2] = b[2] = [10, 10, 10 + 1e-4, 10 + 1e-4]       # identical boxes whose union is below eps
            a[3] = b[3]                                         # IoU exactly 1
        out[f'ov{k}/b1'], out[f'ov{k}/b2'] = a, b
        out[f'ov{k}/iou'] = ref_overlaps(a, b)
        out[f'ov{k}/iof'] = ref_overlaps(a, b, mode='iof')
        out[f'ov{k}/iou_eps1e-3'] = ref_overlaps(a, b, eps=1e-3)
        for key in ('iou', 'iof', 'iou_eps1e-3'):
            assert out[f'ov{k}/{key}'].dtype == np.float32 and out[f'ov{k}/{key}'].shape == (n1, n2)
    out['ov/n'] = np.int64(len(cases))


def main():
    M, ref_overlaps = import_reference_map()
    rng = np.random.default_rng(20261017)
    out = {}
    overlap_vectors(rng, ref_overlaps, out)
    dets, annos = synth_dataset(rng, 60, 6, distinct_scores=True)
    for c in range(6):                                          # no fixture value depends on a host's tie order
        sc = np.concatenate([d[c][:, 4] for d in dets])
        assert len(np.unique(sc)) == len(sc)
    assert all(a['bboxes'].dtype == np.float32 for a in annos)
    assert not any((a['labels'] == 5).any() for a in annos)
    store_dataset(out, dets, annos)
    p = ref_overlaps(np.array([[0, 0, 10, 7]], np.float32), np.array([[0, 0, 10, 10]], np.float32))
    assert p[0, 0] == np.float32(0.7) and p[0, 0] >= 0.7 and not float(p[0, 0]) >= 0.7
    for name, kw in CASES.items():
        d = without_detections(dets) if name == 'empty' else dets
        mean_ap, results = M.eval_map(d, annos, logger='silent', **kw)
        store_result(out, name, mean_ap, results)
        if name in TPFP_CASES:
            fn = M.tpfp_imagenet if kw.get('dataset') == 'det' else M.tpfp_default
            sr = kw.get('scale_ranges')
            area_ranges = None if sr is None else [(lo ** 2, hi ** 2) for lo, hi in sr]
            flags = [fn(dd, g, ign, kw['iou_thr'], area_ranges) for _, _, dd, g, ign in class_major_problems(dets, annos)]
            out[f'{name}/tpfp/tp'] = np.concatenate([f[0] for f in flags], axis=1).astype(np.uint8)
            out[f'{name}/tpfp/fp'] = np.concatenate([f[1] for f in flags], axis=1).astype(np.uint8)
        print(name, mean_ap)
    path = os.path.join(HERE, 'map_eval.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
