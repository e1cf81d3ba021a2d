#!/usr/bin/env python
"""Generate tests/golden/soft_nms.npz: soft-NMS test configs through the REFERENCE's own post-processing code.

mmcv-full is absent, so the name ``batched_nms`` that the reference's bbox_nms module imported is bound to a function
that sends ``type='soft_nms'`` to the restatement of mmcv 1.3.x (tests/_soft_nms_ref.py, the definition of
include/yv4.h) and every other type to the oracle's hard NMS, as _ref_import does.  Everything around it is the
reference's: multiclass_nms (bbox_nms.py:7-93), YOLOCSPHead.get_bboxes on tiny_v4.npz's pred maps, YOLOV3Head.get_bboxes
on tiny_v3.npz's pred maps, and YOLOV3Head.aug_test (dense_test_mixins.py:38-100) on the network and inputs of
v3_tta.npz's 'scales_hflip' case.  The pred maps and images are not stored again.

multiclass_nms cases (synthetic, stored with their inputs): each method, the split path, empty input, every score below
min_score, exact ties, negative coordinates across classes, integer-coordinate pairs whose fp32 IoU equals the
threshold, and YOLOv3's score_factors.

Run in the build container only; the GPU box never sees the reference tree.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
import _soft_nms_ref as R  # noqa: E402
from make_golden_v3 import ARCH, import_v3  # noqa: E402
from oracle import build_ref  # noqa: E402

F32 = np.float32
LINEAR = dict(type='soft_nms', iou_threshold=0.3, method='linear')
NAIVE = dict(type='soft_nms', iou_threshold=0.5, method='naive', min_score=0.0)
GAUSS = dict(type='soft_nms', iou_threshold=0.3, method='gaussian', sigma=0.5)


def bind_batched_nms(ref):
    """Rebind the reference's bbox_nms.batched_nms (the name it imported from mmcv.ops.nms)."""
    hard = ref.nms.batched_nms

    def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
        if dict(nms_cfg).get('type', 'nms') != 'soft_nms':
            return hard(boxes, scores, idxs, nms_cfg, class_agnostic)
        d, k = R.batched_soft_nms(boxes.numpy(), scores.numpy(), idxs.numpy(), nms_cfg, class_agnostic)
        return torch.from_numpy(np.ascontiguousarray(d, F32)), torch.from_numpy(np.ascontiguousarray(k, np.int64))
    ref.nms.batched_nms = batched_nms


def boxes_random(rng, n, lo=0.0, hi=300.0):
    xy = rng.uniform(lo, hi, (n, 2)).astype(F32)
    wh = rng.uniform(8, 60, (n, 2)).astype(F32)
    return np.concatenate([xy, xy + wh], 1).astype(F32)


def boundary_boxes():
    """Integer-coordinate pairs, each alone in a 100 px cell, whose IoU in fp32 equals 0.5 or 0.25 exactly."""
    pairs = [([0, 0, 10, 10], [0, 0, 10, 5], 0.5), ([0, 0, 8, 8], [0, 0, 8, 4], 0.5), ([0, 0, 4, 4], [0, 0, 4, 1], 0.25),
             ([0, 0, 12, 6], [0, 0, 12, 3], 0.5), ([0, 0, 20, 20], [0, 0, 20, 5], 0.25), ([0, 0, 6, 6], [3, 0, 9, 6], 1 / 3)]
    boxes, thr = [], []
    for c, (a, b, t) in enumerate(pairs):
        off = np.array([100 * c, 0, 100 * c, 0], F32)
        a, b = np.array(a, F32) + off, np.array(b, F32) + off
        ovr = R._ovr(a, (a[2] - a[0]) * (a[3] - a[1]), b[None], np.array([(b[2] - b[0]) * (b[3] - b[1])], F32))[0]
        assert ovr == F32(t), (a, b, ovr, t)
        boxes += [a, b]
        thr.append(t)
    return np.stack(boxes).astype(F32), thr


def multiclass_cases(rng):
    C = 4
    cases = {}
    b = boxes_random(rng, 300)
    s = rng.uniform(0, 1, (300, C + 1)).astype(F32)
    cases['linear'] = (b, s, None, 0.05, LINEAR, 100)
    cases['naive'] = (b, s, None, 0.05, NAIVE, 100)
    cases['gaussian'] = (b, s, None, 0.05, GAUSS, 100)
    bs = boxes_random(rng, 2600, 0, 600)
    ss = rng.uniform(0.02, 1, (2600, C + 1)).astype(F32)
    cases['split'] = (bs, ss, None, 0.01, dict(LINEAR, min_score=0.3), 100)
    cases['empty'] = (b[:50], (s[:50] * F32(0.01)).astype(F32), None, 0.05, LINEAR, 100)
    cases['below_min'] = (b[:80], rng.uniform(2e-4, 9e-4, (80, C + 1)).astype(F32), None, 1e-4, LINEAR, 100)
    st = (np.round(s * 4) / 4).astype(F32)
    cases['ties'] = (b, st, None, 0.05, LINEAR, 300)
    bn = boxes_random(rng, 200, -150, 100)
    cases['negative'] = (bn, s[:200], None, 0.05, dict(LINEAR, iou_threshold=0.2), 100)
    bb, thr = boundary_boxes()
    sb = np.zeros((bb.shape[0], C + 1), F32)
    for j in range(bb.shape[0]):
        sb[j, (j // 2) % C] = F32(0.9) if j % 2 == 0 else F32(0.8)
    for t in sorted(set(thr)):
        cases[f'boundary_{t:.3f}'] = (bb, sb, None, 0.05, dict(LINEAR, iou_threshold=t), 100)
    cases['boundary_naive'] = (bb, sb, None, 0.05, dict(NAIVE, iou_threshold=0.5), 100)
    cases['score_factors'] = (b, s, rng.uniform(0.2, 1, 300).astype(F32), 0.05, LINEAR, 100)
    return cases


def main():
    if not _ref_import.available():
        print('reference not present: nothing to do')
        return
    ref = _ref_import.install_shim(build_ref.load_ext())
    v3 = import_v3(ref)
    bind_batched_nms(ref)
    rng = np.random.RandomState(2024)
    data, meta = {}, {}
    # ---- multiclass_nms -------------------------------------------------------------------------------------------
    for name, (b, s, f, thr, cfg, max_num) in multiclass_cases(rng).items():
        kw = {} if f is None else dict(score_factors=torch.from_numpy(f))
        d, l, inds = ref.nms.multiclass_nms(torch.from_numpy(b), torch.from_numpy(s), thr, cfg, max_num,
                                            return_inds=True, **kw)
        p = f'mc/{name}/'
        data.update({p + 'boxes': b, p + 'scores': s, p + 'dets': d.numpy().astype(F32), p + 'labels': l.numpy(),
                     p + 'inds': inds.numpy()})
        if f is not None:
            data[p + 'factors'] = f
        meta[f'mc/{name}'] = dict(score_thr=thr, nms=cfg, max_num=max_num, detections=int(d.shape[0]),
                                  candidates=int((s[:, :-1] > F32(thr)).sum()))
        print(name, meta[f'mc/{name}'])
    assert meta['mc/split']['candidates'] >= 10000 and meta['mc/empty']['detections'] == 0
    assert meta['mc/below_min']['detections'] == 1
    # ---- YOLOCSPHead.get_bboxes on tiny_v4's pred maps ---------------------------------------------------------------
    g4 = np.load(os.path.join(HERE, 'tiny_v4.npz'))
    preds4 = [torch.from_numpy(g4[f'pred{i}']) for i in range(3)]
    metas4 = [dict(scale_factor=g4['scale_factors'][i]) for i in range(preds4[0].shape[0])]
    for tag, cfg in (('linear', LINEAR), ('naive', NAIVE), ('gaussian', GAUSS)):
        head = ref.head.YOLOCSPHead(num_classes=80, in_channels=[8, 8, 8], train_cfg=None,
                                    test_cfg=ref.ConfigDict(nms_pre=-1, score_thr=0.001, nms=cfg, max_per_img=300))
        with torch.no_grad():
            res = head.get_bboxes([p.clone() for p in preds4], metas4, rescale=True)
        for n, (d, l) in enumerate(res):
            data[f'v4/{tag}/dets{n}'] = d.numpy().astype(F32)
            data[f'v4/{tag}/labels{n}'] = l.numpy()
        meta[f'v4/{tag}'] = dict(nms=cfg, detections=[int(d.shape[0]) for d, _ in res])
        print('v4', tag, meta[f'v4/{tag}'])
    # ---- YOLOV3Head.get_bboxes on tiny_v3's pred maps, and aug_test on v3_tta's scales_hflip case --------------------
    v3.darknet.Darknet.arch_settings = {53: ARCH}
    g3 = np.load(os.path.join(HERE, 'tiny_v3.npz'))
    sd = {k[3:]: torch.from_numpy(g3[k].astype(F32) if g3[k].dtype == np.float16 else g3[k])
          for k in g3.files if k.startswith('sd/')}
    v3cfg = dict(nms_pre=40, min_bbox_size=0, score_thr=0.05, conf_thr=0.005, nms=LINEAR, max_per_img=100)
    head3 = v3.head.YOLOV3Head(num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32], train_cfg=None,
                               test_cfg=ref.ConfigDict(v3cfg))
    head3.load_state_dict({k[10:]: v for k, v in sd.items() if k.startswith('bbox_head.')}, strict=True)
    torch.nn.Module.eval(head3)
    preds3 = [torch.from_numpy(g3[f'pred{i}']) for i in range(3)]
    metas3 = [dict(scale_factor=g3['scale_factors'][i]) for i in range(preds3[0].shape[0])]
    with torch.no_grad():
        res = head3.get_bboxes(preds3, metas3, rescale=True)
    for n, (d, l) in enumerate(res):
        data[f'v3/dets{n}'] = d.numpy().astype(F32)
        data[f'v3/labels{n}'] = l.numpy()
    meta['v3'] = dict(test_cfg=v3cfg, detections=[int(d.shape[0]) for d, _ in res])
    print('v3', meta['v3'])
    backbone = v3.darknet.Darknet(depth=53, out_indices=(3, 4, 5))
    neck = v3.neck.YOLOV3Neck(num_scales=3, in_channels=[64, 64, 32], out_channels=[64, 32, 16])
    for pre, m in (('backbone', backbone), ('neck', neck)):
        m.load_state_dict({k[len(pre) + 1:]: v for k, v in sd.items() if k.startswith(pre + '.')}, strict=True)
        torch.nn.Module.eval(m)
    gt = np.load(os.path.join(HERE, 'v3_tta.npz'))
    case = json.loads(str(gt['cases']))['scales_hflip']
    imgs = [torch.from_numpy(gt[f'scales_hflip/img{a}']) for a in range(case['num_augs'])]
    metas = [[dict(img_shape=tuple(int(v) for v in gt[f'scales_hflip/img_shape{a}']),
                   pad_shape=tuple(int(v) for v in gt[f'scales_hflip/pad_shape{a}']),
                   scale_factor=gt[f'scales_hflip/scale_factor{a}'], flip=d is not None, flip_direction=d)]
             for a, d in enumerate(case['flips'])]
    tta_cfg = dict(case['test_cfg'], nms=LINEAR)
    head3.test_cfg = ref.ConfigDict(tta_cfg)
    with torch.no_grad():
        feats = [neck(backbone(x)) for x in imgs]
        res = head3.aug_test(feats, metas, rescale=True)
    for c, arr in enumerate(res):
        data[f'tta/result_{c}'] = arr.astype(F32)
    meta['tta'] = dict(case='scales_hflip', test_cfg=tta_cfg, detections=int(sum(a.shape[0] for a in res)))
    print('tta', meta['tta'])
    data['meta'] = np.array(json.dumps(meta, sort_keys=True))
    out = os.path.join(HERE, 'soft_nms.npz')
    np.savez_compressed(out, **data)
    print('soft_nms', out, f'{os.path.getsize(out) / 1e6:.3f} MB')


if __name__ == '__main__':
    main()
