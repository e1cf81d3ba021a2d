#!/usr/bin/env python
"""Generate tests/golden/v3_tta.npz: YOLOv3 test-time augmentation (flip + multi-scale) by the REFERENCE's own code.

The network is tiny_v3.npz's narrowed Darknet / YOLOV3Neck / YOLOV3Head, built from the reference's modules
(make_golden_v3.import_v3) and loaded with the checkpoint stored THERE (not stored again here).  Per case:

  * the augmentations in MultiScaleFlipAug order (datasets/pipelines/test_time_aug.py:95-106): per scale the
    unflipped image, then one per flip_direction;
  * each augmentation's input tensor (1, 3, H, W) fp32 -- Resize(keep_ratio) -> RandomFlip -> Normalize -> Pad of
    configs/yolo/yolov3_d53_mstrain-608_273e_coco.py, computed by oracle/preprocess_oracle.py's restatement of the
    OpenCV resize (mmcv / OpenCV are absent from the build image), flipped with numpy on the resized image -- and its
    metas (img_shape, pad_shape, scale_factor, flip, flip_direction);
  * each augmentation's pred maps from the reference's head, and get_bboxes(with_nms=False)[0] on them
    (yolo_head.py:208-391): bboxes (S, 4), scores (S, C + 1), conf (S);
  * aug_test (dense_test_mixins.py:38-100, through YOLOV3Head.aug_test) with rescale=True and rescale=False.

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
import _ref_import  # noqa: E402
from make_golden_v3 import ARCH, import_v3  # noqa: E402
from oracle import build_ref  # noqa: E402
from oracle import preprocess_oracle as PP  # noqa: E402

FLIP_AXES = {'horizontal': (1,), 'vertical': (0,), 'diagonal': (0, 1)}

# name -> (source image (h, w), img_scale list, flip_direction list ([] = flip=False), test_cfg)
CASES = {
    'scales_hflip': ((60, 90), [(64, 48), (96, 64)], ['horizontal'],
                     dict(nms_pre=40, min_bbox_size=0, score_thr=0.05, conf_thr=0.005,
                          nms=dict(type='nms', iou_threshold=0.45), max_per_img=100)),
    'vflip_dflip': ((50, 80), [(64, 48)], ['horizontal', 'vertical', 'diagonal'],
                    dict(nms_pre=1000, min_bbox_size=0, score_thr=0.2, conf_thr=0.005,
                         nms=dict(type='nms', iou_threshold=0.5), max_per_img=60)),
    'split': ((72, 96), [(128, 96)], ['horizontal', 'vertical'],
              dict(nms_pre=-1, min_bbox_size=0, score_thr=0.001, conf_thr=0.005,
                   nms=dict(type='nms', iou_threshold=0.45), max_per_img=100)),
    'empty': ((40, 64), [(64, 48)], ['horizontal'],
              dict(nms_pre=40, min_bbox_size=0, score_thr=0.9999, conf_thr=0.005,
                   nms=dict(type='nms', iou_threshold=0.45), max_per_img=100)),
}


def augment(img, scale, direction):
    """Resize(keep_ratio) -> RandomFlip(direction) -> Normalize -> Pad(32) of one 8-bit BGR image."""
    h, w = img.shape[:2]
    nh, nw = PP.rescale_size(h, w, scale)
    res = PP.resize_linear_u8(img, nh, nw)
    if direction is not None:
        res = np.flip(res, axis=FLIP_AXES[direction])
    a = res.astype(np.float32)[..., ::-1]                      # to_rgb
    a = ((a - np.float32(0)) * np.float32(1 / np.float64(255))).astype(np.float32)
    hp, wp = int(np.ceil(nh / 32)) * 32, int(np.ceil(nw / 32)) * 32
    out = np.zeros((hp, wp, 3), np.float32)                    # Pad after Normalize: zeros
    out[:nh, :nw] = a
    meta = dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(hp, wp, 3),
                scale_factor=np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32),
                flip=direction is not None, flip_direction=direction)
    return np.ascontiguousarray(out.transpose(2, 0, 1))[None], meta


def main():
    if not _ref_import.available():
        print('reference not present: nothing to do')
        return
    ref = _ref_import.install_shim(build_ref.load_ext())
    v3 = import_v3(ref)
    v3.darknet.Darknet.arch_settings = {53: ARCH}
    g = np.load(os.path.join(HERE, 'tiny_v3.npz'))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k])
          for k in g.files if k.startswith('sd/')}
    backbone = v3.darknet.Darknet(depth=53, out_indices=(3, 4, 5))
    neck = v3.neck.YOLOV3Neck(num_scales=3, in_channels=[64, 64, 32], out_channels=[64, 32, 16])
    for pre, m in (('backbone', backbone), ('neck', neck)):
        m.load_state_dict({k[len(pre) + 1:]: v for k, v in sd.items() if k.startswith(pre + '.')}, strict=True)
        torch.nn.Module.eval(m)
    rng = np.random.RandomState(7)
    data = {}
    cases = {}
    for name, (hw, scales, dirs, cfg) in CASES.items():
        head = v3.head.YOLOV3Head(num_classes=6, in_channels=[64, 32, 16], out_channels=[96, 64, 32], train_cfg=None,
                                  test_cfg=ref.ConfigDict(cfg))
        head.load_state_dict({k[10:]: v for k, v in sd.items() if k.startswith('bbox_head.')}, strict=True)
        torch.nn.Module.eval(head)
        # a smooth picture (a random 5 x 7 grid, bilinearly enlarged) keeps the fixture small
        src = PP.resize_linear_u8(rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8), *hw)
        data[f'{name}/src'] = src
        augs = [(s, None) for s in scales] if not dirs else [(s, d) for s in scales for d in [None] + dirs]
        imgs, metas = [], []
        for a, (s, d) in enumerate(augs):
            x, meta = augment(src, s, d)
            imgs.append(torch.from_numpy(x))
            metas.append([meta])
            data[f'{name}/img{a}'] = x
            data[f'{name}/img_shape{a}'] = np.array(meta['img_shape'])
            data[f'{name}/pad_shape{a}'] = np.array(meta['pad_shape'])
            data[f'{name}/scale_factor{a}'] = meta['scale_factor']
        with torch.no_grad():
            feats = [neck(backbone(x)) for x in imgs]
            total = 0
            for a, (f, m) in enumerate(zip(feats, metas)):
                preds = head(f)[0]
                for i, p in enumerate(preds):
                    data[f'{name}/pred{a}_{i}'] = p.numpy()
                b, sc, cf = head.get_bboxes(*([list(preds)] + [m, head.test_cfg, False, False]))[0]
                data[f'{name}/bboxes{a}'] = b.numpy()
                data[f'{name}/scores{a}'] = sc.numpy()
                data[f'{name}/conf{a}'] = cf.numpy()
                total += int((sc[:, :-1] > cfg['score_thr']).sum())
            for rescale, tag in ((True, ''), (False, '_norescale')):
                res = head.aug_test(feats, metas, rescale=rescale)
                for c, arr in enumerate(res):
                    data[f'{name}/result{tag}_{c}'] = arr.astype(np.float32)
        ndet = sum(int(data[f'{name}/result_{c}'].shape[0]) for c in range(6))
        cases[name] = dict(scales=[list(s) for s in scales], flip_direction=dirs, test_cfg=cfg, num_augs=len(augs),
                           flips=[d for _, d in augs], candidates=total, detections=ndet)
        print(name, 'augs', len(augs), 'candidates', total, 'detections', ndet)
    assert cases['split']['candidates'] >= 10000, 'the split case must cross split_thr'
    assert cases['empty']['detections'] == 0 and cases['scales_hflip']['detections'] > 0
    data['cases'] = np.array(json.dumps(cases, sort_keys=True))
    out = os.path.join(HERE, 'v3_tta.npz')
    np.savez_compressed(out, **data)
    print('v3_tta', out, f'{os.path.getsize(out) / 1e6:.3f} MB')


if __name__ == '__main__':
    main()
