#!/usr/bin/env python
"""Generate tests/golden/v3_loss.npz by running the REFERENCE's ``YOLOV3Head.loss`` (yolo_head.py:393-586) with its
``GridAssigner`` (grid_assigner.py:73-156) and ``PseudoSampler``, imported through _ref_import.py like
make_golden_v3.py does.

Per case: the pred maps (NCHW fp32), the ground truths per image, ``assigned_gt_inds`` of every image (recorded
from the assigner's return value), the four per-level losses and the gradients of the pred maps for a random
upstream (L, 4) gradient.  Cases: the recipe configuration (80 classes, 3 levels, strides 32/16/8, recipe loss
weights) at small maps, an image without ground truths, duplicate identical ground truths (argmax ties), a centre
exactly on a cell border, tiny and huge boxes, the tuple ``neg_iou_thr``, ``gt_max_assign_all=False`` (with
ground-truth ties and with anchor ties), ``one_hot_smoother=0.1`` and ``reduction='mean'``.

Run in the build container only; the GPU box never sees /root/reference.
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
from make_golden_v3 import import_v3  # noqa: E402
from oracle import build_ref  # noqa: E402

RECIPE_LOSSES = dict(
    loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
    loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
    loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
    loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'))


def _boxes(gen, n, img_w, img_h, smin=4.0, smax=None):
    smax = smax or 0.8 * min(img_w, img_h)
    c = torch.rand(n, 2, generator=gen) * torch.tensor([img_w, img_h])
    s = smin + torch.rand(n, 2, generator=gen) * (smax - smin)
    b = torch.cat([c - s / 2, c + s / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, img_w - 1)
    b[:, 1::2] = b[:, 1::2].clamp(0, img_h - 1)
    return b


def cases(gen):
    W, H = 96, 64                                   # maps 3x2, 6x4, 12x8 at strides 32, 16, 8
    out = []
    # the recipe configuration, several boxes per image, incl. a tiny and a huge one and a centre on a cell border
    b0 = torch.cat([_boxes(gen, 7, W, H), torch.tensor([[30.0, 20.0, 32.0, 23.0], [0.0, 0.0, 95.0, 63.0],
                                                         [8.0, 8.0, 24.0, 24.0]])])     # centre (16, 16): borders
    b1 = _boxes(gen, 9, W, H)
    out.append(dict(name='recipe', C=80, size=(W, H), gt=[b0, b1], head={}, assigner={}))
    # zero ground truths in one image
    out.append(dict(name='zero_gt', C=6, size=(W, H), gt=[torch.zeros(0, 4), _boxes(gen, 5, W, H)], head={},
                    assigner={}))
    # duplicate identical ground truths: argmax ties over gts, equal per-gt maxima
    d = _boxes(gen, 3, W, H)
    out.append(dict(name='dup', C=6, size=(W, H), gt=[torch.cat([d, d[:1], d[1:2], d[:1]]), torch.cat([d[2:], d[2:]])],
                    head={}, assigner={}))
    # centres exactly on cell borders of every level, tiny and huge boxes
    bb = torch.tensor([[12.0, 12.0, 20.0, 20.0], [28.0, 8.0, 36.0, 24.0], [60.0, 28.0, 68.0, 36.0],
                       [47.5, 31.5, 48.5, 32.5], [0.0, 0.0, 96.0, 64.0], [1.0, 2.0, 94.0, 62.0]])
    out.append(dict(name='border_tiny_huge', C=6, size=(W, H), gt=[bb, bb[[4, 0, 3]]], head={}, assigner={}))
    # the tuple neg_iou_thr
    out.append(dict(name='neg_tuple', C=6, size=(W, H), gt=[_boxes(gen, 6, W, H), _boxes(gen, 4, W, H)], head={},
                    assigner=dict(neg_iou_thr=(0.1, 0.4))))
    # gt_max_assign_all=False (the argmax anchor per gt; duplicates make the first-index rule matter)
    d = _boxes(gen, 4, W, H)
    out.append(dict(name='assign_argmax', C=6, size=(W, H), gt=[torch.cat([d, d[:2]]), _boxes(gen, 5, W, H)], head={},
                    assigner=dict(gt_max_assign_all=False, min_pos_iou=0.05)))
    # one_hot_smoother
    out.append(dict(name='smoother', C=6, size=(W, H), gt=[_boxes(gen, 5, W, H), _boxes(gen, 3, W, H)],
                    head=dict(one_hot_smoother=0.1), assigner={}))
    # reduction='mean', other loss weights
    mean = {k: dict(v, reduction='mean', loss_weight=0.5 + i) for i, (k, v) in enumerate(RECIPE_LOSSES.items())}
    out.append(dict(name='mean', C=6, size=(W, H), gt=[_boxes(gen, 6, W, H), _boxes(gen, 6, W, H)], head=dict(losses=mean),
                    assigner=dict(pos_iou_thr=0.3, neg_iou_thr=0.3)))
    # anchor ties for gt_max_assign_all=False: the (16, 30) base anchor of two responsible stride-8 cells has the same IoU
    # (0.6, 0.765) with a gt centred between them; a small second gt makes the other cell responsible.  The reference
    # (torch.max over anchors) claims the FIRST anchor, in image order
    out.append(dict(name='anchor_tie', C=6, size=(W, H),
                    gt=[torch.tensor([[16.0, 5.0, 32.0, 35.0], [17.0, 18.0, 21.0, 22.0]]),
                        torch.tensor([[12.0, 17.0, 28.0, 47.0], [19.0, 25.0, 21.0, 29.0]])],
                    head={}, assigner=dict(gt_max_assign_all=False, pos_iou_thr=0.9, neg_iou_thr=0.3)))
    return out


def main():
    if not _ref_import.available():
        print('reference not present: nothing to do')
        return
    ref = _ref_import.install_shim(build_ref.load_ext())
    v3 = import_v3(ref)
    gen = torch.Generator().manual_seed(47)
    data, meta = {}, []
    for case in cases(gen):
        name, C = case['name'], case['C']
        W, H = case['size']
        hcfg = dict(case['head'])
        losses = hcfg.pop('losses', RECIPE_LOSSES)
        acfg = dict(dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0), **case['assigner'])
        head = v3.head.YOLOV3Head(num_classes=C, in_channels=[8, 8, 8], out_channels=[8, 8, 8],
                                  train_cfg=ref.ConfigDict(assigner=acfg), **losses, **hcfg)
        N = len(case['gt'])
        sizes = [(H // s, W // s) for s in (32, 16, 8)]
        preds = [(torch.randn(N, 3 * (5 + C), h, w, generator=gen) * 2.0).requires_grad_(True) for h, w in sizes]
        labels = [torch.randint(0, C, (len(b),), generator=gen) for b in case['gt']]
        recorded = []
        assign = head.assigner.assign

        def spy(*a, **k):
            r = assign(*a, **k)
            recorded.append(r.gt_inds.clone())
            return r
        head.assigner.assign = spy
        out = head.loss(preds, case['gt'], labels, [dict() for _ in range(N)])
        mat = torch.stack([torch.stack([x.reshape(()) for x in out[k]]) for k in ('loss_cls', 'loss_conf', 'loss_xy',
                                                                                   'loss_wh')], 1)
        gout = torch.rand(3, 4, generator=gen) + 0.5
        grads = torch.autograd.grad((mat * gout).sum(), preds)
        p = name + '/'
        for l in range(3):
            data[p + f'pred{l}'] = preds[l].detach().numpy()
            data[p + f'grad{l}'] = grads[l].numpy()
        for n in range(N):
            data[p + f'gt{n}'] = case['gt'][n].numpy().astype(np.float32)
            data[p + f'label{n}'] = labels[n].numpy()
            data[p + f'assigned{n}'] = recorded[n].numpy().astype(np.int32)
        data[p + 'losses'] = mat.detach().numpy()
        data[p + 'gout'] = gout.numpy()
        meta.append(dict(name=name, C=C, N=N, head=hcfg, losses=losses, assigner=acfg))
        pos = [int((r > 0).sum()) for r in recorded]
        print(name, 'positives', pos, 'negatives', [int((r == 0).sum()) for r in recorded], 'losses',
              mat.detach().numpy().round(3).tolist())
    # torch.max(dim) takes the FIRST maximum on ties (pinned by the 'dup' case's assignments)
    assert int(torch.tensor([[0.5], [0.5]]).max(dim=0)[1]) == 0
    data['meta'] = np.array(json.dumps(meta))
    out = os.path.join(HERE, 'v3_loss.npz')
    np.savez_compressed(out, **data)
    print('v3 loss', out, f'{os.path.getsize(out) / 1e6:.2f} MB')


if __name__ == '__main__':
    main()
