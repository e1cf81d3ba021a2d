"""What tests/test_gpu_eval_hook.py and its two-rank worker share: the tiny detectors of tests/test_gpu_dist_test.py and
tests/test_gpu_v3.py with random weights, five images of different sizes, a loader over the fused input pipeline and a
small synthetic ``CocoGt``.

``lift_head`` makes the random detector produce something to order: the head's weights are random, scaled so that a
noise image's logits have unit spread; its class biases go to +10 (class scores ~1); and the objectness bias is solved
from the network's own response so that, at ``score_thr=0.001``, the flattest image (a constant one) stays just below
the threshold everywhere -- no detection -- while every other image has positions above it."""
import math

import numpy as np
import torch

import mmdet_yolov4_amd as pkg

SCORE_THR = 0.001
NUM_CLASSES = 3
SIZE = 5
IMG_IDS = [31, 7, 19, 4, 23]               # not sorted: positions and ids differ
CAT_IDS = [5, 2, 9]


def make_test_cfg(max_per_img=30, split_thr=None, v3=False):
    nms = dict(type='nms', iou_threshold=0.65)
    if split_thr is not None:
        nms['split_thr'] = split_thr
    cfg = dict(nms_pre=-1, score_thr=SCORE_THR, nms=nms, max_per_img=max_per_img)
    if v3:
        # yolo_head.py:330-370: score_thr is tested on the class scores BEFORE the objectness multiplies them; what
        # filters by objectness is conf_thr, so it carries the threshold here
        cfg.update(min_bbox_size=0, conf_thr=SCORE_THR)
    return cfg


def tiny_v4(cfg, dev, seed=0):
    torch.manual_seed(seed)
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[['conv', 'bottleneck', 'csp', 'csp'], [None, 1, 1, 1], [8, 16, 16, 32]],
                      out_indices=[1, 2, 3]),
        neck=dict(type='YOLOV4Neck', in_channels=[16, 16, 32], out_channels=[16, 16, 32], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=NUM_CLASSES, in_channels=[16, 16, 32], featmap_strides=[4, 8, 16],
                       anchor_generator=dict(type='YOLOV4AnchorGenerator', strides=[4, 8, 16],
                                             base_sizes=[[(8, 8)] * 3, [(16, 16)] * 3, [(32, 32)] * 3])),
        train_cfg=None, test_cfg=cfg))
    det.init_weights()
    return det.eval().to(dev)


class TinyDarknet(pkg.Darknet):
    arch_settings = {53: ((1, 1, 2, 2, 1), ((32, 16), (16, 32), (32, 32), (32, 64), (64, 64)))}


def tiny_v3(cfg, dev, seed=0):
    torch.manual_seed(seed)
    det = pkg.YOLOV3(backbone=dict(type='Darknet', depth=53, out_indices=(3, 4, 5)),
                     neck=dict(type='YOLOV3Neck', num_scales=3, in_channels=[1024, 512, 256], out_channels=[512, 256, 128]),
                     bbox_head=dict(type='YOLOV3Head', num_classes=NUM_CLASSES, in_channels=[512, 256, 128],
                                    out_channels=[1024, 512, 256]), test_cfg=cfg)
    det.backbone = TinyDarknet(depth=53, out_indices=(3, 4, 5))
    det.neck = pkg.YOLOV3Neck(num_scales=3, in_channels=[64, 64, 32], out_channels=[64, 32, 16])
    det.bbox_head = pkg.YOLOV3Head(num_classes=NUM_CLASSES, in_channels=[64, 32, 16], out_channels=[96, 64, 32],
                                   test_cfg=cfg)
    return det.eval().to(dev)


def images():
    """Four noise images and a constant one (index 2), all of different sizes."""
    rng = np.random.default_rng(7)
    out = [rng.integers(0, 256, (90 + 10 * i, 140 - 6 * i, 3), dtype=np.uint8) for i in range(SIZE)]
    out[2] = np.full_like(out[2], 114)
    return out


class Loader:
    """A test loader over ``FusedTestPipeline``: the dataset positions ``indices`` in batches of ``batch`` (the last one
    ragged), each item nested per augmentation as the reference's collate does; ``.dataset`` is what it scores against."""

    def __init__(self, pipe, imgs, indices, batch=2, dataset=None):
        self.pipe, self.imgs, self.indices, self.batch, self.dataset = pipe, imgs, list(indices), batch, dataset

    def __iter__(self):
        for lo in range(0, len(self.indices), self.batch):
            batch, metas = self.pipe([self.imgs[i] for i in self.indices[lo:lo + self.batch]])
            yield dict(img=[batch], img_metas=[metas])


def lift_head(det, loader, seed=3):
    """See the module docstring.  ``loader``: the batches the test loop will see -- an image's response depends a little
    on the canvas its batch gives it, so the response is taken on that canvas.  Returns the position of the image that
    is left without detections."""
    head = det.bbox_head
    attr = 5 + NUM_CLASSES
    gen = torch.Generator().manual_seed(seed)

    def conf_maps():
        for data in loader:
            maps = det.forward_dummy(data['img'][0])[0]
            for n in range(maps[0].shape[0]):
                yield [m[n].reshape(-1, attr, m.shape[2], m.shape[3])[:, 4] for m in maps]
    with torch.no_grad():
        for conv in head.convs_pred:
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen))
            conv.bias.zero_()
        # a noise image's objectness logits get unit spread, whatever the random backbone's feature scale is
        spread = torch.cat([m.reshape(-1) for m in next(conf_maps())]).std()
        for conv in head.convs_pred:
            conv.weight.div_(spread)
            conv.bias.view(-1, attr)[:, 5:] = 10.0
        peak = [max(float(m.max()) for m in maps) for maps in conf_maps()]
        order = np.argsort(peak)
        gap = peak[order[1]] - peak[order[0]]
        # the threshold sits a quarter of the gap above the flattest image's peak: far more than the 5e-5 the class
        # score's sigmoid(10) takes off a logit and than fp32 rounding between two plans of one layer (~1e-6)
        assert gap > 0.01, f'the flattest image is not separated from the rest: {peak}'
        bias = math.log(SCORE_THR / (1 - SCORE_THR)) - peak[order[0]] - 0.25 * gap
        for conv in head.convs_pred:
            conv.bias.view(-1, attr)[:, 4] = bias
    return int(order[0])


def synthetic_gt(results, imgs):
    """A small annotation set: per image its first two detections (so that the metric is not all zeros) and two boxes
    that match nothing, one of them a crowd.  ``results``: the list form over all images."""
    rng = np.random.default_rng(11)
    anns = []
    for pos, (res, img) in enumerate(zip(results, imgs)):
        h, w = img.shape[:2]
        rows = [(c, r) for c, arr in enumerate(res) for r in arr][:2]
        boxes = [(c, [float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1])], 0) for c, r in rows]
        for crowd in (0, 1):
            x, y = rng.uniform(0, w / 2), rng.uniform(0, h / 2)
            boxes.append((int(rng.integers(0, NUM_CLASSES)), [float(x), float(y), float(rng.uniform(4, w / 2)),
                                                               float(rng.uniform(4, h / 2))], crowd))
        for c, box, crowd in boxes:
            anns.append(dict(id=len(anns) + 1, image_id=IMG_IDS[pos], category_id=CAT_IDS[c], bbox=box,
                             area=box[2] * box[3], iscrowd=crowd))
    return pkg.CocoGt(dict(images=[dict(id=i) for i in IMG_IDS],
                           categories=[dict(id=c, name=f'c{c}') for c in CAT_IDS], annotations=anns))
