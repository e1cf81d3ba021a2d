"""Loss side of ``YOLOCSPHead`` (training).

Mirror of ``mmdet/models/dense_heads/yolocsp_head.py:384-575`` (``loss``,
``loss_single_no_assigner``, ``get_targets_no_assigner``), ``GIoULoss`` / ``giou_loss``
(``mmdet/models/losses/iou_loss.py:85-102,330-366``), aligned GIoU of
``mmdet/core/bbox/iou_calculators/iou2d_calculator.py:74-260`` and sigmoid
``CrossEntropyLoss`` (``mmdet/models/losses/cross_entropy_loss.py:58-91,142-214``).

The training step's default configuration (sigmoid BCE + GIoU, no assigner) runs on the fused HIP loss
(``csrc/loss.hip`` via ``YoloLossFunction`` in ``yolocsp_head.py``).  The classes here are the registry
entries the configs name, the tensor-op statement of the same arithmetic (used for dense pred maps,
non-default loss settings and as the GPU-side cross-check in the tests) and YOLOV3Head's losses.
"""
import math

import torch
import torch.nn.functional as F

from .registry import LOSSES


def bbox_overlaps_giou_aligned(b1, b2, eps=1e-6):
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt = torch.max(b1[..., :2], b2[..., :2])
    rb = torch.min(b1[..., 2:], b2[..., 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    e = b1.new_tensor([eps])
    union = torch.max(area1 + area2 - overlap, e)
    ious = overlap / union
    ewh = (torch.max(b1[..., 2:], b2[..., 2:]) - torch.min(b1[..., :2], b2[..., :2])).clamp(min=0)
    earea = torch.max(ewh[..., 0] * ewh[..., 1], e)
    return ious - (earea - union) / earea


def bbox_overlaps(b1, b2, eps=1e-6):
    """Pairwise IoU, core/bbox/iou_calculators/iou2d_calculator.py:74-260 (mode='iou', is_aligned=False):
    (m,4) x (n,4) -> (m,n)."""
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt = torch.max(b1[..., :, None, :2], b2[..., None, :, :2])
    rb = torch.min(b1[..., :, None, 2:], b2[..., None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[..., None] + area2[..., None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    """losses/utils.py:27-54."""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return reduce_loss(loss, reduction)
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction != 'none':
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


def reduce_loss(loss, reduction):
    if reduction == 'none':
        return loss
    if reduction == 'mean':
        return loss.mean()
    if reduction == 'sum':
        return loss.sum()
    raise ValueError(reduction)


@LOSSES.register_module()
class GIoULoss(torch.nn.Module):

    def __init__(self, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.eps, self.reduction, self.loss_weight = eps, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert weight is None and avg_factor is None, 'weighted GIoU is not used by this head'
        reduction = reduction_override if reduction_override else self.reduction
        loss = 1 - bbox_overlaps_giou_aligned(pred, target, eps=self.eps)
        return self.loss_weight * reduce_loss(loss, reduction)


def bbox_overlaps_iou_aligned(b1, b2, eps=1e-6):
    """iou2d_calculator.py:74-260, mode='iou', is_aligned=True (``eps`` is the lower bound of the union)."""
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt = torch.max(b1[..., :2], b2[..., :2])
    rb = torch.min(b1[..., 2:], b2[..., 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.max(area1 + area2 - overlap, b1.new_tensor([eps]))
    return overlap / union


def iou_loss(pred, target, linear=False, eps=1e-6):
    """iou_loss.py:14-36: the aligned IoU (its own union bound stays at the calculator's 1e-6) clamped at ``eps``."""
    ious = bbox_overlaps_iou_aligned(pred, target).clamp(min=eps)
    return 1 - ious if linear else -ious.log()


def _ious_c2(pred, target, eps):
    """The first half iou_loss.py:121-143 and :177-199 share: (ious, c2).  ``eps`` is ADDED to the union and to c2."""
    lt = torch.max(pred[:, :2], target[:, :2])
    rb = torch.min(pred[:, 2:], target[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    ag = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    union = ap + ag - overlap + eps
    ious = overlap / union
    enclose_x1y1 = torch.min(pred[:, :2], target[:, :2])
    enclose_x2y2 = torch.max(pred[:, 2:], target[:, 2:])
    enclose_wh = (enclose_x2y2 - enclose_x1y1).clamp(min=0)
    cw, ch = enclose_wh[:, 0], enclose_wh[:, 1]
    return ious, cw ** 2 + ch ** 2 + eps


def _corners(b):
    return b[:, 0], b[:, 1], b[:, 2], b[:, 3]


def _rho2(p, t):
    """Squared centre distance, as ``((t_x1 + t_x2) - (p_x1 + p_x2))**2 / 4`` per axis."""
    left = ((t[0] + t[2]) - (p[0] + p[2])) ** 2 / 4
    right = ((t[1] + t[3]) - (p[1] + p[3])) ** 2 / 4
    return left + right


def diou_loss(pred, target, eps=1e-7):
    """iou_loss.py:105-157."""
    ious, c2 = _ious_c2(pred, target, eps)
    rho2 = _rho2(_corners(pred), _corners(target))
    return 1 - (ious - rho2 / c2)


def ciou_loss(pred, target, eps=1e-7):
    """iou_loss.py:160-219: ``eps`` also goes onto both heights before the atan, and the trade-off term is
    ``v**2 / (1 - ious + v)`` with the gradient through all of it (nothing detached).  Where that term is 0 / 0
    (``ious == 1`` and ``v == 0``) the result is nan, as in the reference."""
    ious, c2 = _ious_c2(pred, target, eps)
    p, t = _corners(pred), _corners(target)
    w1, h1 = p[2] - p[0], p[3] - p[1] + eps
    w2, h2 = t[2] - t[0], t[3] - t[1] + eps
    rho2 = _rho2(p, t)
    factor = 4 / math.pi ** 2
    v = factor * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
    return 1 - (ious - (rho2 / c2 + v ** 2 / (1 - ious + v)))


class _BoxLoss(torch.nn.Module):
    """The constructor / forward shape of iou_loss.py:222-290,369-447; weighted and ``avg_factor`` forms are not used by
    this head and are refused, as in ``GIoULoss`` above."""

    def __init__(self, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.eps, self.reduction, self.loss_weight = eps, reduction, loss_weight

    def elementwise(self, pred, target):
        raise NotImplementedError

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert weight is None and avg_factor is None, f'weighted {type(self).__name__} is not used by this head'
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * reduce_loss(self.elementwise(pred, target), reduction)


@LOSSES.register_module()
class IoULoss(_BoxLoss):

    def __init__(self, linear=False, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__(eps, reduction, loss_weight)
        self.linear = linear

    def elementwise(self, pred, target):
        return iou_loss(pred, target, linear=self.linear, eps=self.eps)


@LOSSES.register_module()
class DIoULoss(_BoxLoss):

    def elementwise(self, pred, target):
        return diou_loss(pred, target, eps=self.eps)


@LOSSES.register_module()
class CIoULoss(_BoxLoss):

    def elementwise(self, pred, target):
        return ciou_loss(pred, target, eps=self.eps)


@LOSSES.register_module()
class CrossEntropyLoss(torch.nn.Module):
    """Only the ``use_sigmoid=True`` form the head uses (BCE with logits)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0):
        super().__init__()
        if not use_sigmoid or use_mask:
            raise NotImplementedError('only CrossEntropyLoss(use_sigmoid=True) is built')
        self.use_sigmoid, self.reduction, self.loss_weight, self.class_weight = True, reduction, loss_weight, class_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        """cross_entropy_loss.py:58-91 (element-wise ``weight``, ``avg_factor``) + :187-214."""
        reduction = reduction_override if reduction_override else self.reduction
        pw = cls_score.new_tensor(self.class_weight) if self.class_weight is not None else None
        loss = F.binary_cross_entropy_with_logits(cls_score, label.float(), pos_weight=pw, reduction='none')
        if weight is not None:
            weight = weight.float()
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction=reduction, avg_factor=avg_factor)


@LOSSES.register_module()
class MSELoss(torch.nn.Module):
    """losses/mse_loss.py:8-50 (``@weighted_loss`` element-wise MSE)."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        loss = F.mse_loss(pred, target, reduction='none')
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction=self.reduction, avg_factor=avg_factor)


@LOSSES.register_module()
class SoftFocalLoss(torch.nn.Module):
    """yolocsp_head.py:21-50."""

    def __init__(self, raw_loss, gamma=1.5, alpha=0.25):
        super().__init__()
        from .registry import build_loss
        self.loss_fcn = build_loss(raw_loss)
        self.gamma, self.alpha = gamma, alpha
        self.reduction = self.loss_fcn.reduction
        self.loss_fcn.reduction = 'none'

    def forward(self, pred, gt, reduction_override=None):
        loss = self.loss_fcn(pred, gt)
        p = torch.sigmoid(pred)
        p_t = gt * p + (1 - gt) * (1 - p)
        loss = loss * (gt * self.alpha + (1 - gt) * (1 - self.alpha)) * (1.0 - p_t) ** self.gamma
        return reduce_loss(loss, reduction_override if reduction_override is not None else self.reduction)
