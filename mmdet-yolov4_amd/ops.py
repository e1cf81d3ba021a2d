"""torch-tensor front ends of the C-ABI ops (``include/yv4.h``).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
number is produced by ``libyv4_hip.so``.  All wrappers require CUDA (ROCm) tensors
and raise otherwise -- there is no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16,
       torch.float64: _lib.F64}


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if not t.is_cuda:
        raise RuntimeError(
            f'{name} is on {t.device}: the yv4 ops run on an MI355X only (HIP path, no CPU fallback)')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---- Mish ---------------------------------------------------------------------------
def mish_forward(input):
    """``mish_cuda_ext.mish_forward`` (mmdet/ops/mish_cuda/src/mish.cc:14-22): new
    tensor ``empty_like(input)``; input must be contiguous.  Like the reference's dispatcher a CPU tensor runs the
    op's host loop (``yv4_mish_fwd_host``: the library's own restatement of mish.h:16-18 -- the op's CPU behaviour, not
    a path of any plan)."""
    if not isinstance(input, torch.Tensor):
        raise TypeError('input must be a torch.Tensor')
    if not input.is_contiguous():
        raise RuntimeError('mish_forward: input must be contiguous')
    if input.dtype not in _DT:
        raise RuntimeError(f'mish_forward: unsupported dtype {input.dtype}')
    out = torch.empty_like(input)
    if not input.is_cuda:
        check(_lib.lib().yv4_mish_fwd_host(_ptr(input), _ptr(out), input.numel(), _DT[input.dtype]), 'yv4_mish_fwd_host')
        return out
    check(_lib.lib().yv4_mish_fwd(_ptr(input), _ptr(out), input.numel(), _DT[input.dtype],
                                  stream_ptr()), 'yv4_mish_fwd')
    return out


def mish_backward(grad_out, input):
    """``mish_cuda_ext.mish_backward`` (mish.cc:24-33); dispatches on ``grad_out.is_cuda`` as the reference does."""
    if not (isinstance(grad_out, torch.Tensor) and isinstance(input, torch.Tensor)):
        raise TypeError('grad_out and input must be torch.Tensors')
    if grad_out.device != input.device:
        raise RuntimeError(f'mish_backward: grad_out is on {grad_out.device}, input on {input.device}')
    if not (grad_out.is_contiguous() and input.is_contiguous()):
        raise RuntimeError('mish_backward: tensors must be contiguous')
    if grad_out.dtype != input.dtype or grad_out.shape != input.shape:
        raise RuntimeError('mish_backward: grad_out and input must match in dtype and shape')
    if input.dtype not in _DT:
        raise RuntimeError(f'mish_backward: unsupported dtype {input.dtype}')
    gin = torch.empty_like(input)
    if not grad_out.is_cuda:
        check(_lib.lib().yv4_mish_bwd_host(_ptr(grad_out), _ptr(input), _ptr(gin), input.numel(), _DT[input.dtype]),
              'yv4_mish_bwd_host')
        return gin
    check(_lib.lib().yv4_mish_bwd(_ptr(grad_out), _ptr(input), _ptr(gin), input.numel(),
                                  _DT[input.dtype], stream_ptr()), 'yv4_mish_bwd')
    return gin


class MishFunction(torch.autograd.Function):
    """``MishCudaFunction`` (mmdet/ops/mish_cuda/mish.py:18-36): saves the input."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda')
    def forward(ctx, inp):
        if not inp.is_contiguous():
            inp = inp.contiguous()
        ctx.save_for_backward(inp)
        return mish_forward(inp)

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad_out):
        inp, = ctx.saved_tensors
        if not grad_out.is_contiguous():
            grad_out = grad_out.contiguous()
        if not ctx.needs_input_grad[0]:
            return (None, )
        return mish_backward(grad_out, inp)


# ---- layout -------------------------------------------------------------------------
def nchw_to_nhwc(src, dst, dst_cstride, dst_coff=0, zero_pad=0):
    N, Cc, H, W = src.shape
    check(_lib.lib().yv4_nchw_to_nhwc(_ptr(src), _ptr(dst), N, Cc, H, W, dst_cstride, dst_coff,
                                      zero_pad, stream_ptr()), 'yv4_nchw_to_nhwc')


def nhwc_to_nchw(src, dst, C_, H, W, src_cstride, src_coff=0):
    N = dst.shape[0]
    check(_lib.lib().yv4_nhwc_to_nchw(_ptr(src), _ptr(dst), N, C_, H, W, src_cstride, src_coff,
                                      stream_ptr()), 'yv4_nhwc_to_nchw')


# ---- NMS ----------------------------------------------------------------------------
SPLIT_THR_DEFAULT = 10000
FAST_NMS_CAP = 16384   # candidates one workgroup sorts in LDS (csrc/postproc.hip kSortCap)
SOFT_NMS_CAP = 10240   # candidates the soft-NMS images kernel holds in registers (csrc/soft_nms.hip kSoftRegCap)
SOFT_NMS_PROBLEM_CAP = 1 << 19   # candidates of one problem of yv4_soft_nms_split (kSoftGlobalCap)
_SOFT_NMS_ARGS = ('iou_threshold', 'sigma', 'min_score', 'method', 'offset')
POST_NMS_KERNEL = {'nms': 'nms_images', 'soft_nms': 'soft_nms_images'}     # a plan's op name per ``nms_spec`` type


def _soft_params(cfg, who):
    """mmcv soft_nms' arguments in ``cfg`` (its names; defaults 0.3 / 0.5 / 1e-3 / 'linear') -> the kernels' parameters
    ``dict(iou_thr, sigma, min_score, method)``, method as its YV4_SOFT_NMS_* code.  A key soft_nms does not take raises
    TypeError, an offset other than 0 NotImplementedError, an unknown method or sigma <= 0 with 'gaussian' ValueError."""
    bad = sorted(set(cfg) - set(_SOFT_NMS_ARGS))
    if bad:
        raise TypeError(f'{who}: soft_nms takes no nms_cfg keys {bad}')
    if cfg.get('offset', 0) != 0:
        raise NotImplementedError(f'{who}: only offset=0 is built')
    method = cfg.get('method', 'linear')
    if method not in _lib.SOFT_NMS_METHODS:
        raise ValueError(f'soft_nms: method {method!r} is not one of {sorted(_lib.SOFT_NMS_METHODS)}')
    method = _lib.SOFT_NMS_METHODS[method]
    sigma = float(cfg.get('sigma', 0.5))
    if method == _lib.SOFT_NMS_GAUSSIAN and not sigma > 0:
        raise ValueError('soft_nms: sigma must be > 0 for the gaussian method')
    return dict(iou_thr=float(cfg.get('iou_threshold', 0.3)), sigma=sigma, min_score=float(cfg.get('min_score', 1e-3)),
                method=method)


def nms_spec(nms_cfg):
    """``test_cfg.nms`` -> what a plan's post-processing launches: ``dict(type='nms', iou_thr, split_thr)`` or
    ``dict(type='soft_nms', iou_thr, sigma, min_score, method (YV4_SOFT_NMS_* code), split_thr)`` (mmcv soft_nms'
    defaults 0.3 / 0.5 / 1e-3 / 'linear').  Other types raise NotImplementedError; a soft-NMS key the op does not take
    raises TypeError.  ``max_num`` with soft-NMS (mmcv applies it in the split branch only, and the single call refuses
    it) is not built into plans."""
    cfg = dict(nms_cfg)
    nms_type = cfg.pop('type', 'nms')
    split_thr = cfg.pop('split_thr', SPLIT_THR_DEFAULT)
    if nms_type == 'nms':
        return dict(type='nms', iou_thr=cfg.get('iou_threshold', cfg.get('iou_thr')), split_thr=split_thr)
    if nms_type != 'soft_nms':
        raise NotImplementedError(f'nms type {nms_type!r} is not built ("nms", "soft_nms")')
    cfg.pop('class_agnostic', None)              # the head's own class_agnostic decides, as for "nms"
    if 'max_num' in cfg:
        raise NotImplementedError('soft_nms with max_num is not built into plans')
    return dict(_soft_params(cfg, 'soft_nms'), type='soft_nms', split_thr=split_thr)


def _nms_images(spec, keys, key_cap, counts, max_coord, boxes, boxes_per_image, labels, label_stride, fused_classes, N,
                max_out, split_thr, dets, olab, oidx, ocnt, stream):
    """``yv4_nms_images``, or ``yv4_soft_nms_images`` when ``spec['type']`` is 'soft_nms', over N images' candidate
    keys.  The buffers are device addresses (``labels`` may be None); ``spec`` as ``nms_spec`` returns it."""
    L = _lib.lib()
    head = (keys, key_cap, counts, max_coord, boxes, boxes_per_image, labels, label_stride, fused_classes, N)
    tail = (max_out, int(split_thr), dets, olab, oidx, ocnt, stream)
    if spec['type'] == 'soft_nms':
        check(L.yv4_soft_nms_images(*head, spec['method'], spec['iou_thr'], spec['sigma'], spec['min_score'], *tail),
              'yv4_soft_nms_images')
    else:
        check(L.yv4_nms_images(*head, float(spec['iou_thr']), *tail), 'yv4_nms_images')


def post_nms(post, stream):
    """The per-image NMS of a plan's post-processing dictionary (``Plan.postprocess`` / ``tta.emit_tta_post``) on
    ``stream``, hard or soft as ``post['nms']`` says: the classes are fused into the candidate index."""
    _nms_images(post['nms'], post['keys'].data_ptr(), post['key_cap'], post['counts'].data_ptr(),
                post['max_coord'].data_ptr(), post['boxes'].data_ptr(), post['total_anchors'], None, 0,
                post['num_classes'], post['N'], post['max_per_img'], post['split_thr'], post['dets'].data_ptr(),
                post['labels'].data_ptr(), post['index'].data_ptr(), post['count'].data_ptr(), stream)


def split_nms_image(spec, keys, n, max_coord, boxes, labels, fused_classes, max_out, dets, olab, oidx, ocnt, per_label=1):
    """One image's n candidates (a host value) through ``yv4_nms_split`` or, for soft-NMS, ``yv4_soft_nms_split``; the
    workspace is allocated here.  ``max_coord``: the host value of the class-offset unit minus one; -1.0 means no class
    offset (unit 0: the labels still group the candidates, as mmcv's split branch does when class_agnostic).
    ``per_label`` 0 (soft-NMS only): one problem over all candidates, in selection order."""
    L = _lib.lib()
    soft = spec['type'] == 'soft_nms'
    nbytes = int((L.yv4_soft_nms_split_work if soft else L.yv4_nms_split_work)(n))
    if nbytes == 0 or (soft and not per_label and n > SOFT_NMS_PROBLEM_CAP):
        raise NotImplementedError(f'{"soft-" if soft else ""}NMS over {n} candidates in one problem is not built'
                                  + (f' (at most {SOFT_NMS_PROBLEM_CAP})' if soft else ''))
    work = torch.empty(nbytes, dtype=torch.uint8, device=boxes.device)
    head = (_ptr(keys), n, float(max_coord), _ptr(boxes), _ptr(labels), fused_classes)
    tail = (max_out, _ptr(work), _ptr(dets), _ptr(olab), _ptr(oidx), _ptr(ocnt), stream_ptr())
    if not soft:
        check(L.yv4_nms_split(*head, float(spec['iou_thr']), *tail), 'yv4_nms_split')
        return
    check(L.yv4_soft_nms_split(*head, int(per_label), spec['method'], spec['iou_thr'], spec['sigma'], spec['min_score'],
                               *tail), 'yv4_soft_nms_split')
    if int(ocnt.item()) == -2:
        raise NotImplementedError(f'soft-NMS: a label with more than {SOFT_NMS_PROBLEM_CAP} candidates is not built')


def soft_nms_split(keys, n, max_coord, boxes, labels, fused_classes, per_label, spec, max_out, dets, olab, oidx, ocnt):
    """``split_nms_image`` for a soft-NMS parameter dict, under its earlier name and argument order."""
    split_nms_image(dict(spec, type='soft_nms'), keys, n, max_coord, boxes, labels, fused_classes, max_out, dets, olab,
                    oidx, ocnt, per_label=per_label)


def _nms_single(boxes, scores, labels, spec, max_out, split_thr, class_agnostic=False, single_in_global=False):
    """One image's boxes through yv4_nms_prepare and the NMS of ``spec`` (``nms_spec``'s dict; hard NMS needs its
    ``type`` and ``iou_thr`` only): the images kernel below split_thr, the split path per label from split_thr.  Between
    the two, soft-NMS over more than SOFT_NMS_CAP candidates is one problem in global memory; ``single_in_global`` takes
    that form at any size (tests run the same candidates through both).  No class offset when ``class_agnostic``: the
    images kernels get no labels (label 0), the split path, whose labels still group, max_coord = -1.0.  Returns
    (dets(k,5), keep(k,))."""
    soft = spec['type'] == 'soft_nms'
    n = boxes.shape[0]
    dev = boxes.device
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    counts = torch.empty(1, dtype=torch.int32, device=dev)
    maxc = torch.empty(1, dtype=torch.float32, device=dev)
    check(_lib.lib().yv4_nms_prepare(_ptr(boxes), _ptr(scores), n, _ptr(keys), _ptr(counts), _ptr(maxc), stream_ptr()),
          'yv4_nms_prepare')
    cap = max(min(max_out if max_out > 0 else n, n), 1)
    dets = torch.empty((cap, 5), dtype=torch.float32, device=dev)
    olab = torch.empty(cap, dtype=torch.int32, device=dev)
    oidx = torch.empty(cap, dtype=torch.int64, device=dev)
    ocnt = torch.empty(1, dtype=torch.int32, device=dev)
    lab = None if class_agnostic else labels
    if n < split_thr and not single_in_global and n <= (SOFT_NMS_CAP if soft else FAST_NMS_CAP):
        _nms_images(spec, _ptr(keys), n, _ptr(counts), _ptr(maxc), _ptr(boxes), n, _ptr(lab), n, 0, 1, cap, split_thr,
                    _ptr(dets), _ptr(olab), _ptr(oidx), _ptr(ocnt), stream_ptr())
    elif n < split_thr and not soft:
        raise NotImplementedError(
            f'single-call NMS over {n} > {FAST_NMS_CAP} candidates is not built '
            "(mmcv's default split_thr=10000 switches to the per-class path before that)")
    else:
        # mmcv's split branch loops over unique(idxs) even when class_agnostic (then without the coordinate offset)
        mc = -1.0 if class_agnostic else maxc.item()
        per_label = n >= split_thr
        split_nms_image(spec, keys, n, mc, boxes, labels if per_label else lab, 0, cap, dets, olab, oidx, ocnt,
                        per_label=per_label)
    k = int(ocnt.item())
    if k < 0:
        raise RuntimeError(f'yv4_{"soft_" if soft else ""}nms_images flagged the split path unexpectedly')
    return dets[:k], oidx[:k]


def _soft_single(boxes, scores, labels, spec, *args, **kwargs):
    """``_nms_single`` for a soft-NMS parameter dict (with or without its ``type``)."""
    return _nms_single(boxes, scores, labels, dict(spec, type='soft_nms'), *args, **kwargs)


def _no_detections(boxes):
    return boxes.new_zeros((0, 5)), torch.zeros((0,), dtype=torch.int64, device=boxes.device)


def nms(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1):
    """``mmcv.ops.nms.nms`` (1.3.x signature).  ``offset`` must be 0 (the only value the
    reference's configs use).  Returns ``(dets(k,5), keep(k,) int64)`` ordered by
    descending score, ties by ascending index."""
    assert boxes.size(1) == 4
    assert boxes.size(0) == scores.size(0)
    if offset != 0:
        raise NotImplementedError('nms: only offset=0 is built')
    _need_cuda(boxes, 'boxes')
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    inds = None
    if score_threshold > 0:
        valid = scores > score_threshold
        inds = valid.nonzero(as_tuple=False).squeeze(1)
        boxes, scores = boxes[inds].contiguous(), scores[inds].contiguous()
    if boxes.shape[0] == 0:
        return _no_detections(boxes)
    dets, keep = _nms_single(boxes, scores, None, dict(type='nms', iou_thr=iou_threshold), max_num, 1 << 30, True)
    if inds is not None:
        keep = inds[keep]
    return dets, keep


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', offset=0):
    """``mmcv.ops.nms.soft_nms`` (1.3.x signature; the definition in include/yv4.h).  Device tensors only, ``offset``
    must be 0.  Returns ``(dets(k,5), inds(k,) int64)`` in selection order: the boxes as given and the DECAYED scores."""
    assert boxes.size(1) == 4
    assert boxes.size(0) == scores.size(0)
    spec = dict(_soft_params(dict(iou_threshold=iou_threshold, sigma=sigma, min_score=min_score, method=method,
                                  offset=offset), 'soft_nms'), type='soft_nms')
    _need_cuda(boxes, 'boxes')
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    if boxes.shape[0] == 0:
        return _no_detections(boxes)
    return _nms_single(boxes, scores, None, spec, -1, 1 << 30, True)


def _batched_soft_nms(boxes, scores, idxs, nms_cfg_, class_agnostic):
    """batched_nms with type='soft_nms' (mmcv 1.3.x, the decayed split form): below split_thr one soft_nms over the
    class-offset boxes with the decayed scores in selection order; from split_thr one soft_nms per label, survivors
    re-sorted by decayed score (ties to the lower index) and cut to ``max_num``.  ``max_num`` below split_thr is a key
    soft_nms does not take (TypeError), as in mmcv."""
    split_thr = nms_cfg_.pop('split_thr', SPLIT_THR_DEFAULT)
    n = boxes.shape[0]
    max_num = -1
    if n >= split_thr:
        max_num = nms_cfg_.pop('max_num', -1)
    spec = dict(_soft_params(nms_cfg_, 'batched_nms'), type='soft_nms')
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    if n == 0:
        return _no_detections(boxes)
    labels = idxs.to(device=boxes.device, dtype=torch.int32).contiguous()
    return _nms_single(boxes, scores, labels, spec, max_num, split_thr, class_agnostic)


def set_deterministic(on=True):
    """``yv4_set_deterministic``: every floating-point sum that meets in atomics (BatchNorm statistics and their backward,
    loss sums and row gradients, bias gradients, the SPP scatter, the gradient norm) runs on fixed-point integer words or
    in a fixed order, so a training step gives the same bits run to run (the weight gradient's ordered form is this
    host's default already).  The counterpart of ``torch.use_deterministic_algorithms`` for the reference's step, whose
    BatchNorm (torch.nn.BatchNorm2d via mmdet/models/backbones/darknetcsp.py:15-35) is deterministic.  Process-wide;
    switch it between steps."""
    check(_lib.lib().yv4_set_deterministic(1 if on else 0), 'yv4_set_deterministic')


def deterministic():
    return bool(_lib.lib().yv4_get_deterministic())


def set_nms_iou_form(form):
    """Choose which of mmcv-full 1.3.x's two suppression predicates every NMS launch of this process applies:
    'div' (default) -- ``inter / (Sa + Sb - inter) > thr``, mmcv's CPU kernel and the documented definition of this
    package; 'mul' -- ``inter > thr * (Sa + Sb - inter)``, mmcv's CUDA kernel, i.e. what the reference executes on a GPU.
    They select differently only on pairs whose fp32 IoU rounds across the threshold (tests/golden/nms_boundary.npz).
    Also settable through the environment: ``YV4_NMS_IOU_FORM=mul``."""
    code = {'div': _lib.NMS_IOU_DIV, 'mul': _lib.NMS_IOU_MUL, 0: 0, 1: 1}[form]
    check(_lib.lib().yv4_nms_set_iou_form(code), 'yv4_nms_set_iou_form')


def get_nms_iou_form():
    return {0: 'div', 1: 'mul'}[_lib.lib().yv4_nms_get_iou_form()]


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """``mmcv.ops.nms.batched_nms`` as called at
    mmdet/core/post_processing/bbox_nms.py:84.  ``idxs`` may live on the CPU (Q6)."""
    _need_cuda(boxes, 'boxes')
    nms_cfg_ = dict(nms_cfg)
    class_agnostic = nms_cfg_.pop('class_agnostic', class_agnostic)
    nms_type = nms_cfg_.pop('type', 'nms')
    if nms_type == 'soft_nms':
        return _batched_soft_nms(boxes, scores, idxs, nms_cfg_, class_agnostic)
    if nms_type != 'nms':
        raise NotImplementedError(f'batched_nms: nms type {nms_type!r} is not built ("nms", "soft_nms")')
    split_thr = nms_cfg_.pop('split_thr', SPLIT_THR_DEFAULT)
    iou_threshold = nms_cfg_.pop('iou_threshold', nms_cfg_.pop('iou_thr', None))
    if iou_threshold is None:
        raise KeyError('batched_nms: nms_cfg needs iou_threshold')
    score_threshold = nms_cfg_.pop('score_threshold', 0)
    max_num = nms_cfg_.pop('max_num', -1)
    if nms_cfg_.pop('offset', 0) != 0:
        raise NotImplementedError('batched_nms: only offset=0 is built')
    if nms_cfg_:
        raise TypeError(f'batched_nms: unexpected nms_cfg keys {sorted(nms_cfg_)}')
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    if boxes.shape[0] == 0:
        return _no_detections(boxes)
    labels = idxs.to(device=boxes.device, dtype=torch.int32).contiguous()
    inds = None
    if score_threshold > 0:
        inds = (scores > score_threshold).nonzero(as_tuple=False).squeeze(1)
        boxes, scores, labels = boxes[inds].contiguous(), scores[inds].contiguous(), labels[inds].contiguous()
        if boxes.shape[0] == 0:
            return _no_detections(boxes)
    dets, keep = _nms_single(boxes, scores, labels, dict(type='nms', iou_thr=iou_threshold), max_num, split_thr,
                             class_agnostic)
    if inds is not None:
        keep = inds[keep]
    return dets, keep


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None,
                   return_inds=False):
    """``mmdet/core/post_processing/bbox_nms.py:7-93``; same shapes incl. the empty
    case (Q7: boxes ``(0,4)``, labels int64 ``(0,)``)."""
    num_classes = multi_scores.size(1) - 1
    if multi_bboxes.shape[1] > 4:
        bboxes = multi_bboxes.view(multi_scores.size(0), -1, 4)
    else:
        bboxes = multi_bboxes[:, None].expand(multi_scores.size(0), num_classes, 4)
    scores = multi_scores[:, :-1]
    labels = torch.arange(num_classes, dtype=torch.long)  # on the CPU, as in the reference (Q6)
    labels = labels.view(1, -1).expand_as(scores)
    bboxes = bboxes.reshape(-1, 4)
    scores = scores.reshape(-1)
    labels = labels.reshape(-1)
    valid_mask = scores > score_thr
    if score_factors is not None:
        score_factors = score_factors.view(-1, 1).expand(multi_scores.size(0), num_classes)
        scores = scores * score_factors.reshape(-1)
    inds = valid_mask.nonzero(as_tuple=False).squeeze(1)
    bboxes, scores, labels = bboxes[inds], scores[inds], labels.to(inds.device)[inds]
    if bboxes.numel() == 0:
        if return_inds:
            return bboxes, labels, inds
        return bboxes, labels
    dets, keep = batched_nms(bboxes, scores, labels, nms_cfg)
    if max_num > 0:
        dets = dets[:max_num]
        keep = keep[:max_num]
    if return_inds:
        return dets, labels[keep], keep
    return dets, labels[keep]
