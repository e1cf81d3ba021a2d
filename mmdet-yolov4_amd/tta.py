"""Test-time augmentation of ``YOLOV3Head`` on the GPU: ``BBoxTestMixin.aug_test_bboxes``
(``mmdet/models/dense_heads/dense_test_mixins.py:38-100``) after the network.

Per augmentation group (the augmentations that share one padded input shape -- an image and its flips -- run as one
batch of ``N * len(group)`` rows, augmentation-major): ``yv4_decode_filter_v3`` decodes every box (no rescale, no
candidates), ``yv4_conf_topk_levels`` finds each level's ``nms_pre`` admission key and ``yv4_topk_slots`` lists the
boxes of ``get_bboxes(with_nms=False)`` in the reference's order (levels concatenated, a cut level in descending
objectness).  Then ONE ``yv4_tta_merge`` over every augmentation maps the boxes back (``bbox_flip`` over the
augmentation's ``img_shape``, ``/ scale_factor``) and emits the candidate keys of the merged list, and
``yv4_nms_images`` (``yv4_nms_split`` past ``split_thr``) runs ``multiclass_nms`` with ``score_factors = conf``.
Everything is appended to a ``Plan`` on one stream, so a TTA plan captures into one hipGraph.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import LevelDesc, TtaAug, check


def slot_count(level_sizes, nms_pre):
    """S of ``yv4_topk_slots``: a level keeps nms_pre boxes when it has more, else all of them."""
    return sum(nms_pre if 0 < nms_pre < n else n for n in level_sizes)


def _levels(plan, views, strides, base_anchors, A):
    levels = (LevelDesc * len(views))()
    plan.params.append(levels)

    def fill():
        for i, v in enumerate(views):
            levels[i].pred = v.buf.ptr()
            levels[i].H, levels[i].W, levels[i].stride = v.H, v.W, int(strides[i])
            ba = base_anchors[i].float().cpu()
            for a in range(A):
                for c in range(4):
                    levels[i].base_anchors[a][c] = float(ba[a, c])
    return levels, fill


def emit_decode_slots(plan, views, strides, base_anchors, num_classes, nms_pre, res, tag):
    """Decode + slot table of one batch of pred maps (dense NHWC fp32 views).  Fills ``res[tag]`` at allocation with
    boxes (B, total, 4), conf (B, total), cls (B, total, C), slots (B, S); returns the fill function."""
    B = views[0].N
    A = base_anchors[0].shape[0]
    attr = 5 + num_classes
    sizes = []
    for v in views:
        assert v.buf.dtype == torch.float32, 'decode reads fp32 pred maps (emit the head convs with out_f32)'
        assert v.C == A * attr and v.coff == 0 and v.cstride == v.C, 'pred maps must be dense NHWC'
        sizes.append(v.H * v.W * A)
    total = sum(sizes)
    S = slot_count(sizes, nms_pre)
    cut = any(0 < nms_pre < n for n in sizes)
    nl = len(views)
    levels, fill_levels = _levels(plan, views, strides, base_anchors, A)
    sizes_c = (C.c_int32 * nl)(*sizes)
    plan.params.append(sizes_c)
    d = dict(B=B, total=total, S=S, sizes=sizes)
    res[tag] = d

    def alloc():
        dev = plan.device
        d['boxes'] = torch.empty((B, total, 4), dtype=torch.float32, device=dev)
        d['conf'] = torch.empty((B, total), dtype=torch.float32, device=dev)
        d['cls'] = torch.empty((B, total, num_classes), dtype=torch.float32, device=dev)
        d['slots'] = torch.empty((B, S), dtype=torch.int32, device=dev)
        # yv4_decode_filter_v3 wants a key buffer: score_thr 1.0 admits nothing (sigmoid > 1 never holds)
        d['dummy_keys'] = torch.empty(1, dtype=torch.int64, device=dev)
        d['dummy_counts'] = torch.zeros(B, dtype=torch.int32, device=dev)
        d['dummy_max'] = torch.zeros(B, dtype=torch.float32, device=dev)
        if cut:
            nb = _lib.lib().yv4_conf_topk_levels_work(B, total, nl)
            if nb == 0:
                raise RuntimeError('yv4_conf_topk_levels_work: batch * anchors too large for the top-k pre-selection')
            d['topk_work'] = torch.empty(nb, dtype=torch.uint8, device=dev)
            d['topk_keys'] = torch.zeros(B * nl, dtype=torch.int64, device=dev)
        ws = _lib.lib().yv4_topk_slots_work(nl, sizes_c, int(nms_pre))
        d['slot_work'] = torch.empty(max(ws, 256), dtype=torch.uint8, device=dev) if ws else None
        fill_levels()

    def decode(stream):
        check(_lib.lib().yv4_decode_filter_v3(
            levels, nl, B, A, num_classes, 1.0, -1.0, None, d['boxes'].data_ptr(), d['conf'].data_ptr(),
            d['cls'].data_ptr(), d['dummy_keys'].data_ptr(), 1, d['dummy_counts'].data_ptr(), d['dummy_max'].data_ptr(),
            None, stream), 'yv4_decode_filter_v3')

    def topk(stream):
        check(_lib.lib().yv4_conf_topk_levels(levels, nl, B, A, num_classes, int(nms_pre), d['topk_work'].data_ptr(),
                                              d['topk_keys'].data_ptr(), stream), 'yv4_conf_topk_levels')

    def slots(stream):
        check(_lib.lib().yv4_topk_slots(
            d['conf'].data_ptr(), B, total, nl, sizes_c, int(nms_pre), d['topk_keys'].data_ptr() if cut else None,
            d['slot_work'].data_ptr() if d['slot_work'] is not None else None, d['slots'].data_ptr(), S, stream),
            'yv4_topk_slots')
    from .plan import Op
    plan.ops.append(Op('decode', f'tta_decode_{tag}', decode, nbytes=4.0 * B * total * attr))
    if cut:
        plan.ops.append(Op('topk', f'tta_topk_{tag}', topk))
    plan.ops.append(Op('slots', f'tta_slots_{tag}', slots))
    return alloc


def emit_tta_post(plan, head, groups, flips, N, cfg=None):
    """Append the TTA post-processing to ``plan``.  ``groups``: list of (pred views of one batch, augmentation indices
    in batch order); augmentation a of group g is rows [r*N, (r+1)*N) of its batch, r its position in the group.
    ``flips``: the YV4_FLIP_* code per augmentation.  Sets and returns ``plan.post`` (collect_results' layout)."""
    _lib.require('tta', 'test-time augmentation')
    cfg = head.test_cfg if cfg is None else cfg
    spec = ops.nms_spec(cfg['nms'])                  # "nms" or "soft_nms"; other types raise
    num_augs = len(flips)
    if num_augs > _lib.TTA_MAX_AUGS:
        raise NotImplementedError(f'at most {_lib.TTA_MAX_AUGS} test-time augmentations are built, got {num_augs}')
    C_ = head.num_classes
    nms_pre = int(cfg.get('nms_pre', -1))
    res = dict(N=N, num_classes=C_, max_per_img=cfg['max_per_img'], score_thr=cfg['score_thr'],
               iou_thr=spec['iou_thr'], split_thr=spec['split_thr'], num_augs=num_augs, flips=list(flips), nms=spec)
    allocs = []
    where = [None] * num_augs
    for g, (views, augs) in enumerate(groups):
        assert views[0].N == N * len(augs), 'a group batch holds N rows per augmentation'
        allocs.append(emit_decode_slots(plan, views, head.featmap_strides, head.anchor_generator.base_anchors, C_,
                                        nms_pre, res, f'g{g}'))
        for r, a in enumerate(augs):
            where[a] = (f'g{g}', r)
    assert all(w is not None for w in where), 'every augmentation belongs to one group'
    S_total = sum(res[t]['S'] for t, _ in where)
    res['S_total'] = res['total_anchors'] = S_total
    res['key_cap'] = S_total * C_
    table = (TtaAug * num_augs)()
    plan.params.append(table)

    def alloc():
        dev = plan.device
        for f in allocs:
            f()
        for a, (t, r) in enumerate(where):
            d = res[t]
            tot, S = d['total'], d['S']
            table[a].boxes = d['boxes'].data_ptr() + r * N * tot * 16
            table[a].conf = d['conf'].data_ptr() + r * N * tot * 4
            table[a].cls = d['cls'].data_ptr() + r * N * tot * C_ * 4
            table[a].slots = d['slots'].data_ptr() + r * N * S * 4
            table[a].total, table[a].S, table[a].flip = tot, S, int(flips[a])
        res['meta'] = torch.zeros((num_augs, N, 6), dtype=torch.float32, device=dev)
        res['boxes'] = torch.empty((N, S_total, 4), dtype=torch.float32, device=dev)
        res['keys'] = torch.empty((N, res['key_cap']), dtype=torch.int64, device=dev)
        res['counts'] = torch.zeros(N, dtype=torch.int32, device=dev)
        res['max_coord'] = torch.zeros(N, dtype=torch.float32, device=dev)
        res['dets'] = torch.zeros((N, res['max_per_img'], 5), dtype=torch.float32, device=dev)
        res['labels'] = torch.zeros((N, res['max_per_img']), dtype=torch.int32, device=dev)
        res['index'] = torch.zeros((N, res['max_per_img']), dtype=torch.int64, device=dev)
        res['count'] = torch.zeros(N, dtype=torch.int32, device=dev)
    res['_alloc'] = alloc

    def merge(stream):
        check(_lib.lib().yv4_decode_reset(res['counts'].data_ptr(), res['max_coord'].data_ptr(), N, stream),
              'yv4_decode_reset')
        check(_lib.lib().yv4_tta_merge(table, num_augs, N, C_, float(res['score_thr']), res['meta'].data_ptr(),
                                       res['boxes'].data_ptr(), res['keys'].data_ptr(), res['key_cap'],
                                       res['counts'].data_ptr(), res['max_coord'].data_ptr(), stream), 'yv4_tta_merge')

    from .plan import Op
    plan.ops.append(Op('merge', 'tta_merge', merge))
    plan.ops.append(Op('nms', ops.POST_NMS_KERNEL[spec['type']], lambda stream: ops.post_nms(res, stream)))
    plan.post = res
    return res


def set_tta_metas(post, img_metas):
    """img_metas[a][n] -> the (num_augs, N, 6) meta rows img_h, img_w, scale_factor of yv4_tta_merge."""
    A, N = post['num_augs'], post['N']
    if len(img_metas) != A or any(len(m) != N for m in img_metas):
        raise ValueError(f'img_metas must be {A} augmentations x {N} images')
    rows = np.zeros((A, N, 6), dtype=np.float32)
    for a in range(A):
        for n, m in enumerate(img_metas[a]):
            code = flip_code(m)
            if code != post['flips'][a]:
                raise ValueError(f'augmentation {a} was planned with flip code {post["flips"][a]}, meta says {code}')
            sf = np.asarray(m['scale_factor'], dtype=np.float32).reshape(-1)
            if sf.size == 1:
                sf = np.repeat(sf, 4)
            rows[a, n, 0], rows[a, n, 1] = m['img_shape'][0], m['img_shape'][1]
            rows[a, n, 2:] = sf
    post['meta'].copy_(torch.from_numpy(rows), non_blocking=False)


def flip_code(meta):
    if not meta.get('flip', False):
        return _lib.FLIP_NONE
    d = meta.get('flip_direction', 'horizontal')
    if d not in _lib.FLIP_CODES:
        raise ValueError(f'flip_direction {d!r} is not one of {sorted(_lib.FLIP_CODES)}')
    return _lib.FLIP_CODES[d]


def collect_tta(post, img_metas, rescale, num_classes):
    """multiclass_nms results -> one per-class list per image; rescale=False multiplies the boxes by augmentation 0's
    scale_factor again (dense_test_mixins.py:93-98: divide-then-multiply, as the reference does)."""
    from .single_stage import bbox2result
    from .yolocsp_head import collect_results
    out = []
    for n, (d, l) in enumerate(collect_results(post, with_nms=True)):
        if not rescale and d.shape[0]:
            d = d.clone()
            sf = np.asarray(img_metas[0][n]['scale_factor'], dtype=np.float32)
            d[:, :4] *= d.new_tensor(sf)
        out.append(bbox2result(d, l, num_classes))
    return out
