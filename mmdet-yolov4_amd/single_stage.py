"""``SingleStageDetector`` under the reference's registry name.

Mirror of ``mmdet/models/detectors/single_stage.py:35-112`` and the parts of
``mmdet/models/detectors/base.py:111-169`` an inference caller touches
(``forward(return_loss=False)`` -> ``forward_test`` -> ``simple_test``), with
``bbox2result`` of ``mmdet/core/bbox/transforms.py:99-113``.

``simple_test`` replays ONE plan for the whole pipeline -- NCHW->NHWC, 115 fused convs,
SPP, 2 upsamples, decode+filter, NMS -- built once per (batch, height, width) by
``compile``; the host touches the device twice per batch (scale factors in, detections
out).
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from .bricks import HipModule, plan_cache_get, plan_cache_put
from .deferred import DeferredLogVars, read_back_later  # noqa: F401
from .ops import stream_ptr
from .plan import Plan
from .registry import DETECTORS, build_backbone, build_head, build_neck
from .yolocsp_head import collect_results, final_counts, set_scale_factors


def bbox2result(bboxes, labels, num_classes):
    """core/bbox/transforms.py:99-113."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    if isinstance(bboxes, torch.Tensor):
        bboxes = bboxes.detach().cpu().numpy()
        labels = labels.detach().cpu().numpy()
    return [bboxes[labels == i, :] for i in range(num_classes)]


@DETECTORS.register_module()
class SingleStageDetector(HipModule):

    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None):
        super().__init__(init_cfg)
        if pretrained is not None:
            backbone = dict(backbone, pretrained=pretrained)
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        bbox_head = dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.fp16_enabled = False
        self._engines = {}

    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None

    # ---- plan ------------------------------------------------------------------------------
    def emit_feat(self, plan, x):
        feats = self.backbone.emit(plan, x)
        if self.with_neck:
            feats = self.neck.emit(plan, feats)
        return feats

    def emit(self, plan, x):
        """forward_dummy graph: image -> NHWC pred maps."""
        return self.bbox_head.emit(plan, self.emit_feat(plan, x))

    def compile(self, batch, height, width, device='cuda', rescale=True, graph=False, autotune=False, dtype=None):
        """Build (and cache) the end-to-end inference plan for one input geometry.
        graph=True records the launch list into a hipGraph (one replay per call; the
        reference's batch-1 protocol is otherwise bound by ~124 host launches);
        autotune=True times the candidate conv tiles per layer first; dtype: torch.float32 (default,
        the parity dtype), torch.float16 or torch.bfloat16 (``wrap_fp16_model`` sets the default), or
        torch.float8_e4m3fn (needs ``calibrate.calibrate_fp8`` first)."""
        dtype = dtype or getattr(self, 'compute_dtype', torch.float32)
        fp8 = dtype == torch.float8_e4m3fn
        if fp8 and getattr(self, 'fp8_amax', None) is None:
            raise RuntimeError('an fp8 plan needs activation scales: run calibrate.calibrate_fp8(detector, imgs) first')
        key = (batch, height, width, str(device), bool(rescale), bool(graph), self._param_version(), dtype,
               getattr(self, 'fp8_version', 0) if fp8 else 0)
        eng = plan_cache_get(self._engines, key)
        if eng is None:
            plan = self.build_plan(batch, height, width, device, rescale, dtype)
            if autotune and torch.device(device).type == 'cuda':
                plan.inputs[0]['src'] = torch.zeros((batch, 3, height, width), dtype=torch.float32, device=device)
                plan._launch_all(stream_ptr())
                plan.autotune()
            if graph:
                plan.capture()
            eng = plan
            plan_cache_put(self._engines, key, eng, 6)
        return eng

    def build_plan(self, batch, height, width, device, rescale, dtype):
        """The finalized (not captured) end-to-end plan of ``compile``."""
        plan = Plan(device, dtype, fp8_amax=getattr(self, 'fp8_amax', None) if dtype == torch.float8_e4m3fn else None)
        x = self._add_image(plan, batch, height, width, 'img')
        preds = self.emit(plan, x)
        self.bbox_head.emit_postprocess(plan, preds, rescale=rescale)
        plan.pred_views = preds
        return plan.finalize()

    def _add_image(self, plan, batch, height, width, name):
        # 16-bit plans keep the image fp32 when the backbone starts with the 3x3 stem (its own
        # fp32 kernel, 16-bit output); otherwise the image is converted like any other tensor
        conv0 = next((m for m in self.backbone.modules() if isinstance(m, torch.nn.Conv2d)), None)
        stem32 = (plan.h16 and isinstance(conv0, torch.nn.Conv2d) and conv0.kernel_size == (3, 3)
                  and conv0.stride == (1, 1) and conv0.padding == (1, 1) and conv0.in_channels == 3
                  and conv0.out_channels <= 64 and conv0.out_channels % 8 == 0)
        x = plan.add_input_nchw(batch, 3, height, width, name=name, dtype=torch.float32 if stem32 else None)
        plan.hint_single_consumer(x)             # the image feeds the backbone's first conv and nothing else
        return x

    # ---- test-time augmentation ----------------------------------------------------------------
    def compile_tta(self, batch, geometries, flips, device='cuda', graph=False, dtype=None):
        """Build (and cache) the TTA plan of ``aug_test``: ``geometries[a]`` the padded (H, W) of augmentation a's
        batch, ``flips[a]`` its YV4_FLIP_* code.  Augmentations of one geometry (an image and its flips) run the
        network as ONE batch of ``batch * len(group)`` rows; each distinct geometry gets its own network pass.  Then
        decode, slot tables, one merge and the NMS (``tta.emit_tta_post``), all on one stream: ``graph=True`` captures
        the whole plan into one hipGraph.  dtype: torch.float32 (default), torch.float16 or torch.bfloat16."""
        dtype = dtype or getattr(self, 'compute_dtype', torch.float32)
        if dtype == torch.float8_e4m3fn:
            raise NotImplementedError('fp8 TTA plans are not built')
        geometries = tuple(tuple(int(v) for v in g) for g in geometries)
        flips = tuple(int(f) for f in flips)
        if len(geometries) != len(flips) or len(flips) < 2:
            raise ValueError('a TTA plan takes one geometry and one flip code per augmentation, two or more of them')
        key = ('tta', batch, geometries, flips, str(device), bool(graph), self._param_version(), dtype)
        eng = plan_cache_get(self._engines, key)
        if eng is None:
            from .tta import emit_tta_post
            plan = Plan(device, dtype)
            groups = [[a for a, g in enumerate(geometries) if g == geo] for geo in dict.fromkeys(geometries)]
            gviews = []
            for gi, augs in enumerate(groups):
                H, W = geometries[augs[0]]
                x = self._add_image(plan, batch * len(augs), H, W, f'img{gi}')
                gviews.append((list(self.emit(plan, x)), augs))
            emit_tta_post(plan, self.bbox_head, gviews, flips, batch)
            plan.tta_groups = groups
            plan.pred_views = [v for v, _ in gviews]
            plan.finalize()
            if graph:
                plan.capture()
            eng = plan
            plan_cache_put(self._engines, key, eng, 6)
        return eng

    def aug_test(self, imgs, img_metas, rescale=False):
        """single_stage.py:114-137 with the merge of dense_test_mixins.py:38-100: ``imgs[a]`` the (N, 3, H, W) batch
        of augmentation a, ``img_metas[a]`` its N metas.  Returns one per-class list per image.  The reference runs
        a batch of one image; N > 1 is an extension (image n gets the result of its batch-1 run, bit for bit)."""
        self._check_eval()
        if not hasattr(self.bbox_head, 'aug_test_preds'):
            raise NotImplementedError('aug_test (TTA) is not built')
        from .tta import collect_tta, flip_code, set_tta_metas
        if len(imgs) != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        N = imgs[0].shape[0]
        if any(t.shape[0] != N for t in imgs) or any(len(m) != N for m in img_metas):
            raise ValueError('every augmentation must hold the same images')
        geos = tuple((t.shape[2], t.shape[3]) for t in imgs)
        flips = tuple(flip_code(m[0]) for m in img_metas)
        plan = self.compile_tta(N, geos, flips, device=imgs[0].device, graph=True)
        set_tta_metas(plan.post, img_metas)
        plan.run(*[torch.cat([imgs[a] for a in augs]) if len(augs) > 1 else imgs[augs[0]] for augs in plan.tta_groups])
        return collect_tta(plan.post, img_metas, rescale, self.bbox_head.num_classes)

    # ---- reference API ------------------------------------------------------------------------
    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def forward_dummy(self, img):
        return self.bbox_head(self.extract_feat(img))

    def show_results(self, imgs, results, out_files=None, score_thr=0.3, bbox_color=(72, 101, 241),
                     text_color=(72, 101, 241), mask_color=None, thickness=2, font_size=13):
        """The batched form behind ``show_result``: one decode of the file names among ``imgs``, one draw launch, and with
        ``out_files`` one encode (``imwrite``'s batch).  Returns the drawn (h, w, 3) device tensors, or ``out_files``."""
        from . import image_io
        from .draw import draw_boxes_into
        if len(imgs) != len(results) or (out_files is not None and len(out_files) != len(imgs)):
            raise ValueError(f'show_results: {len(imgs)} images, {len(results)} results'
                             + ('' if out_files is None else f' and {len(out_files)} output files'))
        if mask_color is not None:
            raise NotImplementedError('show_result(mask_color=...): masks are not built')
        if out_files is not None:
            image_io.check_jpeg_paths(out_files, 'show_result')
        if not imgs:
            return []
        device = next(self.parameters()).device
        dets, labels = [], []
        for res in results:
            if isinstance(res, tuple) and len(res) == 2 and isinstance(res[0], torch.Tensor):
                d, lab = res                                   # (dets, labels) device tensors
            elif isinstance(res, tuple):
                raise NotImplementedError('show_result: a (bbox, segm) result carries masks, which are not built')
            else:                                              # the per-class list (base.py:296-304)
                d = np.concatenate([np.asarray(r, np.float32).reshape(-1, 5) for r in res], 0) if len(res) else \
                    np.zeros((0, 5), np.float32)
                lab = np.concatenate([np.full(np.asarray(r).reshape(-1, 5).shape[0], k, np.int64)
                                      for k, r in enumerate(res)]) if len(res) else np.zeros(0, np.int64)
                d, lab = torch.from_numpy(d), torch.from_numpy(lab)
            dets.append(d.to(device, torch.float32).reshape(-1, 5))
            labels.append(lab.to(device).reshape(-1))
        classes = getattr(self, 'CLASSES', None)
        if classes is None:
            classes = [f'class {k}' for k in range(self.bbox_head.num_classes)]
        # every picture into one flat buffer: the files of the call are one decode batch, arrays and tensors are copied
        imgs = list(imgs)
        names = [k for k, a in enumerate(imgs) if isinstance(a, (str, os.PathLike))]
        if names:
            for k, a in zip(names, image_io.imread([imgs[k] for k in names], device=device)):
                imgs[k] = a
        offs, end = [], 0
        for k, a in enumerate(imgs):
            if isinstance(a, np.ndarray):
                imgs[k] = a = torch.from_numpy(np.ascontiguousarray(a))
            if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
                raise ValueError(f'show_result: image {k} is not a file name or a (h, w, 3) uint8 array or tensor')
            offs.append(end)
            end += (a.numel() + 255) // 256 * 256
        flat = torch.empty(end, dtype=torch.uint8, device=device)
        views = [flat[o:o + a.numel()].view(a.shape) for o, a in zip(offs, imgs)]
        for v, a in zip(views, imgs):
            v.copy_(a, non_blocking=True)
        places = [(a.shape[0], a.shape[1], o, 3 * a.shape[1]) for o, a in zip(offs, imgs)]
        draw_boxes_into(flat, places, dets, labels, list(classes), score_thr=score_thr, bbox_color=bbox_color,
                        text_color=text_color, thickness=thickness, font_size=font_size)
        if out_files is None:
            return views
        files = image_io.encode_into(flat, [(tuple(a.shape), o, 3 * a.shape[1]) for o, a in zip(offs, imgs)])
        image_io._write_files(files, list(out_files), True)
        return list(out_files)

    def show_result(self, img, result, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241), mask_color=None,
                    thickness=2, font_size=13, win_name='', show=False, wait_time=0, out_file=None):
        """``BaseDetector.show_result`` (``mmdet/models/detectors/base.py:256-341``) on the GPU.  ``img``: a file name
        (a baseline JPEG, decoded on the device), a (h, w, 3) BGR uint8 array or a device tensor; ``result``: the
        per-class list ``simple_test`` returns for one image, or ``(dets (k, 5), labels (k,))`` device tensors.  Boxes
        with ``score > score_thr`` are drawn with their class name (``self.CLASSES``, else ``class {label}``) and score
        by the package's own rule (``draw.py``: a 5x7 bitmap font, not matplotlib's rendering -- parity with the
        reference's picture is not claimed).  Returns the drawn device tensor, or with ``out_file`` writes it as a JPEG
        (``imwrite``'s defaults: quality 95, 4:2:0).  There is no display: ``show=True`` raises, and so do a result
        with masks and a ``mask_color``."""
        if show:
            raise NotImplementedError('show_result(show=True): there is no display window; pass out_file=')
        out = self.show_results([img], [result], None if out_file is None else [out_file], score_thr=score_thr,
                                bbox_color=bbox_color, text_color=text_color, mask_color=mask_color, thickness=thickness,
                                font_size=font_size)
        return None if out_file is not None else out[0]

    def simple_test(self, img, img_metas, rescale=False, results=None, img_index=None):
        """``results``: a ``results.DeviceResults``.  The batch is then appended to it on the device, at the dataset
        positions ``img_index`` (default: the table's next N), and the table is returned: only the (N,) counts are
        read back, which decide the split path as they do for the list form."""
        self._check_eval()
        N, _, H, W = img.shape
        plan = self.compile(N, H, W, device=img.device, rescale=rescale, graph=True)
        set_scale_factors(plan.post, img_metas, rescale)
        plan.run(img)
        if results is not None:
            results.append(plan.post, img_index, counts=final_counts(plan.post))
            return results
        bbox_list = collect_results(plan.post, with_nms=True, head=self.bbox_head)
        return [bbox2result(d, l, self.bbox_head.num_classes) for d, l in bbox_list]

    def _check_eval(self):
        if self.training:
            raise NotImplementedError('inference entry points need .eval(): they replay launch plans with folded BatchNorm; '
                                      'a module in .train() mode runs the autograd path (forward_train / train_step)')

    def forward_test(self, imgs, img_metas, **kwargs):
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        if len(imgs) != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        if len(imgs) == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        # detectors/base.py:147-150
        assert imgs[0].size(0) == 1, 'aug test does not support ' \
                                     'inference with batch size ' \
                                     f'{imgs[0].size(0)}'
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """single_stage.py:51-79: features through the HIP training ops, then the head's losses."""
        x = self.extract_feat(img)
        return self.bbox_head.forward_train(x, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore)

    def _parse_losses(self, losses):
        """detectors/base.py:171-204: total = sum of the entries whose key contains 'loss'; every log variable is the
        mean over ranks, returned as a python float.  The reference issues one all-reduce and one ``.item()`` (a host
        sync) PER log variable (base.py:197-202); here the variables are stacked on the device, exchanged by ONE
        all-reduce and read back by ONE device-to-host copy -- same values, one sync per step, taken when a value is
        first read (``DeferredLogVars``)."""
        if getattr(losses, 'total', None) is not None and not getattr(losses, 'built', True):
            # the fused head's loss matrix (yolocsp_head.FusedLosses): the same sums from the matrix itself
            m = losses.weighted.detach()
            cols = m.sum(0)
            names = (['loss_cls'] if losses.with_cls else []) + ['loss_conf', 'loss_bbox', 'num_gts', 'loss']
            stacked = torch.cat([cols if losses.with_cls else cols[1:], losses.num_gts.detach().float().reshape(1),
                                 losses.total.detach().reshape(1)])
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(stacked.div_(dist.get_world_size()))
            if stacked.is_cuda:
                return losses.total, read_back_later(stacked, names)
            return losses.total, OrderedDict(zip(names, stacked.tolist()))
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError(f'{name} is not a tensor or list of tensors')
        loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        log_vars['loss'] = loss
        stacked = torch.stack([v.detach().float().reshape(()) for v in log_vars.values()])
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(stacked.div_(dist.get_world_size()))
        if stacked.is_cuda:
            # stream-ordered copy into pinned memory; the host waits for it when a value is first read (see
            # DeferredLogVars) -- normally after the backward pass has been queued
            return loss, read_back_later(stacked, list(log_vars))
        for name, value in zip(list(log_vars), stacked.tolist()):
            log_vars[name] = value
        return loss, log_vars

    def train_step(self, data, optimizer):
        """detectors/base.py:206-239."""
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))
