"""The three training hooks of the YOLOv4 recipe, registered under the reference's names, plus
the small runner protocol they are driven through.

Reference surface mirrored here (``HOOKS.register_module``; constructor arguments, the stage
methods that do work, and the arithmetic of every schedule):
  * ``Fp16GradAccumulateOptimizerHook`` -- ``mmdet/core/custom_hooks/accum_optim_hooks.py:9-60``
    (torch >= 1.6 branch; base class ``mmcv.runner.Fp16OptimizerHook`` is third-party, its
    GradScaler behaviour is restated: ``loss_scale='dynamic'`` -> scale 2**16, x2 every 2000
    clean steps, x0.5 and skip on overflow; a float -> static scale)
  * ``StateEMAHook`` -- ``mmdet/core/custom_hooks/ema_hooks.py:8-126``
  * ``DetailedLinearWarmUpHook`` -- ``mmdet/core/custom_hooks/warmup_hooks.py:5-59``
Wired in configs as ``optimizer_config`` / ``custom_hooks``
(``configs/yolov4/yolov4l_coco_mosaic.py:117-147``).

What differs is where the work runs: un-scale + clip + SGD step + loss-scale update are four
kernel launches over the flat gradient arena with no host synchronisation, the EMA is one launch
over the whole state arena (``csrc/optim.hip``, ``flat_state.py``); the reference walks ~430
parameter groups and 658 state entries in Python for the same arithmetic.

The schedule arithmetic is exposed as pure functions (``warmup_factor``, ``ema_momentum``,
``accumulation_steps``) so it is testable without a device.
"""
import math
import os
import time
import warnings
from collections import OrderedDict

import torch

from . import _lib
from ._lib import check
from .flat_state import FlatState
from .ops import stream_ptr
from .registry import HOOKS, RUNNERS

# ---- pure schedule arithmetic ------------------------------------------------------------------


def warmup_factor(cur_iter, warmup_iters, ratio):
    """warmup_hooks.py:43-58: ``prog + (1 - prog) * ratio`` with ``prog = iter / warmup_iters``
    (multiplies the base lr / momentum while ``iter <= warmup_iters``)."""
    prog = cur_iter / warmup_iters
    return prog + (1 - prog) * ratio


def ema_momentum(momentum, cur_iter, warm_up, interval):
    """ema_hooks.py:90-91."""
    return momentum * (1 - math.exp(-cur_iter / (warm_up * interval)))


def accumulation_steps(nominal_batch_size, samples_per_gpu, world_size):
    """accum_optim_hooks.py:33-34 / ema_hooks.py:112-113."""
    return math.ceil(nominal_batch_size / (samples_per_gpu * world_size))


def _unwrap(model):
    return model.module if hasattr(model, 'module') and isinstance(model.module, torch.nn.Module) else model


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


# ---- hook base + priorities (mmcv.runner.Hook / Priority) -----------------------------------------
PRIORITY = dict(HIGHEST=0, VERY_HIGH=10, HIGH=30, ABOVE_NORMAL=40, NORMAL=50, BELOW_NORMAL=60, LOW=70,
                VERY_LOW=90, LOWEST=100)


class Hook:
    stages = ('before_run', 'before_train_epoch', 'before_train_iter', 'after_train_iter', 'after_train_epoch',
              'after_run')

    def before_run(self, runner):
        pass

    def after_run(self, runner):
        pass

    def before_epoch(self, runner):
        pass

    def after_epoch(self, runner):
        pass

    def before_iter(self, runner):
        pass

    def after_iter(self, runner):
        pass

    def before_train_epoch(self, runner):
        self.before_epoch(runner)

    def after_train_epoch(self, runner):
        self.after_epoch(runner)

    def before_train_iter(self, runner):
        self.before_iter(runner)

    def after_train_iter(self, runner):
        self.after_iter(runner)

    # mmcv.runner.Hook's schedule tests
    def every_n_epochs(self, runner, n):
        return (runner.epoch + 1) % n == 0 if n > 0 else False

    def every_n_iters(self, runner, n):
        return (runner.iter + 1) % n == 0 if n > 0 else False


@HOOKS.register_module()
class DistSamplerSeedHook(Hook):
    """mmcv's ``DistSamplerSeedHook`` (``mmcv/runner/hooks/sampler_seed.py``): the loader's sampler learns the epoch
    before it starts, so that a resumed run shuffles as the uninterrupted one does."""

    def before_epoch(self, runner):
        sampler = getattr(runner.data_loader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(runner.epoch)


# ---- a22 ---------------------------------------------------------------------------------------------
@HOOKS.register_module()
class Fp16GradAccumulateOptimizerHook(Hook):
    """Backward + (every ``accumulation`` iterations) un-scale, clip, step, loss-scale update.

    Gradients of the accumulated iterations are **summed**, not averaged (the reference's
    torch >= 1.6 branch never divides by ``accumulation``, accum_optim_hooks.py:37-60).
    The arena keeps the *scaled* gradients: un-scaling and clipping are folded into the one
    multiplier the step kernel applies (``ctrl[0]``), so ``p.grad`` is not rewritten in place."""

    def __init__(self, grad_clip=None, coalesce=True, bucket_size_mb=-1, loss_scale=512., distributed=True,
                 nominal_batch_size=None, accumulation=None, compute_dtype=None, grad_exchange=None):
        # compute_dtype: None leaves the model as it is (fp32 unless wrap_fp16_model was applied);
        # 'fp16' / 'bf16' (or the torch dtypes) make before_run wrap the model like the reference's
        # Fp16OptimizerHook.before_run does (mmcv wrap_fp16_model): 16-bit activations, fp32 master weights
        self.compute_dtype = {None: None, 'fp16': torch.float16, 'bf16': torch.bfloat16, 'fp32': torch.float32,
                              torch.float16: torch.float16, torch.bfloat16: torch.bfloat16,
                              torch.float32: torch.float32}[compute_dtype]
        # grad_exchange: None (YV4_GRAD_EXCHANGE or 'allreduce') | 'allreduce' | 'direct' | 'direct_bf16', see
        # dist.GradReducer
        self.grad_exchange = grad_exchange
        self.grad_clip = grad_clip
        self.coalesce = coalesce
        self.bucket_size_mb = bucket_size_mb
        self.distributed = distributed
        self.accumulation = 1
        self.nominal_batch_size = None
        if accumulation is not None:
            assert isinstance(accumulation, int) and accumulation > 0
            self.accumulation = accumulation
        elif nominal_batch_size is not None:
            self.accumulation = None
            self.nominal_batch_size = nominal_batch_size
        if grad_clip is not None:
            if grad_clip.get('norm_type', 2) != 2:
                raise NotImplementedError('grad_clip: only the L2 norm (norm_type=2) is implemented')
        # GradScaler(init_scale=2**16, growth_factor=2, backoff_factor=.5, growth_interval=2000)
        self.scaler_cfg = dict(init_scale=65536., growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
        self.dynamic = True
        if loss_scale == 'dynamic':
            pass
        elif isinstance(loss_scale, (int, float)):
            self.scaler_cfg['init_scale'] = float(loss_scale)
            self.dynamic = False
        elif isinstance(loss_scale, dict):
            # torch.cuda.amp.GradScaler's keys, or mmcv's legacy LossScaler spelling that the reference's own
            # yolov5_ddp configs use (configs/yolov5_ddp/*:21-23: init_scale, mode, scale_factor, scale_window)
            ls = dict(loss_scale)
            mode = ls.pop('mode', 'dynamic')
            if 'scale_factor' in ls:
                f = float(ls.pop('scale_factor'))
                ls.setdefault('growth_factor', f)
                ls.setdefault('backoff_factor', 1.0 / f)
            if 'scale_window' in ls:
                ls.setdefault('growth_interval', int(ls.pop('scale_window')))
            unknown = set(ls) - set(self.scaler_cfg)
            if unknown:
                raise TypeError(f'loss_scale: unexpected keys {sorted(unknown)}')
            self.scaler_cfg.update(ls)
            self.dynamic = mode == 'dynamic' 
        else:
            raise ValueError(f'loss_scale must be of type float, dict, or "dynamic", got {loss_scale}')
        self.scale_state = None
        self.ctrl = None
        self.reducer = None

    # device state is created lazily on the model's device
    def _ensure_state(self, runner):
        if self.scale_state is None:
            flat = FlatState.of(_unwrap(runner.model))
            self.flat = flat
            self.scale_state = torch.tensor([self.scaler_cfg['init_scale'], 0.], dtype=torch.float32,
                                            device=flat.device)
            self.ctrl = torch.zeros(4, dtype=torch.float32, device=flat.device)
            # 2 sums + one slot per workgroup of the deterministic mode's gradient norm (include/yv4.h)
            self.work = torch.zeros(2 + _lib.GRAD_PREPARE_MAX_WG, dtype=torch.float64, device=flat.device)
            if self.distributed and (_world_size() > 1 or os.environ.get('YV4_REDUCER_AT_WORLD1') == '1'):
                # (YV4_REDUCER_AT_WORLD1=1: build the reducer with one rank too -- tools/train_bench.py --overlap-report
                # measures where in backward each bucket becomes exchangeable; nothing is exchanged)
                from .dist import GradReducer
                mb = self.bucket_size_mb if self.bucket_size_mb and self.bucket_size_mb > 0 else 32
                self.reducer = GradReducer(flat, bucket_mb=mb, mode=self.grad_exchange)

    def before_run(self, runner):
        self._ensure_state(runner)
        if self.compute_dtype is not None:
            from .bricks import wrap_fp16_model
            wrap_fp16_model(_unwrap(runner.model), self.compute_dtype)
        meta = getattr(runner, 'meta', None)
        if meta and 'fp16' in meta and 'loss_scaler' in meta['fp16']:
            self.load_loss_scaler_state_dict(meta['fp16']['loss_scaler'])

    def before_train_epoch(self, runner):
        if self.accumulation is None:
            assert self.nominal_batch_size is not None
            samples_per_gpu = runner.data_loader.sampler.samples_per_gpu
            self.accumulation = accumulation_steps(self.nominal_batch_size, samples_per_gpu, _world_size())

    def loss_scale(self):
        """Current scale (synchronises)."""
        return float(self.scale_state[0].item())

    def after_train_iter(self, runner):
        self._ensure_state(runner)
        model = _unwrap(runner.model)
        first = runner.iter % self.accumulation == 0
        last = (runner.iter + 1) % self.accumulation == 0
        if first:
            # the reference zeroes through the model and through the optimizer; with both on the same gradient arena
            # one memset (and one walk over the parameters) does it
            fs = getattr(model, '_flat_state', None)
            if fs is not None and fs is getattr(runner.optimizer, 'flat', None):
                fs.zero_grad()
            else:
                model.zero_grad()
                runner.optimizer.zero_grad()
        if self.reducer is not None and last:
            self.reducer.arm()
        (runner.outputs['loss'] * self.scale_state[0]).backward()
        from .train_ops import join_side_streams
        join_side_streams()          # (the end-of-backward callback does it; it is dropped when a backward raises)
        if not last:
            return
        if self.reducer is not None:
            self.reducer.finish()
        max_norm = float(self.grad_clip['max_norm']) if self.grad_clip is not None else 0.
        L = _lib.lib()
        f = self.flat
        check(L.yv4_grad_prepare(f.grads.data_ptr(), f.n_param, self.scale_state.data_ptr(), max_norm,
                                 self.work.data_ptr(), self.ctrl.data_ptr(), stream_ptr()), 'yv4_grad_prepare')
        log = getattr(runner, 'log_buffer', None)
        if self.grad_clip is not None and log is not None:
            # the reference's float(grad_norm) drains the device here, between the backward pass and the update; the
            # copy is queued instead and waited for when the log buffer is read
            from .deferred import read_back_later
            log.update(read_back_later(self.ctrl, ['grad_norm', 'grad_scale'], lambda c: [c[1], 1.0 / c[3]]),
                       runner.outputs.get('num_samples', 1))
        runner.optimizer.step(ctrl=self.ctrl)
        if self.dynamic:
            check(L.yv4_loss_scale_update(self.scale_state.data_ptr(), self.ctrl.data_ptr(),
                                          float(self.scaler_cfg['growth_factor']),
                                          float(self.scaler_cfg['backoff_factor']),
                                          int(self.scaler_cfg['growth_interval']), stream_ptr()),
                  'yv4_loss_scale_update')

    # ---- checkpoint state (mmcv Fp16OptimizerHook keeps GradScaler.state_dict() in runner.meta['fp16']) -------
    def loss_scaler_state_dict(self):
        """``torch.cuda.amp.GradScaler.state_dict()`` layout: what the reference's base hook stores in
        ``runner.meta['fp16']['loss_scaler']`` and ``GradScaler.load_state_dict`` requires (one device read)."""
        if self.scale_state is None:
            scale, tracker = float(self.scaler_cfg['init_scale']), 0
        else:
            scale, tracker = self.scale_state.tolist()
        return dict(scale=float(scale), growth_factor=float(self.scaler_cfg['growth_factor']),
                    backoff_factor=float(self.scaler_cfg['backoff_factor']),
                    growth_interval=int(self.scaler_cfg['growth_interval']), _growth_tracker=int(tracker))

    def load_loss_scaler_state_dict(self, sd):
        for k in ('growth_factor', 'backoff_factor', 'growth_interval'):
            if k in sd:
                self.scaler_cfg[k] = sd[k]
        self.scale_state[0] = float(sd['scale'])
        self.scale_state[1] = float(sd.get('_growth_tracker', 0))

    def sync_meta(self, runner):
        """Write the plain loss-scaler dict into ``runner.meta``.  The reference does this after every iteration
        (a device read per step); here it happens when the state is wanted: before a checkpoint is written
        (``Runner.save_checkpoint``), at the end of every epoch and at the end of the run."""
        meta = getattr(runner, 'meta', None)
        if isinstance(meta, dict) and self.scale_state is not None:
            meta.setdefault('fp16', {})['loss_scaler'] = self.loss_scaler_state_dict()

    def after_train_epoch(self, runner):
        self.sync_meta(runner)

    def after_run(self, runner):
        self.sync_meta(runner)


@HOOKS.register_module()
class Fp16OptimizerHook(Fp16GradAccumulateOptimizerHook):
    """mmcv's ``Fp16OptimizerHook`` (third party; the base class of the fork's accumulate hook,
    accum_optim_hooks.py:9): what ``mmdet/apis/train.py:115-118`` builds from ``optimizer_config`` + the top-level
    ``fp16`` block of configs/yolov5_ddp/*.  One optimizer step per iteration = the accumulate hook with a window of 1."""

    def __init__(self, grad_clip=None, coalesce=True, bucket_size_mb=-1, loss_scale=512., distributed=True, **kw):
        super().__init__(grad_clip=grad_clip, coalesce=coalesce, bucket_size_mb=bucket_size_mb, loss_scale=loss_scale,
                         distributed=distributed, accumulation=1, **kw)


@HOOKS.register_module()
class OptimizerHook(Fp16GradAccumulateOptimizerHook):
    """mmcv's plain ``OptimizerHook(grad_clip)`` (``apis/train.py:119-120``): no loss scaling -- the same fused
    clip + step launches with a static scale of 1."""

    def __init__(self, grad_clip=None, **kw):
        kw.setdefault('distributed', True)
        super().__init__(grad_clip=grad_clip, loss_scale=1.0, accumulation=1, **kw)


def build_optimizer_hook(cfg, distributed=True):
    """``mmdet/apis/train.py:115-122``: the optimizer hook a config asks for.  ``cfg`` needs ``optimizer_config`` and
    optionally ``fp16`` (mapping or Config)."""
    get = cfg.get if hasattr(cfg, 'get') else (lambda k, d=None: getattr(cfg, k, d))
    oc = dict(get('optimizer_config') or {})
    fp16 = get('fp16', None)
    if fp16 is not None:
        return Fp16OptimizerHook(**oc, **dict(fp16), distributed=distributed)
    if 'type' not in oc:
        return OptimizerHook(**oc)
    from .registry import build_from_cfg
    return build_from_cfg(oc, HOOKS)


# ---- a23 ---------------------------------------------------------------------------------------------
@HOOKS.register_module()
class StateEMAHook(Hook):
    """EMA of every state-dict entry, kept as model buffers ``ema_<name with '.' -> '_'>`` so that
    checkpoints carry them (ema_hooks.py:52-64).  The buffers are views of one EMA arena laid out
    like the model's FlatState; integer entries (``num_batches_tracked``) are tracked as floats
    (what the reference's buffers become after the first swap, ema_hooks.py:118-126)."""

    def __init__(self, momentum=0.9999, interval=None, nominal_batch_size=None, warm_up=2000, resume_from=None):
        self.interval = 1
        self.nominal_batch_size = None
        self.warm_up = warm_up
        if interval is not None:
            assert isinstance(interval, int) and interval > 0
            self.interval = interval
        elif nominal_batch_size is not None:
            self.interval = None
            self.nominal_batch_size = nominal_batch_size
        assert momentum > 0 and momentum < 1
        self.momentum = momentum
        self.checkpoint = resume_from

    def before_run(self, runner):
        model = _unwrap(runner.model)
        flat = FlatState.of(model)
        self.flat = flat
        self.ema = flat.values.clone()
        self.ema_ints = flat.ints.to(torch.float32)
        from .flat_state import _view_as_param
        views = {}
        for seg in flat.param_segments + flat.buffer_segments:
            views[seg.name] = _view_as_param(self.ema, seg)
        for seg in flat.int_segments:
            views[seg.name] = self.ema_ints[seg.offset:seg.offset + seg.numel].view(seg.shape)
        # registered in state_dict order, like the reference (checkpoint key order)
        self.param_ema_mapping = {}
        for name in list(model.state_dict().keys()):
            if name not in views:
                raise RuntimeError(f'StateEMAHook: state entry {name} is not part of the FlatState')
            bname = f"ema_{name.replace('.', '_')}"
            self.param_ema_mapping[name] = bname
            model.register_buffer(bname, views[name])
        # ema_hooks.py:66-74: resume AFTER the ema_ buffers exist, from the hook's own argument or from the
        # ``resume_from`` of the config text the training script stored in ``runner.meta['config']``
        checkpoint = self.checkpoint
        if checkpoint is None:
            cfg_text = (getattr(runner, 'meta', None) or {}).get('config')
            if cfg_text is not None:
                cfg_dict = dict()
                exec(cfg_text, cfg_dict)
                checkpoint = cfg_dict.get('resume_from')
        if checkpoint is not None:
            runner.resume(checkpoint)

    def current_momentum(self, cur_iter):
        return ema_momentum(self.momentum, cur_iter, self.warm_up, self.interval)

    def after_train_iter(self, runner):
        if (runner.iter + 1) % self.interval != 0:
            return
        m = self.current_momentum(runner.iter)
        f = self.flat
        check(_lib.lib().yv4_ema_update(self.ema.data_ptr(), f.values.data_ptr(), f.n_state, float(m),
                                        stream_ptr()), 'yv4_ema_update')
        if f.n_int:
            self.ema_ints.copy_(f.ints)

    def after_train_epoch(self, runner):
        self._swap_ema_parameters(runner)

    def before_train_epoch(self, runner):
        if self.interval is None:
            assert self.nominal_batch_size is not None
            samples_per_gpu = runner.data_loader.sampler.samples_per_gpu
            self.interval = accumulation_steps(self.nominal_batch_size, samples_per_gpu, _world_size())
        self._swap_ema_parameters(runner)

    def _swap_ema_parameters(self, runner):
        f = self.flat
        with torch.no_grad():
            tmp = f.values.clone()
            f.values.copy_(self.ema)
            self.ema.copy_(tmp)
            if f.n_int:
                tmp_i = f.ints.to(torch.float32)
                f.ints.copy_(self.ema_ints.to(torch.int64))
                self.ema_ints.copy_(tmp_i)
        f.bump_versions()


# ---- a24 ---------------------------------------------------------------------------------------------
@HOOKS.register_module()
class DetailedLinearWarmUpHook(Hook):
    """Per-parameter linear warm-up: bias lr ``ratio_b -> 1``, weight lr ``ratio_w -> 1``,
    momentum ``ratio_m -> 1`` over ``warmup_iters`` iterations; needs one param group per
    parameter in ``named_parameters()`` order (warmup_hooks.py:24-40)."""

    def __init__(self, warmup_iters=10000, lr_weight_warmup_ratio=0., lr_bias_warmup_ratio=10.,
                 momentum_warmup_ratio=0.95):
        self.warmup_iters = warmup_iters
        self.lr_weight_warmup_ratio = lr_weight_warmup_ratio
        self.lr_bias_warmup_ratio = lr_bias_warmup_ratio
        self.momentum_warmup_ratio = momentum_warmup_ratio
        self.bias_base_lr = {}
        self.weight_base_lr = {}
        self.base_momentum = {}

    def before_run(self, runner):
        model = runner.model
        if len(runner.optimizer.param_groups) != len([*model.parameters()]):
            logger = getattr(runner, 'logger', None)
            if logger is not None:
                logger.warning('optimizer config does not support preheat because'
                               ' it is not using seperate param-group for each parameter')
            return
        # a checkpoint written by this package carries the bases (``sync_meta``): a run resumed inside the warm-up
        # window then warms up from them, not from the warmed values its optimizer state holds (the reference reads
        # the groups as they were saved, warmup_hooks.py:22-36, and so does this hook when the meta has no bases)
        saved = (getattr(runner, 'meta', None) or {}).get(self.META_KEY)
        n = len(runner.optimizer.param_groups)
        if not (isinstance(saved, dict) and len(saved.get('lr', ())) == n and len(saved.get('momentum', ())) == n):
            saved = None
        for group_ind, (name, param) in enumerate(model.named_parameters()):
            group = runner.optimizer.param_groups[group_ind]
            lr, momentum = (saved['lr'][group_ind], saved['momentum'][group_ind]) if saved else \
                (group['lr'], group['momentum'])
            self.base_momentum[group_ind] = momentum
            if name.endswith('.bias'):
                self.bias_base_lr[group_ind] = lr
            elif name.endswith('.weight'):
                self.weight_base_lr[group_ind] = lr
        self._bases = dict(lr=[{**self.bias_base_lr, **self.weight_base_lr}.get(i, g['lr'])
                               for i, g in enumerate(runner.optimizer.param_groups)],
                           momentum=[self.base_momentum[i] for i in range(n)])

    META_KEY = 'detailed_warmup_base'
    _bases = None

    def sync_meta(self, runner):
        """The base lr and momentum of every group into ``runner.meta`` (``Runner.save_checkpoint`` calls this): what a
        resumed run needs beyond the optimizer's state."""
        meta = getattr(runner, 'meta', None)
        if isinstance(meta, dict) and self._bases is not None:
            meta[self.META_KEY] = self._bases

    def before_train_iter(self, runner):
        if runner.iter <= self.warmup_iters:
            groups = runner.optimizer.param_groups
            fb = warmup_factor(runner.iter, self.warmup_iters, self.lr_bias_warmup_ratio)
            fw = warmup_factor(runner.iter, self.warmup_iters, self.lr_weight_warmup_ratio)
            fm = warmup_factor(runner.iter, self.warmup_iters, self.momentum_warmup_ratio)
            for group_ind, bias_base in self.bias_base_lr.items():
                groups[group_ind]['lr'] = fb * bias_base
            for group_ind, weight_base in self.weight_base_lr.items():
                groups[group_ind]['lr'] = fw * weight_base
            for group_ind, momentum_base in self.base_momentum.items():
                groups[group_ind]['momentum'] = fm * momentum_base


# ---- lr_config = dict(policy='CosineAnnealing', min_lr_ratio=0.2) ----------------------------------------
def warmup_lr(regular_lr, cur_iter, warmup, warmup_iters, warmup_ratio):
    """mmcv ``LrUpdaterHook.get_warmup_lr`` for one group: the lr of iteration ``cur_iter < warmup_iters``."""
    if warmup == 'constant':
        return regular_lr * warmup_ratio
    if warmup == 'linear':
        k = (1 - cur_iter / warmup_iters) * (1 - warmup_ratio)
        return regular_lr * (1 - k)
    k = warmup_ratio ** (1 - cur_iter / warmup_iters)          # 'exp'
    return regular_lr * k


class LrUpdaterHook(Hook):
    """mmcv's ``LrUpdaterHook`` (``mmcv/runner/hooks/lr_updater.py``, mmcv 1.3.2 .. 1.4.0; third-party, restated, parity
    unpinned): every group's ``initial_lr`` is its base; a subclass gives ``get_lr(runner, base_lr)``, the regular lr at
    ``runner.epoch`` (``by_epoch``) or ``runner.iter``; the optional warm-up replaces it during the first
    ``warmup_iters`` iterations (epochs with ``warmup_by_epoch``) by ``warmup_lr`` of it, and the regular lr comes back
    at iteration ``warmup_iters``.  With ``warmup=None`` the lr is written at the start of every epoch (``by_epoch``)
    or of every iteration, and nowhere else."""

    def __init__(self, by_epoch=True, warmup=None, warmup_iters=0, warmup_ratio=0.1, warmup_by_epoch=False):
        if warmup is not None:
            if warmup not in ('constant', 'linear', 'exp'):
                raise ValueError(f'"{warmup}" is not a supported type for warming up, valid types are "constant", '
                                 '"linear" and "exp"')
            assert warmup_iters > 0, '"warmup_iters" must be a positive integer'
            assert 0 < warmup_ratio <= 1.0, '"warmup_ratio" must be in range (0,1]'
        self.by_epoch, self.warmup, self.warmup_ratio = by_epoch, warmup, warmup_ratio
        self.warmup_by_epoch = warmup_by_epoch
        if warmup_by_epoch:
            self.warmup_epochs, self.warmup_iters = warmup_iters, None
        else:
            self.warmup_epochs, self.warmup_iters = None, warmup_iters
        self.base_lr = []
        self.regular_lr = []

    def get_lr(self, runner, base_lr):
        raise NotImplementedError

    def _set_lr(self, runner, lrs):
        for g, lr in zip(runner.optimizer.param_groups, lrs):
            g['lr'] = lr

    def get_regular_lr(self, runner):
        return [self.get_lr(runner, base) for base in self.base_lr]

    def get_warmup_lr(self, cur_iter):
        return [warmup_lr(lr, cur_iter, self.warmup, self.warmup_iters, self.warmup_ratio) for lr in self.regular_lr]

    def before_run(self, runner):
        for g in runner.optimizer.param_groups:
            g.setdefault('initial_lr', g['lr'])
        self.base_lr = [g['initial_lr'] for g in runner.optimizer.param_groups]

    def before_train_epoch(self, runner):
        if self.warmup_iters is None:
            self.warmup_iters = self.warmup_epochs * len(runner.data_loader)
        if not self.by_epoch:
            return
        self.regular_lr = self.get_regular_lr(runner)
        self._set_lr(runner, self.regular_lr)

    def before_train_iter(self, runner):
        cur_iter = runner.iter
        if not self.by_epoch:
            self.regular_lr = self.get_regular_lr(runner)
            if self.warmup is None or cur_iter >= self.warmup_iters:
                self._set_lr(runner, self.regular_lr)
            else:
                self._set_lr(runner, self.get_warmup_lr(cur_iter))
        elif self.warmup is None or cur_iter > self.warmup_iters:
            return
        elif cur_iter == self.warmup_iters:
            self._set_lr(runner, self.regular_lr)
        else:
            self._set_lr(runner, self.get_warmup_lr(cur_iter))


@HOOKS.register_module()
class StepLrUpdaterHook(LrUpdaterHook):
    """mmcv's ``StepLrUpdaterHook`` (``lr_config = dict(policy='step', step=[218, 246])`` of the YOLOv3 recipe,
    ``configs/yolo/yolov3_d53_mstrain-608_273e_coco.py``): ``base * gamma ** k``, ``k`` the number of ``step`` entries
    already reached (``progress // step`` for an int), not below ``min_lr``."""

    def __init__(self, step, gamma=0.1, min_lr=None, **kwargs):
        if isinstance(step, (list, tuple)):
            assert all(isinstance(s, int) and s > 0 for s in step), '"step" must be a list of positive integers'
            step = list(step)
        elif isinstance(step, int):
            assert step > 0
        else:
            raise TypeError('"step" must be a list or integer')
        self.step, self.gamma, self.min_lr = step, gamma, min_lr
        super().__init__(**kwargs)

    def get_lr(self, runner, base_lr):
        progress = runner.epoch if self.by_epoch else runner.iter
        if isinstance(self.step, int):
            exp = progress // self.step
        else:
            exp = len(self.step)
            for i, s in enumerate(self.step):
                if progress < s:
                    exp = i
                    break
        lr = base_lr * self.gamma ** exp
        if self.min_lr is not None:
            lr = max(lr, self.min_lr)
        return lr


@HOOKS.register_module()
class CosineAnnealingLrUpdaterHook(LrUpdaterHook):
    """mmcv's cosine annealing (third-party; restated): ``lr = min + 0.5 (base - min)(1 + cos(pi * epoch /
    max_epochs))`` per group from its ``initial_lr``, at the start of every epoch (of every iteration from ``iter /
    max_iters`` with ``by_epoch=False``).  The YOLOv4 recipe gives it no warm-up of its own and warms up through
    ``DetailedLinearWarmUpHook`` (``configs/yolov4/yolov4l_coco_mosaic.py:124-139``); the shared ``warmup`` options of
    ``LrUpdaterHook`` are accepted."""

    def __init__(self, min_lr=None, min_lr_ratio=None, **kwargs):
        assert (min_lr is None) ^ (min_lr_ratio is None)
        self.min_lr, self.min_lr_ratio = min_lr, min_lr_ratio
        super().__init__(**kwargs)

    @staticmethod
    def annealing_cos(start, end, factor):
        return end + 0.5 * (start - end) * (math.cos(math.pi * factor) + 1)

    def get_lr(self, runner, base_lr):
        if self.by_epoch:
            progress, max_progress = runner.epoch, runner.max_epochs
        else:
            progress, max_progress = runner.iter, runner.max_iters
        target = base_lr * self.min_lr_ratio if self.min_lr_ratio is not None else self.min_lr
        return self.annealing_cos(base_lr, target, progress / max_progress)


# ---- validation in training: mmdet/core/evaluation/eval_hooks.py, and the slice of mmcv's CheckpointHook it needs ----
@HOOKS.register_module()
class CheckpointHook(Hook):
    """The part of mmcv's ``CheckpointHook`` that ``save_best`` depends on: ``runner.save_checkpoint`` every ``interval``
    epochs (iterations with ``by_epoch=False``; ``interval=-1`` never), on rank 0 only, into ``out_dir`` (default
    ``runner.work_dir``), and the written file's path in ``runner.meta['hook_msgs']['last_ckpt']``.  Registered before
    the evaluation hook at the same priority it runs first, so the evaluation's ``best_ckpt`` is this epoch's file."""

    def __init__(self, interval=-1, by_epoch=True, save_optimizer=True, out_dir=None, **kwargs):
        self.interval, self.by_epoch, self.save_optimizer, self.out_dir = interval, by_epoch, save_optimizer, out_dir
        self.args = kwargs

    def _save(self, runner, filename_tmpl):
        if runner.rank != 0:
            return
        out_dir = self.out_dir or runner.work_dir
        if out_dir is None:
            raise ValueError('CheckpointHook needs out_dir= or a runner with a work_dir')
        path = runner.save_checkpoint(out_dir, filename_tmpl=filename_tmpl, save_optimizer=self.save_optimizer,
                                      **self.args)
        if runner.meta is not None:
            runner.meta.setdefault('hook_msgs', dict())['last_ckpt'] = path

    def after_train_epoch(self, runner):
        if self.by_epoch and self.every_n_epochs(runner, self.interval):
            self._save(runner, 'epoch_{}.pth')

    def after_train_iter(self, runner):
        if not self.by_epoch and self.every_n_iters(runner, self.interval):
            self._save(runner, f'iter_{runner.iter + 1}.pth')


def contiguous_runs(spans):
    """``[(offset, length), ...]`` -> the ``[lo, hi)`` ranges that cover them with one range per run of spans that
    touch (sorted by offset; a span that starts where the previous one ends extends it)."""
    runs = []
    for off, n in sorted(spans):
        if runs and runs[-1][1] == off:
            runs[-1][1] = off + n
        else:
            runs.append([off, off + n])
    return [tuple(r) for r in runs]


def bn_stat_runs(model, flat):
    """The arena ranges of ``running_mean`` / ``running_var`` of every tracked ``_BatchNorm`` of ``model``: what the
    reference's ``_broadcast_bn_buffer`` sends one tensor at a time (eval_hooks.py:247-259).  The arena pads every
    segment to 4 floats; the padding belongs to its segment's span.  ``ema_*`` buffers, integer buffers and parameters
    are not part of it."""
    from torch.nn.modules.batchnorm import _BatchNorm
    from .flat_state import _pad4
    wanted = set()
    for name, m in model.named_modules():
        if isinstance(m, _BatchNorm) and m.track_running_stats:
            wanted.update((f'{name}.running_mean' if name else 'running_mean', f'{name}.running_var' if name else 'running_var'))
    return contiguous_runs([(seg.offset, _pad4(seg.numel)) for seg in flat.buffer_segments if seg.name in wanted])


@HOOKS.register_module()
class EvalHook(Hook):
    """``EvalHook`` of ``mmdet/core/evaluation/eval_hooks.py:14-187``: run the test loop over ``dataloader`` when the
    schedule says so, score with ``dataloader.dataset.evaluate(results, logger=runner.logger, **eval_kwargs)``, put
    every metric into ``runner.log_buffer.output`` and, with ``save_best``, keep ``best_score`` / ``best_ckpt`` in
    ``runner.meta['hook_msgs']`` and the symlink ``best_<key>.pth`` in ``runner.work_dir``.

    Schedule: with ``start=None`` after every ``interval``-th epoch; otherwise never before epoch ``start`` (counted
    from 1), then every ``interval`` epochs from it (``start=3, interval=2``: 3, 5, 7); a run resumed at or beyond
    ``start`` evaluates once before its first epoch, if the same test admits it.  ``by_epoch=False`` counts iterations.

    Differences from the reference, both on purpose: ``dataloader`` is any iterable of test batches with a
    ``.dataset`` (the reference insists on ``torch.utils.data.DataLoader``; this package's loaders are generators over
    the fused input pipeline); and the result form.  ``flat=None`` takes the flat test loop -- the result table built
    and scored on the GPU (``results.DeviceResults``) -- when ``dataloader.dataset.accepts_flat`` is true and the list
    loop otherwise; ``flat=True`` / ``False`` decide it outright.  The hook puts the model back into the mode it found
    it in: with ``by_epoch=False`` the next training iteration follows directly."""

    rule_map = {'greater': lambda x, y: x > y, 'less': lambda x, y: x < y}
    init_value_map = {'greater': -math.inf, 'less': math.inf}
    greater_keys = ['mAP', 'AR']
    less_keys = ['loss']
    distributed = False              # DistEvalHook: evaluate and save on rank 0 only

    def __init__(self, dataloader, start=None, interval=1, by_epoch=True, save_best=None, rule=None, flat=None,
                 **eval_kwargs):
        if not hasattr(dataloader, 'dataset'):
            raise TypeError(f'dataloader must carry a .dataset to evaluate against, but got {type(dataloader)}')
        if not interval > 0:
            raise ValueError(f'interval must be positive, but got {interval}')
        if start is not None and start < 0:
            warnings.warn(f'The evaluation start epoch {start} is smaller than 0, use 0 instead', UserWarning)
            start = 0
        assert isinstance(save_best, str) or save_best is None
        self.dataloader, self.start, self.interval, self.by_epoch = dataloader, start, interval, by_epoch
        self.save_best = save_best
        self.flat = flat
        self.eval_kwargs = eval_kwargs
        self.initial_epoch_flag = True
        if self.save_best is not None:
            self._init_rule(rule, self.save_best)

    def _init_rule(self, rule, key_indicator):
        if rule is not None and rule not in self.rule_map:
            raise KeyError(f'rule must be greater, less or None, but got {rule}.')
        if rule is None and key_indicator != 'auto':
            if any(key in key_indicator for key in self.greater_keys):
                rule = 'greater'
            elif any(key in key_indicator for key in self.less_keys):
                rule = 'less'
            else:
                raise ValueError(f'Cannot infer the rule for key {key_indicator}, thus a specific rule must be '
                                 'specified.')
        self.rule = rule
        self.key_indicator = key_indicator
        if self.rule is not None:
            self.compare_func = self.rule_map[self.rule]

    def before_run(self, runner):
        if self.save_best is not None:
            if runner.meta is None:
                warnings.warn('runner.meta is None. Creating a empty one.')
                runner.meta = dict()
            runner.meta.setdefault('hook_msgs', dict())

    def before_train_epoch(self, runner):
        """A resumed run is evaluated once before its first epoch."""
        if not self.initial_epoch_flag:
            return
        if self.start is not None and runner.epoch >= self.start:
            self.after_train_epoch(runner)
        self.initial_epoch_flag = False

    def evaluation_flag(self, runner):
        if self.start is None:
            return self.every_n_epochs(runner, self.interval)
        if (runner.epoch + 1) < self.start:
            return False
        return (runner.epoch + 1 - self.start) % self.interval == 0

    def use_flat(self):
        if self.flat is not None:
            return bool(self.flat)
        # measured (tools/val_loop_bench.py): the flat pass takes 0.32 of the list pass, far outside the spread
        return bool(getattr(self.dataloader.dataset, 'accepts_flat', False))

    def _test_loop(self, runner):
        from .apis import single_gpu_test
        return single_gpu_test(runner.model, self.dataloader, flat=self.use_flat())

    def _run(self, runner):
        was_training = runner.model.training
        results = self._test_loop(runner)
        runner.model.train(was_training)
        if runner.rank == 0 or not self.distributed:
            key_score = self.evaluate(runner, results)
            if self.save_best:
                self.save_best_checkpoint(runner, key_score)

    def after_train_epoch(self, runner):
        if self.by_epoch and self.evaluation_flag(runner):
            self._run(runner)

    def after_train_iter(self, runner):
        if not self.by_epoch and self.every_n_iters(runner, self.interval):
            self._run(runner)

    def save_best_checkpoint(self, runner, key_score):
        msgs = runner.meta['hook_msgs']
        best_score = msgs.get('best_score', self.init_value_map[self.rule])
        if not self.compare_func(key_score, best_score):
            return
        msgs['best_score'] = key_score
        last_ckpt = msgs['last_ckpt']
        msgs['best_ckpt'] = last_ckpt
        link = os.path.join(runner.work_dir, f'best_{self.key_indicator}.pth')
        if os.path.lexists(link):
            os.remove(link)
        same_dir = os.path.abspath(os.path.dirname(last_ckpt)) == os.path.abspath(runner.work_dir)
        os.symlink(os.path.basename(last_ckpt) if same_dir else os.path.abspath(last_ckpt), link)
        if runner.logger is not None:
            time_stamp = runner.epoch + 1 if self.by_epoch else runner.iter + 1
            runner.logger.info(f'Now best checkpoint is epoch_{time_stamp}.pth.'
                               f'Best {self.key_indicator} is {key_score:0.4f}')

    def evaluate(self, runner, results):
        eval_res = self.dataloader.dataset.evaluate(results, logger=runner.logger, **self.eval_kwargs)
        for name, val in eval_res.items():
            runner.log_buffer.output[name] = val
        runner.log_buffer.ready = True
        if self.save_best is None:
            return None
        if self.key_indicator == 'auto':
            self._init_rule(self.rule, list(eval_res.keys())[0])
        return eval_res[self.key_indicator]


@HOOKS.register_module()
class DistEvalHook(EvalHook):
    """``DistEvalHook`` of ``eval_hooks.py:190-303``: every rank runs its share of ``dataloader`` through
    ``multi_gpu_test``; rank 0 evaluates and saves, the others do neither.

    ``tmpdir`` is accepted and unused: the gather is ``dist.collect_results`` / ``dist.collect_flat`` (collectives), not
    the reference's shared temporary directory.  ``gpu_collect`` puts the gather's buffers on the rank's GPU; an RCCL
    group has no other place for them, so it is implied there.

    ``broadcast_bn_buffer``: the reference broadcasts ``running_var`` and ``running_mean`` of every tracked BatchNorm
    from rank 0, two collectives per layer.  Here they are segments of the model's ``FlatState`` arena, sent as one
    broadcast per contiguous run of them (one, for a model whose float buffers are all BatchNorm statistics), followed
    by ``bump_versions()`` so that the eval plans fold the received statistics."""

    distributed = True

    def __init__(self, dataloader, start=None, interval=1, by_epoch=True, tmpdir=None, gpu_collect=False, save_best=None,
                 rule=None, broadcast_bn_buffer=True, flat=None, **eval_kwargs):
        super().__init__(dataloader, start=start, interval=interval, by_epoch=by_epoch, save_best=save_best, rule=rule,
                         flat=flat, **eval_kwargs)
        self.broadcast_bn_buffer = broadcast_bn_buffer
        self.tmpdir = tmpdir
        self.gpu_collect = gpu_collect

    def _broadcast_bn_buffer(self, runner):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 0
        model = _unwrap(runner.model)
        flat = FlatState.of(model)
        runs = bn_stat_runs(model, flat)
        for lo, hi in runs:
            dist.broadcast(flat.values[lo:hi], 0)
        if runs:
            flat.bump_versions()
        return len(runs)

    def _test_loop(self, runner):
        from . import dist as D
        from .apis import multi_gpu_test
        if self.broadcast_bn_buffer:
            self._broadcast_bn_buffer(runner)
        return multi_gpu_test(runner.model, self.dataloader, gpu_collect=self.gpu_collect or D.backend_name() == 'nccl',
                              flat=self.use_flat())


# ---- the runner protocol the hooks are driven through ------------------------------------------------
class _Sampler:
    def __init__(self, samples_per_gpu):
        self.samples_per_gpu = samples_per_gpu


class BatchSource:
    """Anything iterable over ``train_step`` data dicts, plus the one attribute the hooks read
    from mmcv's loader: ``sampler.samples_per_gpu``."""

    def __init__(self, batches, samples_per_gpu):
        self.batches = batches
        self.sampler = _Sampler(samples_per_gpu)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class LogBuffer:
    def __init__(self):
        self.history = []
        self.by_name = OrderedDict()      # name -> [(entry, count)]: mmcv's val_history / n_history, entries by reference
        self.output = OrderedDict()      # mmcv LogBuffer.output: what the evaluation hooks write their metrics into
        self.ready = False

    #: ``False``: ``update`` drops what it is given (``EpochBasedRunner`` sets it when no logger hook would ever read or
    #: clear the history, which would otherwise grow, pinned buffers and events included, for the whole run)
    keep = True

    def update(self, values, count=1):
        if not self.keep:
            return
        # a DeferredLogVars stays as it is (copying it would wait for the device); its names are known without its values
        entry = values if getattr(values, 'pending', False) else dict(values)
        self.history.append((entry, count))
        for k in dict.keys(entry):
            self.by_name.setdefault(k, []).append((entry, count))

    def average(self, n=0):
        """mmcv ``LogBuffer.average``: per variable the mean of its last ``n`` entries (all of them for ``n=0``)
        weighted by their ``count``, into ``output``, in the order the variables first appeared.  This is where pending
        entries are read: the caller -- a logger hook at its interval -- waits for their copies, nobody else does.
        Per-variable lists (mmcv's ``val_history``) make a call cost ``n`` reads a variable, wherever in the epoch."""
        assert n >= 0
        for k, entries in self.by_name.items():
            last = entries[-n:]
            self.output[k] = sum(e[k] * c for e, c in last) / sum(c for _, c in last)
        self.ready = True

    def clear(self):
        self.history.clear()
        self.by_name.clear()
        self.clear_output()

    def clear_output(self):
        self.output.clear()
        self.ready = False


class Runner:
    """The slice of mmcv's ``EpochBasedRunner`` the three hooks touch: ``model``, ``optimizer``,
    ``iter``, ``epoch``, ``max_epochs``, ``outputs``, ``data_loader``, ``log_buffer``, ``meta``,
    hooks called in priority order at each stage, ``outputs = model.train_step(data, optimizer)``
    per iteration (mmcv ``epoch_based_runner.py`` ``run_iter``/``train``)."""

    def __init__(self, model, optimizer, logger=None, meta=None, max_epochs=1, work_dir=None):
        self.model, self.optimizer, self.logger = model, optimizer, logger
        self.work_dir = work_dir
        self.meta = meta if meta is not None else {}
        self.max_epochs = max_epochs
        self.iter = 0
        self.epoch = 0
        self.inner_iter = 0
        self.outputs = None
        self.data_loader = None
        self.log_buffer = LogBuffer()
        self._hooks = []

    def register_hook(self, hook, priority='NORMAL'):
        pr = PRIORITY[priority] if isinstance(priority, str) else int(priority)
        hook.priority = pr
        # mmcv inserts after the last hook of equal or higher priority
        i = len(self._hooks)
        while i > 0 and self._hooks[i - 1].priority > pr:
            i -= 1
        self._hooks.insert(i, hook)

    def register_hook_from_cfg(self, cfg):
        from .registry import build_from_cfg
        cfg = dict(cfg)
        priority = cfg.pop('priority', 'NORMAL')
        self.register_hook(build_from_cfg(cfg, HOOKS), priority)

    # ---- mmcv ``BaseRunner.register_training_hooks`` and its helpers (``base_runner.py``, mmcv 1.3.2 .. 1.4.0) ---------
    def register_lr_hook(self, lr_config):
        """``policy='step'`` names ``StepLrUpdaterHook``: the policy, title-cased when it is all lower case, plus
        ``LrUpdaterHook``.  A hook object is registered as it is."""
        if lr_config is None:
            return
        if isinstance(lr_config, dict):
            assert 'policy' in lr_config
            cfg = dict(lr_config)
            policy = cfg.pop('policy')
            if policy == policy.lower():
                policy = policy.title()
            name = policy + 'LrUpdaterHook'
            if HOOKS.get(name) is None:
                raise NotImplementedError(f"lr_config policy {lr_config['policy']!r} ({name}) is not built: "
                                          "'step' and 'CosineAnnealing' are")
            cfg['type'] = name
            hook = HOOKS.build(cfg)
        else:
            hook = lr_config
        self.register_hook(hook, 'VERY_HIGH')

    def register_momentum_hook(self, momentum_config):
        if momentum_config is not None:
            raise NotImplementedError(f'momentum_config={momentum_config!r}: no momentum updater hook is built (the '
                                      'YOLOv4 recipe warms the momentum up through DetailedLinearWarmUpHook)')

    def register_optimizer_hook(self, optimizer_config):
        if optimizer_config is None:
            return
        if isinstance(optimizer_config, dict):
            cfg = dict(optimizer_config)
            cfg.setdefault('type', 'OptimizerHook')
            hook = HOOKS.build(cfg)
        else:
            hook = optimizer_config
        self.register_hook(hook, 'ABOVE_NORMAL')

    def register_checkpoint_hook(self, checkpoint_config):
        if checkpoint_config is None:
            return
        if isinstance(checkpoint_config, dict):
            cfg = dict(checkpoint_config)
            cfg.setdefault('type', 'CheckpointHook')
            hook = HOOKS.build(cfg)
        else:
            hook = checkpoint_config
        self.register_hook(hook, 'NORMAL')

    def register_logger_hooks(self, log_config):
        if log_config is None:
            return
        log_interval = log_config['interval']
        for info in log_config['hooks']:
            if HOOKS.get(info['type']) is None or not issubclass(HOOKS.get(info['type']), LoggerHook):
                raise NotImplementedError(f"log_config: logger hook {info['type']!r} is not built: TextLoggerHook is")
            self.register_hook(HOOKS.build(dict(info), default_args=dict(interval=log_interval)), 'VERY_LOW')

    def register_training_hooks(self, lr_config, optimizer_config=None, checkpoint_config=None, log_config=None,
                                momentum_config=None):
        """The default training hooks in mmcv's order and at mmcv's priorities: lr updater ``VERY_HIGH``, (momentum
        updater ``HIGH``: refused), optimizer ``ABOVE_NORMAL``, checkpoint ``NORMAL``, ``IterTimerHook`` ``LOW``, logger
        hooks ``VERY_LOW``.  Hooks of one priority run in the order they were registered."""
        self.register_lr_hook(lr_config)
        self.register_momentum_hook(momentum_config)
        self.register_optimizer_hook(optimizer_config)
        self.register_checkpoint_hook(checkpoint_config)
        self.register_hook(IterTimerHook(), 'LOW')
        self.register_logger_hooks(log_config)

    def current_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def call_hook(self, stage):
        for h in self._hooks:
            getattr(h, stage)(self)

    @property
    def rank(self):
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    @property
    def max_iters(self):
        return self.max_epochs * len(self.data_loader)

    # ---- checkpoints: mmcv ``BaseRunner.save_checkpoint`` / ``resume`` (``epoch_based_runner.py``,
    # ``base_runner.py``): {'meta': {..., epoch, iter}, 'state_dict': weights on the CPU (the ``ema_*`` buffers
    # included: they are registered buffers, ema_hooks.py:52-64), 'optimizer': torch-layout state dict} ------------
    def save_checkpoint(self, out_dir, filename_tmpl='epoch_{}.pth', save_optimizer=True, meta=None,
                        create_symlink=True):
        import os
        import time
        from collections import OrderedDict
        for h in self._hooks:
            if hasattr(h, 'sync_meta'):
                h.sync_meta(self)
        meta = dict(meta or {})
        meta.update(self.meta or {})
        meta.update(epoch=self.epoch + 1, iter=self.iter, time=time.asctime())
        model = _unwrap(self.model)
        state = OrderedDict((k, v.detach().cpu()) for k, v in model.state_dict().items())
        ckpt = dict(meta=meta, state_dict=state)
        if save_optimizer and self.optimizer is not None:
            ckpt['optimizer'] = self.optimizer.state_dict()
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, filename_tmpl.format(self.epoch + 1))
        torch.save(ckpt, path)
        if create_symlink:
            link = os.path.join(out_dir, 'latest.pth')
            if os.path.islink(link) or os.path.exists(link):
                os.remove(link)
            os.symlink(os.path.basename(path), link)
        return path

    def load_checkpoint(self, filename, map_location='cpu', strict=False):
        ckpt = torch.load(filename, map_location=map_location, weights_only=False)
        state = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt
        if all(k.startswith('module.') for k in state):
            state = {k[7:]: v for k, v in state.items()}
        model = _unwrap(self.model)
        missing, unexpected = model.load_state_dict(state, strict=strict)
        flat = getattr(model, '_flat_state', None)
        if flat is not None:
            flat.bump_versions()
        elif hasattr(model, 'invalidate_plans'):
            model.invalidate_plans()
        ckpt['_missing_keys'], ckpt['_unexpected_keys'] = list(missing), list(unexpected)
        return ckpt

    def resume(self, checkpoint, resume_optimizer=True, map_location='cpu'):
        ckpt = self.load_checkpoint(checkpoint, map_location=map_location)
        self.epoch = ckpt['meta']['epoch']
        self.iter = ckpt['meta']['iter']
        hook_msgs = dict((self.meta or {}).get('hook_msgs', {}))
        hook_msgs.update(ckpt['meta'].get('hook_msgs', {}))
        self.meta = dict(ckpt['meta'])                       # mmcv: "resume meta information meta"
        self.meta['hook_msgs'] = hook_msgs
        if 'optimizer' in ckpt and resume_optimizer and self.optimizer is not None:
            self.optimizer.load_state_dict(ckpt['optimizer'])
        return ckpt

    def run(self, data_loader, max_epochs=None):
        if max_epochs is not None:
            self.max_epochs = max_epochs
        self.data_loader = data_loader
        self.call_hook('before_run')
        while self.epoch < self.max_epochs:
            self.model.train()
            self.call_hook('before_train_epoch')
            for i, data in enumerate(data_loader):
                self.inner_iter = i
                self.call_hook('before_train_iter')
                self.outputs = self.model.train_step(data, self.optimizer)
                self.call_hook('after_train_iter')
                self.iter += 1
            self.call_hook('after_train_epoch')
            self.epoch += 1
        self.call_hook('after_run')


# ---- the timer and the text logger (mmcv/runner/hooks/iter_timer.py, logger/base.py, logger/text.py) ---------------
@HOOKS.register_module()
class IterTimerHook(Hook):
    """mmcv's ``IterTimerHook``: ``data_time`` (from the end of the last iteration to the start of this one: the
    loader) and ``time`` (the same, to the end of this iteration's hooks) into the log buffer, from ``time.time()``.
    Nothing waits for the device here, so ``time`` is host time: how long the host took to QUEUE the iteration.  Over a
    logging interval its mean is the device's time per iteration as soon as the host runs ahead of the device and is
    held back by it (the loader's decode status read, a full launch queue); a single value says little."""

    def before_epoch(self, runner):
        self.t = time.time()

    def before_iter(self, runner):
        runner.log_buffer.update({'data_time': time.time() - self.t})

    def after_iter(self, runner):
        runner.log_buffer.update({'time': time.time() - self.t})
        self.t = time.time()


class LoggerHook(Hook):
    """mmcv's ``LoggerHook`` base: when to average the log buffer and call ``log``."""

    def __init__(self, interval=10, ignore_last=True, reset_flag=False, by_epoch=True):
        self.interval, self.ignore_last, self.reset_flag, self.by_epoch = interval, ignore_last, reset_flag, by_epoch

    def log(self, runner):
        raise NotImplementedError

    def before_run(self, runner):
        for hook in runner._hooks[::-1]:            # the last logger hook of the run clears the output
            if isinstance(hook, LoggerHook):
                hook.reset_flag = True
                break

    def before_epoch(self, runner):
        runner.log_buffer.clear()

    def _flush(self, runner):
        if runner.log_buffer.ready:
            self.log(runner)
            if self.reset_flag:
                runner.log_buffer.clear_output()

    def after_train_iter(self, runner):
        if self.by_epoch and (runner.inner_iter + 1) % self.interval == 0:
            runner.log_buffer.average(self.interval)
        elif not self.by_epoch and self.every_n_iters(runner, self.interval):
            runner.log_buffer.average(self.interval)
        elif runner.inner_iter + 1 == len(runner.data_loader) and not self.ignore_last:
            runner.log_buffer.average(self.interval)      # not precise, but more stable (mmcv)
        self._flush(runner)

    def after_train_epoch(self, runner):
        self._flush(runner)


def _round_float(items):
    if isinstance(items, (list, tuple)):
        return [_round_float(x) for x in items]
    if isinstance(items, float):
        return round(items, 5)
    if hasattr(items, 'item') and getattr(items, 'ndim', 1) == 0:          # a numpy scalar (the scorers return them)
        return _round_float(items.item())
    return items


@HOOKS.register_module()
class TextLoggerHook(LoggerHook):
    """mmcv's ``TextLoggerHook`` on rank 0: every ``interval`` iterations one line through ``runner.logger`` --
    ``Epoch [e][i/n]\\tlr: 1.000e-02, eta: 0:00:10, time: 0.100, data_time: 0.010, memory: 123, loss_cls: 0.5000, ...``
    -- and one JSON object in ``<work_dir>/<timestamp>.log.json`` (``mode``, ``epoch``, ``iter``, ``lr``, ``memory``,
    then the averaged variables in the order they reached the buffer, floats rounded to 5 digits).  After an evaluation
    the metrics the evaluation hook left in ``log_buffer.output`` go out as a ``mode: 'val'`` line.  The first JSON line
    is ``runner.meta``.  ``memory`` is ``torch.cuda.max_memory_allocated`` in MB, the maximum over the ranks (one
    reduce per logged line).  ``lr`` is the first group's."""

    def __init__(self, by_epoch=True, interval=10, ignore_last=True, reset_flag=False, interval_exp_name=1000):
        super().__init__(interval, ignore_last, reset_flag, by_epoch)
        self.time_sec_tot = 0
        self.interval_exp_name = interval_exp_name
        self.json_log_path = None

    def before_run(self, runner):
        super().before_run(runner)
        self.start_iter = runner.iter
        if runner.work_dir is not None:
            self.json_log_path = os.path.join(runner.work_dir, f"{getattr(runner, 'timestamp', None)}.log.json")
            if runner.meta is not None:
                self._dump_log(runner.meta, runner)

    def _max_memory(self, runner):
        import torch.distributed as dist
        device = next(_unwrap(runner.model).parameters()).device
        mem_mb = int(torch.cuda.max_memory_allocated(device) / (1024 * 1024)) if device.type == 'cuda' else 0
        if _world_size() > 1:
            t = torch.tensor([mem_mb], dtype=torch.int, device=device if str(dist.get_backend()) == 'nccl' else 'cpu')
            dist.reduce(t, 0, op=dist.ReduceOp.MAX)
            mem_mb = int(t.item())
        return mem_mb

    def _log_info(self, log_dict, runner):
        if runner.logger is None:
            return
        import datetime
        meta = runner.meta
        if meta is not None and 'exp_name' in meta:
            if self.every_n_iters(runner, self.interval_exp_name) or \
                    (self.by_epoch and runner.inner_iter + 1 == len(runner.data_loader)):
                runner.logger.info(f"Exp name: {meta['exp_name']}")
        if log_dict['mode'] == 'train':
            lr_str = f"lr: {log_dict['lr']:.3e}"
            if self.by_epoch:
                log_str = f"Epoch [{log_dict['epoch']}][{log_dict['iter']}/{len(runner.data_loader)}]\t"
            else:
                log_str = f"Iter [{log_dict['iter']}/{runner.max_iters}]\t"
            log_str += f'{lr_str}, '
            if 'time' in log_dict:
                self.time_sec_tot += log_dict['time'] * self.interval
                time_sec_avg = self.time_sec_tot / (runner.iter - self.start_iter + 1)
                eta_sec = time_sec_avg * (runner.max_iters - runner.iter - 1)
                log_str += f'eta: {datetime.timedelta(seconds=int(eta_sec))}, '
                log_str += f"time: {log_dict['time']:.3f}, data_time: {log_dict['data_time']:.3f}, "
                if 'memory' in log_dict:
                    log_str += f"memory: {log_dict['memory']}, "
        elif self.by_epoch:
            log_str = f"Epoch({log_dict['mode']}) [{log_dict['epoch']}][{log_dict['iter']}]\t"
        else:
            log_str = f"Iter({log_dict['mode']}) [{log_dict['iter']}]\t"
        items = []
        for name, val in log_dict.items():
            if name in ('mode', 'Epoch', 'iter', 'lr', 'time', 'data_time', 'memory', 'epoch'):
                continue
            if isinstance(val, float):
                val = f'{val:.4f}'
            items.append(f'{name}: {val}')
        runner.logger.info(log_str + ', '.join(items))

    def _dump_log(self, log_dict, runner):
        if runner.rank != 0 or self.json_log_path is None:
            return
        import json
        json_log = OrderedDict((k, _round_float(v)) for k, v in log_dict.items())
        with open(self.json_log_path, 'a+') as f:
            f.write(json.dumps(json_log, default=str) + '\n')

    def log(self, runner):
        out = runner.log_buffer.output
        cur_iter = out.pop('eval_iter_num') if 'eval_iter_num' in out else runner.inner_iter + 1
        # (the evaluation hooks run inside the train workflow: a line without 'time' is theirs)
        log_dict = OrderedDict(mode='train' if 'time' in out else 'val', epoch=runner.epoch + 1, iter=cur_iter)
        log_dict['lr'] = runner.current_lr()[0]
        if 'time' in out and torch.cuda.is_available():
            log_dict['memory'] = self._max_memory(runner)
        log_dict = OrderedDict(log_dict, **{k: (v.item() if hasattr(v, 'item') and getattr(v, 'ndim', 1) == 0 else v)
                                            for k, v in out.items()})
        if runner.rank == 0:
            self._log_info(log_dict, runner)
        self._dump_log(log_dict, runner)
        return log_dict


# ---- the runner a config names ---------------------------------------------------------------------------------------
@RUNNERS.register_module()
class EpochBasedRunner(Runner):
    """``Runner`` plus what mmcv's ``EpochBasedRunner`` does for its logger hooks: after every iteration
    ``outputs['log_vars']`` goes into the log buffer weighted by ``num_samples`` -- a ``DeferredLogVars`` as it is,
    still pending, so the loop waits for nothing and the logger pays the read-back at its interval --, ``timestamp``
    names the ``.log.json`` file, and a resumed run keeps the ``config`` text of the run that resumes (``StateEMAHook``
    looks for ``resume_from`` in it)."""

    def __init__(self, model, optimizer=None, work_dir=None, logger=None, meta=None, max_epochs=None, max_iters=None,
                 batch_processor=None):
        if max_iters is not None or batch_processor is not None:
            raise NotImplementedError('EpochBasedRunner: max_iters / batch_processor are not built; give max_epochs')
        super().__init__(model, optimizer, logger=logger, meta=meta, max_epochs=max_epochs, work_dir=work_dir)
        self.timestamp = None
        self.mode = 'train'
        if work_dir is not None:
            os.makedirs(work_dir, exist_ok=True)

    @property
    def world_size(self):
        return _world_size()

    @property
    def rank(self):
        """The process group's rank; without a group the launcher's ``RANK`` (0 when unset), as ``get_root_logger``."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank()
        return int(os.environ.get('RANK', '0'))

    def resume(self, checkpoint, resume_optimizer=True, map_location='cpu'):
        mine = {k: self.meta[k] for k in ('config', 'exp_name', 'seed', 'env_info') if k in (self.meta or {})}
        ckpt = super().resume(checkpoint, resume_optimizer=resume_optimizer, map_location=map_location)
        self.meta.update(mine)
        if self.logger is not None:
            self.logger.info('resumed epoch %d, iter %d', self.epoch, self.iter)
        return ckpt

    def run(self, data_loader, workflow=None, max_epochs=None):
        if workflow is not None and [tuple(w) for w in workflow] != [('train', 1)]:
            raise NotImplementedError(f"workflow={workflow!r}: only [('train', 1)] is built (validation runs through "
                                      'EvalHook)')
        if isinstance(data_loader, (list, tuple)):
            assert len(data_loader) == 1
            data_loader = data_loader[0]
        if max_epochs is not None:
            self.max_epochs = max_epochs
        assert self.max_epochs is not None, 'max_epochs must be specified during instantiation'
        self.data_loader = data_loader
        self.log_buffer.keep = any(isinstance(h, LoggerHook) for h in self._hooks)
        if self.logger is not None:
            self.logger.info('Start running, work_dir: %s, max: %d epochs', self.work_dir, self.max_epochs)
        self.call_hook('before_run')
        while self.epoch < self.max_epochs:
            self.model.train()
            self.call_hook('before_train_epoch')
            for i, data in enumerate(data_loader):
                self.inner_iter = i
                self.call_hook('before_train_iter')
                self.outputs = self.model.train_step(data, self.optimizer)
                if 'log_vars' in self.outputs:
                    self.log_buffer.update(self.outputs['log_vars'], self.outputs['num_samples'])
                self.call_hook('after_train_iter')
                self.iter += 1
            self.call_hook('after_train_epoch')
            self.epoch += 1
        self.call_hook('after_run')


def build_runner(cfg, default_args=None):
    """mmcv ``build_runner``: ``cfg.runner`` (``dict(type='EpochBasedRunner', max_epochs=...)``) with the model,
    optimizer, work_dir, logger and meta as ``default_args``."""
    if cfg.get('type') != 'EpochBasedRunner':
        raise NotImplementedError(f"runner type {cfg.get('type')!r} is not built: EpochBasedRunner is")
    return RUNNERS.build(dict(cfg), default_args=default_args)
