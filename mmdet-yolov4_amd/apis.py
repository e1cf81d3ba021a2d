"""``inference_detector`` under the reference's name (``mmdet/apis/inference.py:88-158``).

The reference composes ``cfg.data.test.pipeline`` per image on the CPU (mmcv / OpenCV), collates, scatters and calls
``model(return_loss=False, rescale=True, **data)``.  Here the same pipeline block drives ``FusedTestPipeline`` (one
launch per image, parity unpinned -- see ``preprocess.py``) and the detector's fused ``simple_test``.  Image files are
read by ``image_io.imread`` (the reference reads them with ``mmcv.imread``): baseline JPEG, decoded on the GPU to the
bytes libjpeg-turbo gives; EXIF orientation is not applied."""
import os

import numpy as np
import torch

from .image_io import imread

from .preprocess import FusedTestPipeline


def inference_detector(model, imgs, test_pipeline=None):
    """``imgs``: an (h, w, 3) uint8 array (BGR, as ``mmcv.imread`` returns), a (h, w, 3) ``torch.uint8`` tensor on the
    model's device, a file name (``str`` / ``os.PathLike``: a baseline JPEG, decoded on the GPU) or a list / tuple of
    them, mixed freely.  Returns the per-image result (a list of per-class (k, 5) arrays) or, for a list, the list of
    them -- like the reference.  ``test_pipeline`` defaults to ``model.cfg.data.test.pipeline``."""
    is_batch = isinstance(imgs, (list, tuple))
    if not is_batch:
        imgs = [imgs]
    for i in imgs:
        if not isinstance(i, (np.ndarray, torch.Tensor, str, os.PathLike)):
            raise TypeError(f'inference_detector takes arrays, uint8 tensors and file names, not {type(i).__name__}')
    if test_pipeline is None:
        cfg = getattr(model, 'cfg', None)
        if cfg is None:
            raise ValueError('pass test_pipeline= or attach the config as model.cfg (init_detector does in the reference)')
        test_pipeline = cfg.data.test.pipeline
    device = next(model.parameters()).device
    pipe = test_pipeline if callable(test_pipeline) else FusedTestPipeline.from_config(test_pipeline, device=device)
    imgs = list(imgs)
    files = [k for k, i in enumerate(imgs) if isinstance(i, (str, os.PathLike))]
    if files:       # the files of the call are one decode batch
        for k, img in zip(files, imread([imgs[k] for k in files], device=device)):
            imgs[k] = img
    batch, metas = pipe(imgs)
    with torch.no_grad():
        if isinstance(batch, list):      # test-time augmentation: one batch per augmentation (N images each)
            results = model.aug_test(batch, metas, rescale=True)
        else:
            results = model.simple_test(batch, metas, rescale=True)
    return results if is_batch else results[0]


def _unwrap(field):
    """A test-time batch carries one entry per augmentation (``img=[tensor]``, ``img_metas=[[meta, ...]]``); with one
    augmentation the path is ``BaseDetector.forward_test`` -> ``simple_test`` (mmdet/models/detectors/base.py:128-166)."""
    if isinstance(field, (list, tuple)) and len(field) == 1 and isinstance(field[0], (list, tuple, torch.Tensor)):
        return field[0]
    return field


def _test_batches(data_loader, device):
    """``(img, img_metas, tta)`` per batch of a test loader: ``tta`` batches keep one entry per augmentation
    (BaseDetector.forward_test -> aug_test, detectors/base.py:147-153).  The flat loop's copy of the unwrapping that
    ``single_gpu_test``'s list loop keeps inline: that loop is the yardstick the flat one is measured against and stays
    as it was, so a change to the batch format has to be made in both."""
    for data in data_loader:
        img, metas = data['img'], data['img_metas']
        if isinstance(img, (list, tuple)) and len(img) > 1:
            yield [t.to(device, non_blocking=True) for t in img], list(metas), True
        else:
            yield _unwrap(img).to(device, non_blocking=True), _unwrap(metas), False


def _flat_loop(model, data_loader, position):
    """The test loop with the result table built on the device (``results.DeviceResults``): ``position(j)`` is the
    dataset position of the loop's j-th image.  Per batch the host reads the (N,) counts and nothing else;
    test-time-augmentation batches come back as lists (``aug_test``) and are uploaded once."""
    from .results import DeviceResults
    model.eval()
    device = next(model.parameters()).device
    table = DeviceResults(model.bbox_head.num_classes, device)
    seen = 0
    with torch.no_grad():
        for img, metas, tta in _test_batches(data_loader, device):
            n = len(metas[0]) if tta else len(metas)
            index = [position(seen + j) for j in range(n)]
            if tta:
                table.append_lists(model.forward_test(img, metas, rescale=True), index)
            else:
                model.simple_test(img, metas, rescale=True, results=table, img_index=index)
            seen += n
    return table.tensors()


def _show_metas(metas):
    """The per-image metas of a batch: a test-time-augmentation batch nests them per augmentation."""
    return metas[0] if metas and isinstance(metas[0], (list, tuple)) else metas


def _show_batch(model, metas, batch_results, out_dir, score_thr):
    """The visualisation branch of the reference's loop (``mmdet/apis/test.py:30-57``) for one batch: the ORIGINAL files
    (``img_meta['filename']``) are decoded, drawn on and written to ``out_dir / ori_filename`` in one ``show_results``
    call.  The reference draws on the de-normalised network input resized back to the original size; the boxes are in
    original coordinates either way."""
    metas = _show_metas(metas)
    for m in metas:
        for key in ('filename', 'ori_filename'):
            if not m.get(key):
                raise ValueError(f"single_gpu_test(out_dir=...) reads the picture from img_meta[{key!r}], which this "
                                 'batch does not carry')
    model.show_results([m['filename'] for m in metas], batch_results,
                       [os.path.join(out_dir, m['ori_filename']) for m in metas], score_thr=score_thr)


def single_gpu_test(model, data_loader, flat=False, show=False, out_dir=None, show_score_thr=0.3):
    """Run the detector over ``data_loader`` and return the list of per-image results
    (``mmdet/apis/test.py:16-68``).  Each item is ``dict(img=..., img_metas=...)``
    as the test pipeline's collate produces; ``rescale=True`` like the reference's test loop.

    ``out_dir``: every image is drawn with its detections above ``show_score_thr`` and written to ``out_dir /
    img_meta['ori_filename']`` (a JPEG), one decode, draw and encode call per batch (``show_results``); the picture
    drawn on is the original file, not the de-normalised network input.  ``show=True`` raises: there is no display.

    ``flat=True`` returns the flat form instead -- ``(dets (D, 5) float32, labels (D,) int64, img_index (D,) int64)`` as
    GPU tensors, ``img_index`` the running image number -- equal to ``coco_eval.flatten_results`` of the list bit for
    bit, without the detections leaving the device."""
    if show:
        raise NotImplementedError('single_gpu_test(show=True): there is no display window; pass out_dir=')
    if flat and out_dir is not None:
        raise ValueError('single_gpu_test(flat=True, out_dir=...): drawing from the flat result table is not built')
    if flat:
        return _flat_loop(model, data_loader, lambda j: j)
    model.eval()
    device = next(model.parameters()).device
    results = []
    with torch.no_grad():
        for data in data_loader:
            img, metas = data['img'], data['img_metas']
            if isinstance(img, (list, tuple)) and len(img) > 1:
                # test-time augmentation: BaseDetector.forward_test -> aug_test (detectors/base.py:147-153)
                results.extend(model.forward_test([t.to(device, non_blocking=True) for t in img], list(metas),
                                                  rescale=True))
            else:
                img, metas = _unwrap(img), _unwrap(metas)
                results.extend(model.simple_test(img.to(device, non_blocking=True), metas, rescale=True))
            if out_dir is not None:
                _show_batch(model, list(metas), results[len(results) - len(_show_metas(metas)):], out_dir, show_score_thr)
    return results


def multi_gpu_test(model, data_loader, size=None, gpu_collect=True, flat=False):
    """Every rank runs its ``sampler_indices`` share, then rank 0 receives the merged, dataset-ordered list and the
    others ``None`` (``mmdet/apis/test.py:71-113``).  ``size`` defaults to ``len(data_loader.dataset)``.  With
    ``gpu_collect`` the byte buffers of the gather live on the rank's GPU (RCCL); otherwise on the host (gloo) --
    the reference's other branch goes through a shared temp directory instead.

    ``flat=True``: the flat form of ``single_gpu_test``.  Rank r's j-th image sits at dataset position ``j * world + r``
    (the sampler's round-robin deal), ``dist.collect_flat`` gathers the three tensors and rank 0 returns them ordered
    by position, without the sampler's padding, on the model's device."""
    from . import dist as D
    if size is None:
        size = len(data_loader.dataset)
    device = next(model.parameters()).device if gpu_collect else 'cpu'
    if flat:
        rank, world = D.rank_world()
        dets, labels, img_index = _flat_loop(model, data_loader, lambda j: j * world + rank)
        return D.collect_flat(dets, labels, img_index, size, device=device)
    results = single_gpu_test(model, data_loader)
    return D.collect_results(results, size, device=device)


# ---- the reference's ``mmdet/apis`` entry points for a run from a config file ----------------------------------------
def set_random_seed(seed, deterministic=False):
    """``apis/train.py:18-34``: seeds ``random``, ``numpy`` and ``torch`` (CPU and every device).  ``deterministic``
    additionally turns on this package's deterministic mode (``set_deterministic(True)``: the kernels whose reductions
    race take their ordered forms), which is what makes two runs of one seed bit-equal here; the cudnn switches the
    reference sets are set too and touch no kernel of this package."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    if deterministic:
        from .ops import set_deterministic
        set_deterministic(True)
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False


def get_root_logger(log_file=None, log_level='INFO'):
    """``mmdet/utils/logger.py`` over mmcv's ``get_logger`` (third-party, restated): THE logger ``'mmdet'``.  The first
    call gives it a stream handler on every rank and, on rank 0 when ``log_file`` is given, a file handler; ranks other
    than 0 log at ``ERROR``.  Later calls return it as it is."""
    import logging
    from .dist import env_world, rank_world
    logger = logging.getLogger('mmdet')
    if getattr(logger, '_yv4_initialised', False):
        return logger
    rank, world = rank_world()
    if world == 1:
        rank = env_world()[0]
    fmt = logging.Formatter('%(asctime)s - %(name)s - %(levelname)s - %(message)s')
    level = getattr(logging, log_level) if isinstance(log_level, str) else log_level
    handlers = [logging.StreamHandler()]
    if rank == 0 and log_file is not None:
        handlers.append(logging.FileHandler(log_file, 'w'))
    for h in handlers:
        h.setFormatter(fmt)
        h.setLevel(level)
        logger.addHandler(h)
    logger.setLevel(level if rank == 0 else logging.ERROR)
    logger.propagate = False
    logger._yv4_initialised = True
    return logger


def _load_config(config, cfg_options=None):
    from .registry import Config
    if isinstance(config, (str, os.PathLike)):
        config = Config.fromfile(os.fspath(config))
    elif not isinstance(config, Config):
        raise TypeError(f'config must be a filename or Config object, but got {type(config)}')
    if cfg_options is not None:
        config.merge_from_dict(cfg_options)
    return config


_DTYPES = {None: None, 'fp32': None, 'f32': None, torch.float32: None, 'fp16': torch.float16, 'f16': torch.float16,
           torch.float16: torch.float16, 'bf16': torch.bfloat16, torch.bfloat16: torch.bfloat16}


def load_weights(model, filename, map_location='cpu', strict=False):
    """mmcv ``load_checkpoint`` as ``Runner.load_checkpoint`` does it: a ``module.`` prefix is stripped, the load is
    not strict, the plans learn of the new weights.  Returns the checkpoint."""
    from .hooks import Runner
    return Runner(model, None).load_checkpoint(filename, map_location=map_location, strict=strict)


def init_detector(config, checkpoint=None, device='cuda:0', cfg_options=None, dtype=None):
    """``apis/inference.py:16-53``: the detector of ``config`` (a file name or a ``Config``) with the weights of
    ``checkpoint``, on ``device``, in eval mode, with ``model.cfg`` and ``model.CLASSES`` (the checkpoint's, else the 80
    COCO names with a warning) -- ready for ``inference_detector(model, 'file.jpg')``.  ``dtype`` (this package's):
    ``torch.float16`` / ``torch.bfloat16`` run the plans with 16-bit activations (``wrap_fp16_model``); a config with an
    ``fp16`` block means ``torch.float16``."""
    import warnings
    from .bricks import wrap_fp16_model
    from .datasets import COCO_CLASSES
    from .registry import build_detector
    config = _load_config(config, cfg_options)
    if dtype not in _DTYPES:
        raise ValueError(f'dtype {dtype!r} is not fp32, fp16 or bf16')
    config.model.pretrained = None
    config.model.train_cfg = None
    model = build_detector(config.model, test_cfg=config.get('test_cfg'))
    if checkpoint is not None:
        ckpt = load_weights(model, checkpoint, map_location='cpu')
        if 'CLASSES' in ckpt.get('meta', {}):
            model.CLASSES = ckpt['meta']['CLASSES']
        else:
            warnings.warn("Class names are not saved in the checkpoint's meta data, use COCO classes by default.")
            model.CLASSES = COCO_CLASSES
    model.cfg = config
    model.to(device)
    model.eval()
    compute = _DTYPES[dtype]
    if compute is None and config.get('fp16', None) is not None:
        compute = torch.float16
    if compute is not None:
        wrap_fp16_model(model, compute)
    return model


def samples_per_gpu(cfg, logger=None):
    """``cfg.data.samples_per_gpu``, or the deprecated ``imgs_per_gpu`` with the reference's warnings
    (``apis/train.py:48-60``); the config is left holding the value under the new name."""
    if 'imgs_per_gpu' in cfg.data:
        logger = logger or get_root_logger(log_level=cfg.get('log_level', 'INFO'))
        logger.warning('"imgs_per_gpu" is deprecated in MMDet V2.0. Please use "samples_per_gpu" instead')
        if 'samples_per_gpu' in cfg.data:
            logger.warning(f'Got "imgs_per_gpu"={cfg.data.imgs_per_gpu} and "samples_per_gpu"={cfg.data.samples_per_gpu}, '
                           f'"imgs_per_gpu"={cfg.data.imgs_per_gpu} is used in this experiments')
        else:
            logger.warning(f'Automatically set "samples_per_gpu"="imgs_per_gpu"={cfg.data.imgs_per_gpu} in this '
                           'experiments')
        cfg.data.samples_per_gpu = cfg.data.imgs_per_gpu
    return cfg.data.samples_per_gpu


def broadcast_model_state(model, src=0):
    """Every rank takes rank ``src``'s parameters and buffers: what constructing the reference's
    ``MMDistributedDataParallel`` does (``apis/train.py:74-82``; torch's DDP broadcasts the module's state from rank 0),
    so that ranks which initialised their weights from different random streams train ONE model.  Two broadcasts, the
    float arena and the integer arena of the model's ``FlatState``; a no-op without a process group.  Returns the
    number of collectives."""
    import torch.distributed as tdist
    if not (tdist.is_available() and tdist.is_initialized()):
        return 0
    from .flat_state import FlatState
    flat = FlatState.of(model.module if hasattr(model, 'module') and isinstance(model.module, torch.nn.Module) else model)
    sent = 0
    for arena in (flat.values, flat.ints):
        if arena.numel():
            tdist.broadcast(arena, src)
            sent += 1
    flat.bump_versions()
    return sent


def train_detector(model, dataset, cfg, distributed=False, validate=False, timestamp=None, meta=None, entropy=None,
                   prefetch=0):
    """``apis/train.py:37-170`` on this package's parts.  ``dataset``: ``cfg.data.train`` (a dataset block with its
    pipeline; ``build_train_loader`` makes the loader from it with ``cfg.data.samples_per_gpu``, ``cfg.seed`` and the
    process group's rank and world) or a ready ``TrainLoader``.  Optimizer: ``build_optimizer(model, cfg.optimizer)``;
    runner: ``cfg.runner`` (``EpochBasedRunner``; without it ``total_epochs``, with the reference's warning); hooks:
    ``register_training_hooks`` with the optimizer hook of ``build_optimizer_hook``, ``DistSamplerSeedHook`` (always: the
    loader's order is a function of the epoch, which a resumed run has to tell it), with ``validate`` the evaluation hook
    over ``build_test_loader(cfg.data.val)``, then ``custom_hooks`` at their priorities.  ``cfg.resume_from`` /
    ``cfg.load_from``, with ``distributed`` rank 0's parameters and buffers to every rank
    (``broadcast_model_state``: the reference's DDP wrapper does it), then the run.  ``entropy`` / ``prefetch``: the loaders' (``TrainLoader``)."""
    import warnings
    from . import dist as D
    from .datasets import TrainLoader, build_test_loader, build_train_loader
    from .hooks import (DistEvalHook, DistSamplerSeedHook, EvalHook, HOOKS, build_optimizer_hook, build_runner)
    from .optim import build_optimizer
    from .registry import build_from_cfg
    logger = get_root_logger(log_level=cfg.get('log_level', 'INFO'))
    workflow = cfg.get('workflow', [('train', 1)])
    if [tuple(w) for w in workflow] != [('train', 1)]:
        raise NotImplementedError(f"workflow={workflow!r}: only [('train', 1)] is built (validation runs through "
                                  'EvalHook)')
    if 'runner' not in cfg:
        cfg.runner = {'type': 'EpochBasedRunner', 'max_epochs': cfg.total_epochs}
        warnings.warn('config is now expected to have a `runner` section, please set `runner` in your config.',
                      UserWarning)
    elif 'total_epochs' in cfg:
        assert cfg.total_epochs == cfg.runner.max_epochs
    if cfg.runner['type'] != 'EpochBasedRunner':
        raise NotImplementedError(f"runner type {cfg.runner['type']!r} is not built: EpochBasedRunner is")

    rank, world = D.rank_world() if distributed else (0, 1)
    model = model.cuda() if next(model.parameters()).device.type != 'cuda' else model
    device = next(model.parameters()).device
    if isinstance(dataset, TrainLoader):
        loader = dataset
    else:
        if isinstance(dataset, (list, tuple)):
            if len(dataset) != 1:
                raise NotImplementedError('train_detector: one training dataset (the workflow has one phase)')
            dataset = dataset[0]
        loader = build_train_loader(dataset, samples_per_gpu(cfg, logger), seed=cfg.get('seed') or 0, rank=rank, world=world,
                                    device=device, entropy=entropy, prefetch=prefetch)

    optimizer = build_optimizer(model, cfg.optimizer)
    runner = build_runner(cfg.runner, default_args=dict(model=model, optimizer=optimizer, work_dir=cfg.get('work_dir'),
                                                        logger=logger, meta=meta))
    runner.timestamp = timestamp           # (so that the .log and .log.json names agree)
    optimizer_hook = build_optimizer_hook(cfg, distributed=distributed)
    runner.register_training_hooks(cfg.get('lr_config'), optimizer_hook, cfg.get('checkpoint_config'),
                                   cfg.get('log_config'), cfg.get('momentum_config', None))
    runner.register_hook(DistSamplerSeedHook())
    if validate:
        val_loader = build_test_loader(cfg.data.val, rank=rank, world=world, device=device, entropy=entropy,
                                       prefetch=prefetch)
        eval_cfg = dict(cfg.get('evaluation', {}) or {})
        eval_cfg['by_epoch'] = True
        runner.register_hook((DistEvalHook if distributed else EvalHook)(val_loader, **eval_cfg))
    if cfg.get('custom_hooks', None):
        custom_hooks = cfg.custom_hooks
        assert isinstance(custom_hooks, list), f'custom_hooks expect list type, but got {type(custom_hooks)}'
        for hook_cfg in custom_hooks:
            assert isinstance(hook_cfg, dict), f'Each item in custom_hooks expects dict type, but got {type(hook_cfg)}'
            hook_cfg = dict(hook_cfg)
            priority = hook_cfg.pop('priority', 'NORMAL')
            runner.register_hook(build_from_cfg(hook_cfg, HOOKS), priority=priority)
    if cfg.get('resume_from'):
        runner.resume(cfg.resume_from)
    elif cfg.get('load_from'):
        runner.load_checkpoint(cfg.load_from)
    if distributed:
        # the ranks' own init_weights() drew from their own random streams: one model from here on
        broadcast_model_state(model, 0)
    runner.run(loader, workflow)
    return runner
