#!/usr/bin/env python
"""Train a detector from a config file, the way the reference's ``tools/train.py`` does:
    python tools/train.py <config.py> --work-dir out
    python -m torch.distributed.run --nproc_per_node=8 tools/train.py <config.py> --launcher pytorch
The config is one of the reference's (``configs/yolov4/*.py``, ``configs/yolo/*.py``) or one written like them;
INTEGRATION.md lists the keys that are honoured, ignored and refused.  Writes into the work directory: the config as it
was run, ``<timestamp>.log``, ``<timestamp>.log.json``, ``epoch_N.pth`` / ``latest.pth`` and, with ``save_best``,
``best_<metric>.pth``."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DTYPES = ('fp32', 'fp16', 'bf16')


def parse_args(argv=None):
    from mmdet_yolov4_amd.registry import DictAction
    parser = argparse.ArgumentParser(description='Train a detector')
    parser.add_argument('config', help='train config file path')
    parser.add_argument('--work-dir', help='the dir to save logs and models')
    parser.add_argument('--resume-from', help='the checkpoint file to resume from')
    parser.add_argument('--no-validate', action='store_true',
                        help='whether not to evaluate the checkpoint during training')
    group_gpus = parser.add_mutually_exclusive_group()
    group_gpus.add_argument('--gpus', type=int, help='number of gpus to use (only applicable to non-distributed training)')
    group_gpus.add_argument('--gpu-ids', type=int, nargs='+',
                            help='ids of gpus to use (only applicable to non-distributed training)')
    parser.add_argument('--seed', type=int, default=None, help='random seed')
    parser.add_argument('--deterministic', action='store_true',
                        help="bit-equal runs of one seed: the package's deterministic kernels")
    parser.add_argument('--cfg-options', nargs='+', action=DictAction,
                        help='override settings of the config: key=value pairs, e.g. data.samples_per_gpu=4 '
                             'lr_config.step=[8,11]')
    parser.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none', help='job launcher')
    parser.add_argument('--local_rank', type=int, default=0)
    parser.add_argument('--dtype', choices=DTYPES, default='fp32',
                        help='activation / conv operand type (master weights, statistics and losses stay fp32)')
    parser.add_argument('--entropy', choices=['host', 'device', 'device_sync'], default=None,
                        help="where the loaders' JPEG Huffman decode runs (default: the package's)")
    parser.add_argument('--prefetch', type=int, default=1, choices=[0, 1],
                        help="1: the next batch's file reads and host decode half run beside the step")
    args = parser.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    return args


def refuse_launch(args):
    """What this tool does not build, by name, before anything else happens."""
    if args.launcher in ('slurm', 'mpi'):
        raise NotImplementedError(f"--launcher {args.launcher} is not built: 'none' and 'pytorch' (one process per GPU, "
                                  'rank and world from the environment) are')
    gpus = getattr(args, 'gpus', None)
    ids = getattr(args, 'gpu_ids', None)
    if args.launcher == 'none' and ((gpus is not None and gpus > 1) or (ids is not None and len(ids) > 1)):
        raise NotImplementedError('--gpus / --gpu-ids above one GPU without a launcher (the reference\'s DataParallel) '
                                  'is not built: start one process per GPU with --launcher pytorch')


def env_info():
    import torch
    import mmdet_yolov4_amd as pkg
    rows = [('sys.platform', sys.platform), ('Python', sys.version.replace('\n', '')), ('PyTorch', torch.__version__),
            ('HIP', getattr(torch.version, 'hip', None)), ('GPU 0', torch.cuda.get_device_name(0)),
            ('mmdet_yolov4_amd', pkg.__version__)]
    return '\n'.join(f'{k}: {v}' for k, v in rows)


def main(argv=None):
    args = parse_args(argv)
    refuse_launch(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/train.py: no GPU is visible (torch.cuda.is_available() is False); nothing was built')
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import dist as D
    from mmdet_yolov4_amd.apis import samples_per_gpu
    from mmdet_yolov4_amd.registry import Config

    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    if args.work_dir is not None:                      # CLI > the file's work_dir > the file's name
        cfg.work_dir = args.work_dir
    elif cfg.get('work_dir', None) is None:
        cfg.work_dir = os.path.join('./work_dirs', os.path.splitext(os.path.basename(args.config))[0])
    if args.resume_from is not None:
        cfg.resume_from = args.resume_from
    for key in ('resume_from', 'load_from'):
        if key not in cfg:
            setattr(cfg, key, None)

    distributed = args.launcher != 'none'
    rank, local_rank, world = D.env_world() if distributed else (0, (args.gpu_ids or [0])[0], 1)
    device = torch.device('cuda', local_rank)
    torch.cuda.set_device(device)
    if distributed:
        D.init('nccl', device)
    cfg.gpu_ids = list(range(world)) if distributed else [local_rank]

    os.makedirs(os.path.abspath(cfg.work_dir), exist_ok=True)
    if rank == 0:
        cfg.dump(os.path.join(cfg.work_dir, os.path.basename(args.config)))
    timestamp = time.strftime('%Y%m%d_%H%M%S', time.localtime())
    logger = pkg.get_root_logger(log_file=os.path.join(cfg.work_dir, f'{timestamp}.log'),
                                 log_level=cfg.get('log_level', 'INFO'))
    meta = dict()
    info = env_info()
    dash_line = '-' * 60 + '\n'
    logger.info('Environment info:\n' + dash_line + info + '\n' + dash_line)
    meta['env_info'] = info
    meta['config'] = cfg.pretty_text
    logger.info(f'Distributed training: {distributed}')
    logger.info(f'Config:\n{cfg.pretty_text}')
    if args.seed is not None:
        logger.info(f'Set random seed to {args.seed}, deterministic: {args.deterministic}')
        pkg.set_random_seed(args.seed, deterministic=args.deterministic)
    elif args.deterministic:
        pkg.set_deterministic(True)
    cfg.seed = args.seed
    meta['seed'] = args.seed
    meta['exp_name'] = os.path.basename(args.config)

    model = pkg.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.to(device)
    if args.dtype != 'fp32':
        pkg.wrap_fp16_model(model, torch.float16 if args.dtype == 'fp16' else torch.bfloat16)
    loader = pkg.build_train_loader(cfg.data.train, samples_per_gpu(cfg, logger), seed=args.seed or 0, rank=rank, world=world,
                                    device=device, entropy=args.entropy, prefetch=args.prefetch)
    classes = tuple(loader.dataset.CLASSES)
    if cfg.get('checkpoint_config', None) is not None:
        # the package version and the class names travel in every checkpoint (init_detector reads CLASSES back)
        cfg.checkpoint_config.meta = dict(mmdet_yolov4_amd_version=pkg.__version__, CLASSES=classes)
    model.CLASSES = classes
    pkg.train_detector(model, loader, cfg, distributed=distributed, validate=not args.no_validate, timestamp=timestamp,
                       meta=meta, entropy=args.entropy, prefetch=args.prefetch)
    loader.close()
    if distributed:
        D.finalize()


if __name__ == '__main__':
    main()
