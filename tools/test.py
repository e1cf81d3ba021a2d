#!/usr/bin/env python
"""Test (and evaluate) a checkpoint from a config file, the way the reference's ``tools/test.py`` does:
    python tools/test.py <config.py> out/latest.pth --eval bbox
    python tools/test.py <config.py> out/latest.pth --format-only --eval-options jsonfile_prefix=out/results
    python tools/test.py <config.py> out/latest.pth --out results.pkl --show-dir out/painted
When nothing but ``--eval`` is asked and the dataset takes it, the result table stays on the GPU and is scored there
(``single_gpu_test(flat=True)``); ``--out``, ``--format-only`` and ``--show-dir`` take the per-image lists."""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVAL_HOOK_KEYS = ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule')


def parse_args(argv=None):
    from mmdet_yolov4_amd.registry import DictAction
    parser = argparse.ArgumentParser(description='Test (and evaluate) a detector')
    parser.add_argument('config', help='test config file path')
    parser.add_argument('checkpoint', help='checkpoint file')
    parser.add_argument('--out', help='output result file in pickle format')
    parser.add_argument('--fuse-conv-bn', action='store_true',
                        help='accepted for compatibility: the inference plans fold BatchNorm into the convs anyway')
    parser.add_argument('--format-only', action='store_true',
                        help='write the results in the form a test server takes (format_results), without evaluating')
    parser.add_argument('--eval', type=str, nargs='+', help='evaluation metrics, e.g. "bbox", "fast-bbox", "proposal_fast"')
    parser.add_argument('--show', action='store_true', help='refused: there is no display; use --show-dir')
    parser.add_argument('--show-dir', help='directory where painted images will be saved')
    parser.add_argument('--show-score-thr', type=float, default=0.3, help='score threshold (default: 0.3)')
    parser.add_argument('--gpu-collect', action='store_true', help="gather the ranks' results on the GPUs")
    parser.add_argument('--tmpdir', help='accepted and unused: the ranks\' results are gathered by collectives')
    parser.add_argument('--cfg-options', nargs='+', action=DictAction, help='override settings of the config: key=value')
    parser.add_argument('--eval-options', nargs='+', action=DictAction,
                        help='keyword arguments of dataset.evaluate() / format_results(): key=value')
    parser.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none', help='job launcher')
    parser.add_argument('--local_rank', type=int, default=0)
    parser.add_argument('--dtype', choices=['fp32', 'fp16', 'bf16'], default='fp32',
                        help='activation / conv operand type of the inference plans')
    args = parser.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    return args


def check_args(args):
    """The reference's argument checks (``tools/test.py:104-114``) and what this tool refuses by name."""
    assert args.out or args.eval or args.format_only or args.show or args.show_dir, \
        'nothing to do: name at least one operation among --out, --eval, --format-only and --show-dir'
    if args.eval and args.format_only:
        raise ValueError('--eval and --format-only cannot be both given: the first scores, the second only writes')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise ValueError(f'--out {args.out}: the result file is a pickle and must end in .pkl or .pickle')
    if args.show:
        raise NotImplementedError('--show is not built: there is no display; --show-dir writes the painted images')
    if args.launcher in ('slurm', 'mpi'):
        raise NotImplementedError(f"--launcher {args.launcher} is not built: 'none' and 'pytorch' are")
    if args.show_dir and args.launcher != 'none':
        raise NotImplementedError('--show-dir with a launcher is not built (multi_gpu_test paints nothing, as in the '
                                  'reference)')


def main(argv=None):
    args = parse_args(argv)
    check_args(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/test.py: no GPU is visible (torch.cuda.is_available() is False); nothing was built')
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import dist as D
    from mmdet_yolov4_amd.apis import load_weights
    from mmdet_yolov4_amd.registry import Config

    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    cfg.model.pretrained = None
    cfg.model.train_cfg = None
    distributed = args.launcher != 'none'
    rank, local_rank, world = D.env_world() if distributed else (0, 0, 1)
    device = torch.device('cuda', local_rank)
    torch.cuda.set_device(device)
    if distributed:
        D.init('nccl', device)

    # (the block's own samples_per_gpu is the batch, else 1: tools/test.py:138-141)
    loader = pkg.build_test_loader(cfg.data.test, rank=rank, world=world, device=device)
    dataset = loader.dataset
    model = pkg.build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
    checkpoint = load_weights(model, args.checkpoint, map_location='cpu')
    model.CLASSES = checkpoint.get('meta', {}).get('CLASSES', dataset.CLASSES)
    model.to(device).eval()
    dtype = {'fp32': None, 'fp16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    if dtype is None and cfg.get('fp16', None) is not None:
        dtype = torch.float16
    if dtype is not None:
        pkg.wrap_fp16_model(model, dtype)

    lists_wanted = bool(args.out or args.format_only or args.show_dir)
    flat = not lists_wanted and bool(getattr(dataset, 'accepts_flat', False))
    if args.show_dir:
        os.makedirs(args.show_dir, exist_ok=True)
    if not distributed:
        outputs = pkg.single_gpu_test(model, loader, flat=flat, out_dir=args.show_dir, show_score_thr=args.show_score_thr)
    else:
        outputs = pkg.multi_gpu_test(model, loader, gpu_collect=args.gpu_collect or D.backend_name() == 'nccl', flat=flat)
    loader.close()

    if rank == 0:
        if args.out:
            print(f'\nwriting results to {args.out}')
            with open(args.out, 'wb') as f:
                pickle.dump(outputs, f)
        kwargs = {} if args.eval_options is None else args.eval_options
        if args.format_only:
            dataset.format_results(outputs, **kwargs)
        if args.eval:
            eval_kwargs = dict(cfg.get('evaluation', {}) or {})
            for key in EVAL_HOOK_KEYS:                 # (what configures the EvalHook, not the scoring)
                eval_kwargs.pop(key, None)
            eval_kwargs.update(dict(metric=args.eval, **kwargs))
            print(dataset.evaluate(outputs, **eval_kwargs))
    if distributed:
        D.finalize()


if __name__ == '__main__':
    main()
