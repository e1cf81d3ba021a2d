#!/usr/bin/env python
"""What the config-file layer costs a training run: images/s of one epoch from generated image files
(``tools/loader_bench.py``'s generator, the mosaic recipe at the model's size)
  * through ``train_detector`` with ``IterTimerHook`` and ``TextLoggerHook(interval=50)`` -- what ``tools/train.py`` runs,
  * through the same hooks assembled by hand on ``Runner`` without the timer and the logger,
both timed over the epochs after the first (which compiles plans and tunes tiles), the device drained at epoch boundaries
only.  ``tools/train_bench.py --model M --batch B --size S --dtype D`` gives the step on a batch kept on the device.
    python tools/train_api_bench.py --model yolov4s --size 416 --dtype fp16 --batch 32 --images 512"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def mosaic(size):
    return [
        dict(type='MosaicPipeline',
             individual_pipeline=[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                                  dict(type='Resize', img_scale=(size, size), keep_ratio=True)], pad_val=114),
        dict(type='Albu', bbox_params=dict(type='BboxParams', format='pascal_voc', label_fields=['gt_labels'], min_area=4,
                                           min_visibility=0.2, filter_lost_elements=True),
             transforms=[dict(type='PadIfNeeded', min_height=3 * size, min_width=3 * size, border_mode=0,
                              value=[114, 114, 114]),
                         dict(type='RandomCrop', width=2 * size, height=2 * size),
                         dict(type='RandomScale', scale_limit=0.5, interpolation=1),
                         dict(type='CenterCrop', width=size, height=size), dict(type='HorizontalFlip', p=0.5)]),
        dict(type='HueSaturationValueJitter', hue_ratio=0.015, saturation_ratio=0.7, value_ratio=0.4),
        dict(type='GtBBoxesFilter', min_size=2, max_aspect_ratio=20),
        dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
        dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='yolov4s')
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--dtype', default='fp16', choices=['fp32', 'fp16', 'bf16'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--images', type=int, default=512)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--interval', type=int, default=50)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('train_api_bench: no GPU')
    import bench
    import loader_bench
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import hooks as H
    from mmdet_yolov4_amd.optim import build_optimizer
    from mmdet_yolov4_amd.registry import Config
    dev = torch.device('cuda', 0)
    dtype = {'fp32': None, 'fp16': torch.float16, 'bf16': torch.bfloat16}[a.dtype]
    optimizer = dict(type='SGD', lr=0.01, momentum=0.937, weight_decay=0.0005, nesterov=True,
                     paramwise_cfg=dict(bias_decay_mult=0., norm_decay_mult=0.))
    opt_hook = dict(type='Fp16GradAccumulateOptimizerHook', nominal_batch_size=a.batch, loss_scale='dynamic',
                    grad_clip=dict(max_norm=35, norm_type=2))
    ema = dict(type='StateEMAHook', momentum=0.9999, nominal_batch_size=a.batch, warm_up=10000, priority='HIGH')
    warm = dict(type='DetailedLinearWarmUpHook', warmup_iters=10000, priority='NORMAL')

    class EpochClock(H.Hook):
        """Seconds per epoch, the device drained at the epoch's two ends and nowhere else."""

        def __init__(self):
            self.seconds = []

        def before_train_epoch(self, runner):
            torch.cuda.synchronize()
            self.t = time.perf_counter()

        def after_train_epoch(self, runner):
            torch.cuda.synchronize()
            self.seconds.append(time.perf_counter() - self.t)

    def detector():
        torch.manual_seed(0)
        det = pkg.build_detector(bench.model_cfg(a.model))
        det.init_weights()
        det.to(dev)
        if dtype is not None:
            pkg.wrap_fp16_model(det, dtype)
        return det

    with tempfile.TemporaryDirectory() as root:
        loader_bench.make_set(root, a.images, 480, 640)
        train = dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', classes=('a', 'b'),
                     pipeline=mosaic(a.size))
        cfg = Config(dict(data=dict(samples_per_gpu=a.batch, workers_per_gpu=2, train=train), optimizer=optimizer,
                          optimizer_config=opt_hook, lr_config=dict(policy='CosineAnnealing', min_lr_ratio=0.2),
                          custom_hooks=[ema, warm], checkpoint_config=None,
                          log_config=dict(interval=a.interval, hooks=[dict(type='TextLoggerHook')]),
                          runner=dict(type='EpochBasedRunner', max_epochs=a.epochs), workflow=[('train', 1)], load_from=None,
                          resume_from=None, seed=0, work_dir=os.path.join(root, 'work'), log_level='WARNING'))
        rows = {}
        # ---- train_detector: what tools/train.py runs ----
        clock = EpochClock()
        H.HOOKS.register_module(name='TrainApiBenchClock', module=type('TrainApiBenchClock', (H.Hook,), dict(
            before_train_epoch=lambda self, r: clock.before_train_epoch(r),
            after_train_epoch=lambda self, r: clock.after_train_epoch(r))))
        cfg.custom_hooks = [ema, warm, dict(type='TrainApiBenchClock', priority='LOWEST')]
        loader = pkg.build_train_loader(cfg.data.train, a.batch, seed=0, device=dev, prefetch=1)
        runner = pkg.train_detector(detector(), loader, cfg, validate=False, timestamp='bench')
        per_epoch = len(loader) * a.batch
        rows['train_detector'] = [round(per_epoch / s, 1) for s in clock.seconds]
        loader.close()
        del runner
        # ---- the same hooks by hand, no timer, no logger ----
        clock2 = EpochClock()
        det = detector()
        loader = pkg.build_train_loader(cfg.data.train, a.batch, seed=0, device=dev, prefetch=1)
        runner = H.Runner(det, build_optimizer(det, optimizer), max_epochs=a.epochs)
        runner.log_buffer = None
        runner.register_hook(H.CosineAnnealingLrUpdaterHook(min_lr_ratio=0.2), 'VERY_HIGH')
        runner.register_hook_from_cfg(ema)
        runner.register_hook_from_cfg(opt_hook | dict(priority='ABOVE_NORMAL'))
        runner.register_hook(H.DistSamplerSeedHook())
        runner.register_hook_from_cfg(warm)
        runner.register_hook(clock2, 'LOWEST')
        runner.run(loader)
        rows['by_hand'] = [round(per_epoch / s, 1) for s in clock2.seconds]
        loader.close()
    print(json.dumps(dict(metric='images/sec over an epoch from files', model=a.model, size=a.size, dtype=a.dtype,
                          batch=a.batch, images_per_epoch=per_epoch, interval=a.interval, per_epoch=rows,
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
