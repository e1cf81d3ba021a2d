"""The training loader on a directory of generated JPEGs: files/s and batches/s per entropy mode and ``prefetch``.

    python tools/loader_bench.py [--images 128] [--batch 16] [--epochs 3] [--recipe mosaic|v3] [--size 480x640]
                                 [--step-ms 0] [--json PATH]

Writes ``--images`` files of ``--size`` (4:2:0, quality 90, the shape of a COCO file; made with Pillow) and a COCO
annotation file with a few boxes each into a temporary directory, then measures, per entropy mode (``host``, ``device``,
``device_sync``) and ``prefetch`` (0, 1):
  * one epoch of ``build_train_loader`` end to end, host clock around a device synchronise per batch: the median over
    ``--epochs`` epochs after one warm-up epoch, and the spread; files/s counts the files decoded (4 per sample for the
    mosaic recipe);
  * the host seconds per phase that the loader records (``TrainLoader.times``): index draws, file reads, header parse
    plus host half (the Huffman decodes with ``host``), the decode call, the pipeline call.  With ``prefetch=1`` reads
    and host half run on the worker thread, so their sum may exceed the epoch's wall time;
  * ``--step-ms``: a sleep per batch standing in for the train step, which is what ``prefetch=1`` overlaps with;
and, for comparison, the same batches composed by hand from the loader's recorded draws: ``imread`` of each sample's
files (one call per sample) and the fused pipeline.  The recipes are the reference's at full size: mosaic 640 (tiles 640,
canvas 1920, crop 1280) and YOLOv3 mstrain 320..608.  There is no pass mark.  Needs the GPU and Pillow.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOSAIC = [
    dict(type='MosaicPipeline',
         individual_pipeline=[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
                              dict(type='Resize', img_scale=(640, 640), keep_ratio=True)], pad_val=114),
    dict(type='Albu', bbox_params=dict(type='BboxParams', format='pascal_voc', label_fields=['gt_labels'], min_area=4,
                                       min_visibility=0.2, filter_lost_elements=True),
         transforms=[dict(type='PadIfNeeded', min_height=1920, min_width=1920, border_mode=0, value=[114, 114, 114]),
                     dict(type='RandomCrop', width=1280, height=1280),
                     dict(type='RandomScale', scale_limit=0.5, interpolation=1),
                     dict(type='CenterCrop', width=640, height=640), dict(type='HorizontalFlip', p=0.5)]),
    dict(type='HueSaturationValueJitter', hue_ratio=0.015, saturation_ratio=0.7, value_ratio=0.4),
    dict(type='GtBBoxesFilter', min_size=2, max_aspect_ratio=20),
    dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
    dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
V3 = [
    dict(type='LoadImageFromFile', to_float32=True), dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion'), dict(type='Expand', mean=[0, 0, 0], to_rgb=True, ratio_range=(1, 2)),
    dict(type='MinIoURandomCrop', min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9), min_crop_size=0.3),
    dict(type='Resize', img_scale=[(320, 320), (608, 608)], keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True), dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def make_set(root, n, h, w):
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w]
    images, anns = [], []
    os.makedirs(os.path.join(root, 'img'))
    for i in range(n):
        hh, ww = (h, w) if i % 4 else (w, h)      # a quarter portrait: both groups of the sampler
        y, x = (yy, xx) if i % 4 else (xx.T, yy.T)
        base = np.stack([127 + 100 * np.sin(x / (23.0 + i % 17) + c) * np.cos(y / (31.0 + i % 13) - c) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, (hh, ww, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2)
        with open(os.path.join(root, 'img', f'{i:06d}.jpg'), 'wb') as f:
            f.write(buf.getvalue())
        images.append(dict(id=i, width=ww, height=hh, file_name=f'{i:06d}.jpg'))
        for k in range(4):
            bw, bh = int(rng.integers(20, ww // 2)), int(rng.integers(20, hh // 2))
            bx, by = int(rng.integers(0, ww - bw)), int(rng.integers(0, hh - bh))
            anns.append(dict(id=4 * i + k, image_id=i, category_id=1 + k % 2, bbox=[bx, by, bw, bh], area=bw * bh, iscrowd=0))
    with open(os.path.join(root, 'ann.json'), 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name='a'), dict(id=2, name='b')]), f)
    return sum(os.path.getsize(os.path.join(root, 'img', im['file_name'])) for im in images) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=128)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--recipe', default='mosaic', choices=('mosaic', 'v3'))
    ap.add_argument('--size', default='480x640')
    ap.add_argument('--step-ms', type=float, default=0.0)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.exit('loader_bench: Pillow is needed to make the image files')
    import torch
    import mmdet_yolov4_amd as pkg
    if not torch.cuda.is_available():
        sys.exit('loader_bench: no GPU')
    h, w = (int(v) for v in args.size.split('x'))
    pipeline = MOSAIC if args.recipe == 'mosaic' else V3
    per = 4 if args.recipe == 'mosaic' else 1
    result = dict(device=torch.cuda.get_device_name(0), recipe=args.recipe, images=args.images, batch=args.batch,
                  size=args.size, step_ms=args.step_ms, rows=[])
    with tempfile.TemporaryDirectory() as root:
        result['file_bytes'] = make_set(root, args.images, h, w)
        cfg = dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', classes=('a', 'b'),
                   pipeline=pipeline)

        def epoch(loader, record=None):
            loader.set_epoch(0)
            t0 = time.perf_counter()
            for data in loader:
                torch.cuda.synchronize()
                if record is not None:
                    record.append(loader.draws)
                if args.step_ms:
                    time.sleep(args.step_ms / 1e3)
            return time.perf_counter() - t0

        draws = []
        for entropy in ('host', 'device', 'device_sync'):
            for prefetch in (0, 1):
                loader = pkg.build_train_loader(cfg, args.batch, seed=0, entropy=entropy, prefetch=prefetch)
                epoch(loader, draws if not draws else None)                      # warm-up
                secs = [epoch(loader) for _ in range(args.epochs)]
                med = statistics.median(secs)
                nb = len(loader)
                row = dict(entropy=entropy, prefetch=prefetch, epoch_s=med, spread_s=(min(secs), max(secs)),
                           batches_per_s=nb / med, files_per_s=nb * args.batch * per / med,
                           phase_ms_per_batch={k: 1e3 * v / nb for k, v in loader.times.items()})
                result['rows'].append(row)
                print(f"{entropy:12s} prefetch={prefetch}  {row['batches_per_s']:8.1f} batches/s  {row['files_per_s']:9.0f} files/s"
                      f"  epoch {1e3 * med:8.1f} ms ({1e3 * min(secs):.1f} .. {1e3 * max(secs):.1f})  per batch: "
                      + '  '.join(f'{k} {v:.2f} ms' for k, v in row['phase_ms_per_batch'].items()))
                loader.close()
        # the same batches by hand: imread per sample, then the pipeline with the recorded parameters
        loader = pkg.build_train_loader(cfg, args.batch, seed=0)
        ds = loader.dataset

        def by_hand():
            t0 = time.perf_counter()
            for d in draws:
                samples = []
                for group in d['sources']:
                    imgs = pkg.imread([os.path.join(ds.img_prefix, ds.data_infos[j]['filename']) for j in group],
                                      orientation=True)
                    tr = [(im, a['bboxes'], a['labels']) for im, a in zip(imgs, (ds.get_ann_info(j) for j in group))]
                    samples.append(tuple(tr) if per == 4 else tr[0])
                loader.pipeline(samples, params=d['params'])
                torch.cuda.synchronize()
                if args.step_ms:
                    time.sleep(args.step_ms / 1e3)
            return time.perf_counter() - t0

        by_hand()
        secs = [by_hand() for _ in range(args.epochs)]
        med = statistics.median(secs)
        result['by_hand'] = dict(epoch_s=med, spread_s=(min(secs), max(secs)), batches_per_s=len(draws) / med,
                                 files_per_s=len(draws) * args.batch * per / med)
        print(f"by hand (imread per sample, host)  {len(draws) / med:8.1f} batches/s  {len(draws) * args.batch * per / med:9.0f} "
              f"files/s  epoch {1e3 * med:8.1f} ms ({1e3 * min(secs):.1f} .. {1e3 * max(secs):.1f})")
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(device=result['device'], file_bytes=result['file_bytes'])))


if __name__ == '__main__':
    main()
