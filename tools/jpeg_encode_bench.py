#!/usr/bin/env python
"""The JPEG encoder, measured: ``imencode`` on the device against Pillow (libjpeg-turbo) on the host, and a validation
pass with and without ``out_dir``.

    python tools/jpeg_encode_bench.py [--passes 7] [--counts 32,256] [--size 480x640] [--images 320] [--batch 32]
                                      [--only encode,val] [--json PATH]

Everything runs in one process.  The forms that are compared alternate, after one warming pass of each, and every figure
is the median with min / max over ``--passes`` passes (at least 7).  A time is a host clock around work that ends in a
device synchronise, but for the stages, which are device events around each call.

  * ``encode``: N generated 480x640 pictures (``tools/test_loader_bench.py``'s) already on the device, quality 95, 4:2:0:
    ``imencode`` end to end; its parts -- stage 1 and stage 2 by device events, the read-back (the counts, the gather of
    the scan bytes on the device and their pinned copy), the headers -- and the file writes (``imwrite``'s thread pool)
    into a temporary directory.  Against Pillow's encode of the same pixels from host arrays on 1 and on 16 threads (the stand-in for ``cv2.imwrite``, which is what
    ``mmcv.imwrite`` costs); skipped by name where Pillow is missing.  The files of both are compared byte for byte.
  * ``val``: YOLOv4-S at 416 in fp16 over ``--images`` files at ``--batch`` (the set of ``tools/test_loader_bench.py``):
    ``single_gpu_test`` with and without ``out_dir``.

There is no pass mark.  Needs the GPU; Pillow for the comparison and for ``val``'s files.  Prints ONE JSON line."""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from test_loader_bench import alternate, make_set, picture, stats, val_block      # noqa: E402


def bench_encode(pkg, torch, a, dev, n, h, w, have_pillow):
    from mmdet_yolov4_amd import image_io as io_
    rng = np.random.default_rng(1)
    host = [picture(rng, i, h, w) for i in range(n)]                 # R G B for Pillow
    imgs = [torch.from_numpy(x).to(dev) for x in host]
    shapes = [tuple(x.shape) for x in host]
    row = dict(images=n, quality=95, subsampling='420')

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    files = pkg.imencode(imgs, channel_order='rgb')
    row['file_bytes'] = round(sum(len(f) for f in files) / n)

    # the parts, over pixels placed once
    et = io_.EncodeTable(shapes)
    pixels = torch.empty(et.pixel_bytes, dtype=torch.uint8, device=dev)
    for t, x in zip(et.table, imgs):
        pixels[int(t.src_off):int(t.src_off) + x.numel()] = x.reshape(-1)
    row['work_megabytes'] = round(et.work_bytes / 1e6, 1)
    row['out_megabytes'] = round(et.out_bytes / 1e6, 1)
    row['read_back_megabytes'] = round(sum(len(f) for f in files) / 1e6, 1)
    parts = {k: [] for k in ('stage1', 'stage2', 'readback', 'headers', 'write')}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f'{i:05d}.jpg') for i in range(n)]

        def once(record):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            coef, work, out, sizes = io_.encode_stages(et, pixels, 'rgb', stages=1)
            ev[1].record()
            coef, work, out, sizes = io_.encode_stages(et, pixels, 'rgb', coef=coef, stages=2)
            ev[2].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts = sizes.cpu().numpy()                 # the steps of image_io._read_back, timed apart
            dense = torch.cat([out[int(t.out_off):int(t.out_off) + int(c)] for t, c in zip(et.table, counts)])
            got = torch.empty(dense.numel(), dtype=torch.uint8, pin_memory=True)
            got.copy_(dense)
            t1 = time.perf_counter()
            made = et.files(got.numpy(), counts, np.concatenate([[0], np.cumsum(counts)[:-1]]))
            t2 = time.perf_counter()
            io_._write_files(made, paths, False)
            t3 = time.perf_counter()
            if record:
                for k, v in zip(parts, (ev[0].elapsed_time(ev[1]) / 1e3, ev[1].elapsed_time(ev[2]) / 1e3, t1 - t0, t2 - t1,
                                        t3 - t2)):
                    parts[k].append(v)
            return made
        assert once(False) == files
        for _ in range(a.passes):
            once(True)
    for k, v in parts.items():
        row[k + '_ms'] = stats(v)

    forms = {'device': lambda: sync_time(lambda: pkg.imencode(imgs, channel_order='rgb'))[0]}
    if have_pillow:
        from PIL import Image

        def pil(x):
            buf = io.BytesIO()
            Image.fromarray(x).save(buf, 'JPEG', quality=95, subsampling=2)
            return buf.getvalue()

        def threads(k):
            def run():
                t0 = time.perf_counter()
                if k == 1:
                    out = [pil(x) for x in host]
                else:
                    with ThreadPoolExecutor(max_workers=k) as pool:
                        out = list(pool.map(pil, host))
                run.files = out
                return time.perf_counter() - t0
            return run
        forms['pillow_1_thread'], forms['pillow_16_threads'] = threads(1), threads(16)
    else:
        row['pillow'] = 'skipped: Pillow is not installed'
    rec = alternate(forms, a.passes)
    for k, v in rec.items():
        row[k + '_ms'] = stats(v)
        row[k + '_images_per_s'] = round(n / float(np.median(v)))
    if have_pillow:
        row['equal_to_pillow'] = forms['pillow_1_thread'].files == files and forms['pillow_16_threads'].files == files
        row['device_over_pillow_16'] = round(row['device_ms']['median'] / row['pillow_16_threads_ms']['median'], 3)
    print('encode  ', json.dumps(row), flush=True)
    return row


def bench_val(pkg, torch, a, dev, cfg):
    import bench
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg('yolov4s'))
    det.init_weights()
    det.eval().to(dev)
    pkg.wrap_fp16_model(det, torch.float16)
    loader = pkg.build_test_loader(cfg, a.batch, device=dev, prefetch=1)
    first = next(iter(loader))
    shape = first['img'][0].shape
    plan = det.compile(shape[0], shape[2], shape[3], device=dev, rescale=True, graph=False)
    bench.init_head(det, plan, first['img'][0].clone(), 2000.0)
    with tempfile.TemporaryDirectory() as out_dir:
        def run(**kw):
            def f():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pkg.single_gpu_test(det, loader, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            return f
        rec = alternate(dict(plain=run(), out_dir=run(out_dir=out_dir, show_score_thr=0.3)), a.passes)
        written = len(os.listdir(os.path.join(out_dir, '')))
    loader.close()
    row = dict(model='yolov4s', dtype='fp16', images=a.images, batch=a.batch, files_written=written,
               plain_ms=stats(rec['plain']), out_dir_ms=stats(rec['out_dir']))
    row['out_dir_over_plain'] = round(row['out_dir_ms']['median'] / row['plain_ms']['median'], 3)
    row['extra_ms_per_image'] = round((row['out_dir_ms']['median'] - row['plain_ms']['median']) / a.images, 3)
    print('val     ', json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--counts', default='32,256')
    ap.add_argument('--size', default='480x640')
    ap.add_argument('--images', type=int, default=320)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--only', default='encode,val')
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    if a.passes < 7:
        sys.exit('jpeg_encode_bench: at least 7 passes')
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd.datasets import COCO_CLASSES
    if not torch.cuda.is_available():
        sys.exit('jpeg_encode_bench: no GPU')
    dev = torch.device('cuda', 0)
    h, w = (int(v) for v in a.size.split('x'))
    only = set(a.only.split(','))
    line = dict(tool='jpeg_encode_bench', device=torch.cuda.get_device_name(0), passes=a.passes, size=a.size)
    if 'encode' in only:
        line['encode'] = [bench_encode(pkg, torch, a, dev, int(n), h, w, have_pillow) for n in a.counts.split(',')]
    if 'val' in only:
        if not have_pillow:
            line['val'] = 'skipped: Pillow is needed to make the image files'
        else:
            with tempfile.TemporaryDirectory() as root:
                make_set(root, a.images, h, w, COCO_CLASSES)
                cfg = dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', pipeline=val_block(416))
                line['val'] = bench_val(pkg, torch, a, dev, cfg)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
