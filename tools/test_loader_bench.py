#!/usr/bin/env python
"""The test side's input path, measured: the one-launch batched letterbox against the per-image path, the batched
kernel on its own, the test loader from files, and a validation pass from files against the same pass from pre-built
device batches.

    python tools/test_loader_bench.py [--passes 7] [--calls 10] [--images 320] [--batch 32] [--size 480x640]
                                      [--only pipeline,kernel,loader,val] [--json PATH]

Everything runs in one process.  Where two forms are compared they alternate, after one warming pass of each, and every
figure is the median with min / max over ``--passes`` passes (at least 7); a time is a host clock around work that ends
in a device synchronise, but for the kernel's own time, which is device events around ``--calls`` launches.

  * ``pipeline``: one ``FusedTestPipeline`` call, ``batched=True`` against ``batched=False`` (one launch an image into a
    zeroed batch), per call over ``--calls`` calls a pass: 32 sources of 480x640 to a 640 canvas and 256 to a 416 canvas,
    a quarter of them portrait so that the batch is ragged; device inputs (what the loader passes) and numpy inputs.
  * ``kernel``: ``yv4_letterbox_u8_batch`` alone over a table made once: device time, the bytes it reads and writes
    (source pixels once, every destination float once) over that time, and the same for a device-to-device copy of the
    destination's size (bytes read plus written), as a share.
  * ``loader``: ``build_test_loader`` over Pillow-made files (4:2:0, quality 90): files/s and the host milliseconds per
    batch by phase (``TestLoader.times``), per entropy mode and ``prefetch``, with the batched and the per-image pipeline.
  * ``val``: YOLOv4-S at 416 in fp16, ``--images`` images at ``--batch``: the loader, ``single_gpu_test(flat=True)`` and
    ``evaluate`` from files (``prefetch=1``; entropy ``host`` and ``device_sync``), against the same loop and scoring over
    the loader's batches kept on the device.

There is no pass mark.  Needs the GPU and Pillow.  Prints ONE JSON line."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NORM = dict(mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True)


def val_block(scale):
    """The test_pipeline block of configs/yolov4/*.py at ``scale``."""
    return [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(scale, scale), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32),
                             dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                             dict(type='Collect', keys=['img'])])]


def picture(rng, i, h, w):
    """A smooth picture with some noise, landscape but every fourth one portrait."""
    hh, ww = (h, w) if i % 4 else (w, h)
    y, x = np.mgrid[0:hh, 0:ww]
    base = np.stack([127 + 100 * np.sin(x / (23.0 + i % 17) + c) * np.cos(y / (31.0 + i % 13) - c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 12, (hh, ww, 3)), 0, 255).astype(np.uint8)


def make_set(root, n, h, w, names):
    from PIL import Image
    rng = np.random.default_rng(0)
    images, anns = [], []
    os.makedirs(os.path.join(root, 'img'))
    for i in range(n):
        img = picture(rng, i, h, w)
        hh, ww = img.shape[:2]
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2)
        with open(os.path.join(root, 'img', f'{i:06d}.jpg'), 'wb') as f:
            f.write(buf.getvalue())
        images.append(dict(id=i, width=ww, height=hh, file_name=f'{i:06d}.jpg'))
        for k in range(7):
            bw, bh = int(rng.integers(20, ww // 2)), int(rng.integers(20, hh // 2))
            bx, by = int(rng.integers(0, ww - bw)), int(rng.integers(0, hh - bh))
            anns.append(dict(id=7 * i + k + 1, image_id=i, category_id=1 + int(rng.integers(0, len(names))),
                             bbox=[bx, by, bw, bh], area=bw * bh, iscrowd=int(k == 6)))
    with open(os.path.join(root, 'ann.json'), 'w') as f:
        json.dump(dict(images=images, annotations=anns,
                       categories=[dict(id=c + 1, name=n) for c, n in enumerate(names)]), f)
    return sum(os.path.getsize(os.path.join(root, 'img', im['file_name'])) for im in images) / n


def stats(xs, scale=1e3, digits=3):
    return dict(median=round(float(np.median(xs)) * scale, digits), min=round(float(np.min(xs)) * scale, digits),
                max=round(float(np.max(xs)) * scale, digits))


def alternate(forms, passes):
    """``forms``: {name: function -> seconds}.  One warming pass of each, then ``passes`` rounds in which they alternate."""
    for f in forms.values():
        f()
    rec = {k: [] for k in forms}
    for _ in range(passes):
        for k, f in forms.items():
            rec[k].append(f())
    return rec


def bench_pipeline(pkg, torch, a, dev, h, w):
    out = []
    rng = np.random.default_rng(1)
    for batch, scale in ((32, 640), (256, 416)):
        host = [picture(rng, i, h, w) for i in range(batch)]
        for kind, imgs in (('device', [torch.from_numpy(x).to(dev) for x in host]), ('numpy', host)):
            pipes = {name: pkg.FusedTestPipeline(img_scale=(scale, scale), device=dev, batched=b, **NORM)
                     for name, b in (('batched', True), ('per_image', False))}

            def call(pipe):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    pipe(imgs)
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.calls
            x, y = pipes['batched'](imgs)[0], pipes['per_image'](imgs)[0]
            if not torch.equal(x, y):
                raise SystemExit('the batched and the per-image pipeline disagree')
            rec = alternate({k: (lambda p=p: call(p)) for k, p in pipes.items()}, a.passes)
            row = dict(batch=batch, scale=scale, canvas=list(x.shape[2:]), inputs=kind,
                       batched_ms=stats(rec['batched']), per_image_ms=stats(rec['per_image']))
            row['batched_over_per_image'] = round(row['batched_ms']['median'] / row['per_image_ms']['median'], 3)
            b, p = row['batched_ms'], row['per_image_ms']
            # not slower: the median is not above, or the min-max ranges overlap
            row['not_slower'] = b['median'] <= p['median'] or (b['min'] <= p['max'] and p['min'] <= b['max'])
            print(f"pipeline batch {batch:3d} -> {scale} ({kind:6s})  batched {row['batched_ms']}  per image "
                  f"{row['per_image_ms']} ms a call", flush=True)
            out.append(row)
    return out


def bench_kernel(pkg, torch, a, dev, h, w):
    from mmdet_yolov4_amd import _lib
    out = []
    rng = np.random.default_rng(2)
    for batch, scale in ((32, 640), (256, 416)):
        imgs = [torch.from_numpy(picture(rng, i, h, w)).to(dev) for i in range(batch)]
        pipe = pkg.FusedTestPipeline(img_scale=(scale, scale), device=dev, **NORM)
        geo = [pipe._geometry(im.shape[0], im.shape[1], (scale, scale)) for im in imgs]
        H, W = max(g[4] for g in geo), max(g[5] for g in geo)
        table = (_lib.LetterboxSlot * batch)()
        for i, (t, im, (sh, sw, nh, nw, hp, wp)) in enumerate(zip(table, imgs, geo)):
            t.src, t.src_h, t.src_w, t.src_pitch = im.data_ptr(), sh, sw, 3 * sw
            t.inv_sx, t.inv_sy, t.dst_off = 1.0 / (nw / sw), 1.0 / (nh / sh), i * 3 * H * W
            t.new_h, t.new_w, t.pad_h, t.pad_w, t.H, t.W, t.flip = nh, nw, hp, wp, H, W, 0
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        total = batch * 3 * H * W
        dst, other = torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.float32, device=dev)
        stream = pkg.ops.stream_ptr()

        def launch():
            _lib.check(_lib.lib().yv4_letterbox_u8_batch(
                table, table_dev.data_ptr(), batch, dst.data_ptr(), total, pipe.mean.ctypes.data_as(C.c_void_p),
                pipe.std.ctypes.data_as(C.c_void_p), 1, 0, 1, stream), 'yv4_letterbox_u8_batch')

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 1e3 / a.calls
        rec = alternate(dict(kernel=lambda: timed(launch), copy=lambda: timed(lambda: other.copy_(dst))), a.passes)
        moved = 4 * total + sum(3 * g[0] * g[1] for g in geo)
        k, c = float(np.median(rec['kernel'])), float(np.median(rec['copy']))
        row = dict(batch=batch, scale=scale, canvas=[H, W], kernel_us=stats(rec['kernel'], 1e6, 1),
                   copy_us=stats(rec['copy'], 1e6, 1), kernel_bytes=moved, kernel_GBps=round(moved / k / 1e9, 1),
                   copy_GBps=round(8 * total / c / 1e9, 1))
        row['share_of_copy_rate'] = round(row['kernel_GBps'] / row['copy_GBps'], 3)
        print(f"kernel   batch {batch:3d} -> {scale}  {row['kernel_us']} us  {row['kernel_GBps']} GB/s;  copy of the "
              f"destination {row['copy_us']} us  {row['copy_GBps']} GB/s", flush=True)
        out.append(row)
    return out


def bench_loader(pkg, torch, a, dev, cfg):
    out = []
    for entropy in ('host', 'device', 'device_sync'):
        for prefetch in (0, 1):
            loaders = {name: pkg.build_test_loader(cfg, a.batch, device=dev, entropy=entropy, prefetch=prefetch, batched=b)
                       for name, b in (('batched', True), ('per_image', False))}
            phases = {}

            def one(name):
                ld = loaders[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for data in ld:
                    torch.cuda.synchronize()
                phases[name] = {k: round(1e3 * v / len(ld), 3) for k, v in ld.times.items()}
                return time.perf_counter() - t0
            rec = alternate({k: (lambda k=k: one(k)) for k in loaders}, a.passes)
            for name, ld in loaders.items():
                med = float(np.median(rec[name]))
                row = dict(entropy=entropy, prefetch=prefetch, pipeline=name, pass_ms=stats(rec[name]),
                           files_per_s=round(a.images / med), phase_ms_per_batch=phases[name])
                print(f"loader   {entropy:12s} prefetch={prefetch} {name:9s} {row['files_per_s']:7d} files/s  pass "
                      f"{row['pass_ms']} ms  per batch {row['phase_ms_per_batch']}", flush=True)
                out.append(row)
                ld.close()
    return out


def bench_val(pkg, torch, a, dev, cfg):
    import bench
    torch.manual_seed(0)
    det = pkg.build_detector(bench.model_cfg('yolov4s'))
    det.init_weights()
    det.eval().to(dev)
    pkg.wrap_fp16_model(det, torch.float16)
    loaders = {f'files_{e}': pkg.build_test_loader(cfg, a.batch, device=dev, entropy=e, prefetch=1)
               for e in ('host', 'device_sync')}
    first = loaders['files_host']
    kept = [dict(img=[b.clone() for b in d['img']], img_metas=d['img_metas']) for d in first]
    shape = kept[0]['img'][0].shape
    plan = det.compile(shape[0], shape[2], shape[3], device=dev, rescale=True, graph=False)
    per_img = bench.init_head(det, plan, kept[0]['img'][0], 2000.0)

    class Kept(list):
        dataset = first.dataset

    def run(ld):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pkg.single_gpu_test(det, ld, flat=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):      # (the summary table)
            score = ld.dataset.evaluate(res, metric='bbox', logger='silent')
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0, t2 - t1, t2 - t0), score, int(res[0].shape[0])
    forms = dict(loaders, kept=Kept(kept))
    warm = {k: run(ld) for k, ld in forms.items()}
    for k in loaders:
        if warm[k][1:] != warm['kept'][1:]:
            raise SystemExit(f"the pass from files ({k}) and the pass from kept batches disagree: {warm[k][1:]} != "
                             f"{warm['kept'][1:]}")
    rec = {k: [] for k in forms}
    for _ in range(a.passes):
        for k, ld in forms.items():
            rec[k].append(run(ld)[0])
    row = dict(model='yolov4s', dtype='fp16', images=a.images, batch=a.batch, prefetch=1,
               canvases=sorted({tuple(d['img'][0].shape[2:]) for d in kept}), candidates_per_image=round(per_img, 1),
               rows=warm['kept'][2], bbox_mAP=warm['kept'][1].get('bbox_mAP'))
    for k in forms:
        t = np.asarray(rec[k])
        row[k] = dict(loop_ms=stats(t[:, 0]), scoring_ms=stats(t[:, 1]), total_ms=stats(t[:, 2]))
        print(f"val      {k:18s} total {row[k]['total_ms']} ms  loop {row[k]['loop_ms']}  scoring {row[k]['scoring_ms']}",
              flush=True)
    for k, ld in loaders.items():
        row[k + '_over_kept_total'] = round(row[k]['total_ms']['median'] / row['kept']['total_ms']['median'], 3)
        ld.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--images', type=int, default=320)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', default='480x640')
    ap.add_argument('--only', default='pipeline,kernel,loader,val')
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    if a.passes < 7:
        sys.exit('test_loader_bench: at least 7 passes')
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.exit('test_loader_bench: Pillow is needed to make the image files')
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd.datasets import COCO_CLASSES
    if not torch.cuda.is_available():
        sys.exit('test_loader_bench: no GPU')
    dev = torch.device('cuda', 0)
    h, w = (int(v) for v in a.size.split('x'))
    only = set(a.only.split(','))
    line = dict(tool='test_loader_bench', device=torch.cuda.get_device_name(0), passes=a.passes, calls=a.calls, size=a.size)
    if 'pipeline' in only:
        line['pipeline'] = bench_pipeline(pkg, torch, a, dev, h, w)
    if 'kernel' in only:
        line['kernel'] = bench_kernel(pkg, torch, a, dev, h, w)
    if only & {'loader', 'val'}:
        with tempfile.TemporaryDirectory() as root:
            line['file_bytes'] = round(make_set(root, a.images, h, w, COCO_CLASSES))
            cfg = dict(type='CocoDataset', ann_file='ann.json', data_root=root, img_prefix='img/', pipeline=val_block(416))
            if 'loader' in only:
                line['loader'] = bench_loader(pkg, torch, a, dev, cfg)
            if 'val' in only:
                line['val'] = bench_val(pkg, torch, a, dev, cfg)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
