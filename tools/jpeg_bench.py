"""Phases of the hybrid JPEG decode on 32 images of 480x640, 4:2:0, quality 90 (the shape of a COCO file).

    python tools/jpeg_bench.py [--images 32] [--repeats 5] [--device-batches 32,256] [--json PATH]
                               [--entropy device_sync [--chunk-bytes 64,256,1024] [--max-rounds 8]]

Prints, per phase, the median over ``--repeats`` windows (and the spread):
  * host parse + entropy decode per image on one thread and on 16 threads (files/s),
  * the upload of the pinned staging buffer (table + quantisation tables + coefficients),
  * the two device kernels of ``yv4_jpeg_reconstruct`` by HIP events over a window of back-to-back calls on resident
    buffers, and the bytes/s they achieve against the measured HBM copy rate of the MI355X (6.29 TB/s): bytes are what
    the algorithm moves -- coefficients read (2 B), planes written and read (1 B + 1 B), pixels written (3 B),
  * ``imdecode`` of the batch end to end (host clock around a device synchronise),
  * Pillow's (libjpeg-turbo's) decode of the same files on one thread, as the reference, where Pillow is importable,
  * with ``--device-batches``, per batch size B (the image set repeated to B files) and for the same files re-encoded with
    ``restart_marker_rows=1`` (30 segments per file instead of one): the host side of the device Huffman decode
    (``ScanTables``: parse, segment table, packed tables; one thread), the staging bytes and their upload, HIP events
    around ``yv4_jpeg_entropy_decode_device`` alone and around it plus ``yv4_jpeg_reconstruct`` on resident buffers, and
    ``imdecode`` end to end with ``entropy='device'`` against ``entropy='host'`` on 16 and on 2 threads (2 is one rank's
    share when eight ranks split 16 CPUs).  ``--json`` writes everything measured to a file.
  * with ``--entropy device_sync`` on top of that, in the same process and per ``--chunk-bytes`` value: the chunk and
    workgroup counts, the rounds the batch's chains need to close (from the CPU run of the same core), HIP events around
    ``yv4_jpeg_entropy_decode_device_sync`` alone at ``--max-rounds`` and at 0 rounds (one pass, the sums and nothing
    stored: every multi-chunk image is undecided), the images left undecided, and ``imdecode(entropy='device_sync')`` end
    to end -- next to the one lane per segment kernel and the host paths measured just before.
The images are made with Pillow; without it the tool says so and exits.  There is no pass mark.  Needs the GPU: a
measurement path that finds none fails.
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12      # measured float4 copy rate of the MI355X (8.0e12 is the specification)
THREADS = 16


def make_images(n, h=480, w=640, **kw):
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):      # smooth structure plus texture: ~120 KB per file at quality 90, a detailed photograph
        base = np.stack([127 + 100 * np.sin(xx / (23.0 + i) + c) * np.cos(yy / (31.0 + 2 * i) - c) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2, **kw)
        out.append(buf.getvalue())
    return out


def windows(fn, repeats):
    """median and (min, max) of ``fn()`` -- seconds per window -- after one warm-up window"""
    fn()
    t = [fn() for _ in range(repeats)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device-batches', default='', help='comma-separated batch sizes for the device Huffman decode phases')
    ap.add_argument('--json', default='', help='write the results to this file as well')
    ap.add_argument('--entropy', default='device', choices=('device', 'device_sync'),
                    help="device_sync: measure the chunk decode as well, per --chunk-bytes value")
    ap.add_argument('--chunk-bytes', default='', help='comma-separated chunk sizes (default: the module default)')
    ap.add_argument('--max-rounds', type=int, default=None, help='synchronisation rounds (default: the module default)')
    args = ap.parse_args()
    try:
        import PIL  # noqa: F401
    except ImportError:
        print('jpeg_bench: Pillow is not importable here, so the input images cannot be made; nothing measured')
        return 0
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import image_io
    from mmdet_yolov4_amd._lib import JpegImage, JpegInfo
    from mmdet_yolov4_amd.ops import stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_bench: no GPU')
    dev = torch.device('cuda:0')
    L = pkg._lib.lib()
    bufs = make_images(args.images)
    N = len(bufs)
    file_bytes = sum(len(b) for b in bufs)
    res = dict(images=N, height=480, width=640, sampling='4:2:0', quality=90, mean_file_bytes=file_bytes // N)

    # ---- host half ------------------------------------------------------------------------------------------------
    infos = image_io._parse_all(bufs, 'jpeg_bench')
    table = (JpegImage * N)()
    totals = (C.c_int64 * 3)()
    assert L.yv4_jpeg_layout(infos, N, table, totals) == 0
    ncoef, work_bytes, out_bytes = (int(t) for t in totals)
    stage, (_, quant_off, coef_off) = image_io._stage(((table, C.sizeof(table)), image_io._quant_section(infos),
                                                       (lambda p: None, 2 * ncoef)))      # coefficients: host() below
    base = stage.data_ptr()

    def host(n):
        info = JpegInfo()
        assert L.yv4_jpeg_parse(bufs[n], len(bufs[n]), C.byref(info)) == 0
        st = L.yv4_jpeg_entropy_decode(bufs[n], len(bufs[n]), C.byref(info), base + coef_off + 2 * int(table[n].coef_off),
                                       int(info.ncoef))
        assert st == 0

    rounds = 8

    def one_thread():
        t0 = time.perf_counter()
        for _ in range(rounds):
            for n in range(N):
                host(n)
        return time.perf_counter() - t0

    pool = ThreadPoolExecutor(max_workers=THREADS)

    def many_threads():      # one pass per batch, as imdecode runs it: no two threads share an image's coefficients
        t0 = time.perf_counter()
        for _ in range(rounds):
            list(pool.map(host, range(N)))
        return time.perf_counter() - t0

    for name, fn in (('host_1_thread', one_thread), (f'host_{THREADS}_threads', many_threads)):
        med, lo, hi = windows(fn, args.repeats)
        res[name + '_files_per_s'] = round(N * rounds / med, 1)
        res[name + '_spread'] = [round(N * rounds / hi, 1), round(N * rounds / lo, 1)]
        print(f'{name:>22}: {N * rounds / med:9.1f} files/s   ({1e3 * med / (N * rounds):.3f} ms per file; '
              f'windows {N * rounds / hi:.0f} .. {N * rounds / lo:.0f} files/s)')
    pool.shutdown()

    # ---- upload ---------------------------------------------------------------------------------------------------
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    up = torch.empty(stage.numel(), dtype=torch.uint8, device=dev)
    copies = 20

    def upload():
        ev0.record()
        for _ in range(copies):
            up.copy_(stage, non_blocking=True)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3

    med, lo, hi = windows(upload, args.repeats)
    res['upload_ms'] = round(1e3 * med / copies, 4)
    res['upload_gb_per_s'] = round(stage.numel() * copies / med / 1e9, 2)
    print(f'{"upload":>22}: {1e3 * med / copies:9.4f} ms for {stage.numel() / 1e6:.2f} MB   ({res["upload_gb_per_s"]} GB/s; '
          f'windows {1e3 * lo / copies:.4f} .. {1e3 * hi / copies:.4f} ms)')

    # ---- device kernels -------------------------------------------------------------------------------------------
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    calls = 200
    pixels = sum(int(t.width) * int(t.height) for t in table)
    moved = 4 * ncoef + 3 * pixels

    def kernels():
        ev0.record()
        for _ in range(calls):
            st = L.yv4_jpeg_reconstruct(table, up.data_ptr(), N, up.data_ptr() + coef_off, ncoef, up.data_ptr() + quant_off,
                                        work.data_ptr(), work_bytes, out.data_ptr(), out_bytes, 0, stream_ptr())
            assert st == 0
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3

    med, lo, hi = windows(kernels, args.repeats)
    res['device_ms'] = round(1e3 * med / calls, 4)
    res['device_files_per_s'] = round(N * calls / med, 1)
    res['device_bytes_per_s'] = round(moved * calls / med, 0)
    res['device_share_of_hbm'] = round(moved * calls / med / HBM_BYTES_PER_S, 4)
    print(f'{"device kernels":>22}: {1e3 * med / calls:9.4f} ms per batch of {N}   ({N * calls / med:.0f} files/s; '
          f'{moved / 1e6:.2f} MB moved -> {moved * calls / med / 1e9:.1f} GB/s = {100 * moved * calls / med / HBM_BYTES_PER_S:.1f} % '
          f'of the {HBM_BYTES_PER_S / 1e12:.2f} TB/s HBM copy rate; windows {1e3 * lo / calls:.4f} .. {1e3 * hi / calls:.4f} ms)')

    # ---- end to end -----------------------------------------------------------------------------------------------
    def end_to_end():
        t0 = time.perf_counter()
        for _ in range(4):
            pkg.imdecode(bufs, device=dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    med, lo, hi = windows(end_to_end, args.repeats)
    res['imdecode_files_per_s'] = round(4 * N / med, 1)
    print(f'{"imdecode(batch)":>22}: {4 * N / med:9.1f} files/s   ({1e3 * med / 4:.2f} ms per batch of {N}; '
          f'windows {4 * N / hi:.0f} .. {4 * N / lo:.0f} files/s)')

    # the decode is only worth timing if it is right
    from PIL import Image
    got = pkg.imdecode(bufs, channel_order='rgb', device=dev)
    for b, g in zip(bufs, got):
        assert np.array_equal(g.cpu().numpy(), np.asarray(Image.open(io.BytesIO(b)))), 'decode differs from Pillow'

    def pillow():
        t0 = time.perf_counter()
        for _ in range(rounds):
            for b in bufs:
                np.asarray(Image.open(io.BytesIO(b)))
        return time.perf_counter() - t0

    med, lo, hi = windows(pillow, args.repeats)
    res['pillow_1_thread_files_per_s'] = round(N * rounds / med, 1)
    print(f'{"Pillow, 1 thread":>22}: {N * rounds / med:9.1f} files/s   ({1e3 * med / (N * rounds):.3f} ms per file; '
          f'windows {N * rounds / hi:.0f} .. {N * rounds / lo:.0f} files/s)   [bytes equal to imdecode: yes]')
    if args.device_batches:
        sizes = [int(b) for b in args.device_batches.split(',')]
        restart = make_images(min(N, 32), restart_marker_rows=1)
        res['device_entropy'] = [device_phases(kind, src, B, args.repeats, dev)
                                 for kind, src in (('plain', bufs), ('restart_rows_1', restart)) for B in sizes]
        if args.entropy == 'device_sync':
            chunk_sizes = [int(c) for c in args.chunk_bytes.split(',')] if args.chunk_bytes else [image_io.DEFAULT_CHUNK_BYTES]
            rounds_max = image_io.DEFAULT_MAX_ROUNDS if args.max_rounds is None else args.max_rounds
            res['max_rounds'] = rounds_max
            for r, (kind, src) in zip(res['device_entropy'], [(k, s) for k, s in (('plain', bufs), ('restart_rows_1', restart))
                                                              for _ in sizes]):
                r['device_sync'] = [sync_phases(kind, src, r['batch'], args.repeats, dev, cb, rounds_max) for cb in chunk_sizes]
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    return 0


def device_phases(kind, src, B, repeats, dev):
    """The phases of the device Huffman decode for the first ``B`` files of ``src`` repeated."""
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import image_io
    from mmdet_yolov4_amd._lib import JpegImage
    from mmdet_yolov4_amd.ops import stream_ptr
    L = pkg._lib.lib()
    bufs = [src[i % len(src)] for i in range(B)]
    r = dict(files=kind, batch=B)
    print(f'--- device Huffman decode: {kind}, batch of {B} ---')

    def prepare():
        t0 = time.perf_counter()
        image_io.ScanTables(bufs)
        return time.perf_counter() - t0

    med, lo, hi = windows(prepare, repeats)
    r['prepare_1_thread_files_per_s'] = round(B / med, 1)
    t = image_io.ScanTables(bufs)
    r['segments'], r['workgroups'] = t.nseg, t.nwg
    print(f'{"prepare, 1 thread":>22}: {B / med:9.1f} files/s   ({1e6 * med / B:.1f} us per file; {t.nseg} segments in {t.nwg} '
          f'workgroups)')

    table = (JpegImage * B)()
    totals = (C.c_int64 * 3)()
    assert L.yv4_jpeg_layout(t.infos, B, table, totals) == 0
    ncoef, work_bytes, out_bytes = (int(v) for v in totals)
    stage, offs = image_io._stage(((table, C.sizeof(table)), image_io._quant_section(t.infos)) + t.sections())
    end = stage.numel()
    r['staging_bytes'], r['host_path_staging_bytes'] = end, offs[2] + 2 * ncoef
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    up = torch.empty(end, dtype=torch.uint8, device=dev)
    copies = 20

    def upload():
        ev0.record()
        for _ in range(copies):
            up.copy_(stage, non_blocking=True)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3

    med, lo, hi = windows(upload, repeats)
    r['upload_ms'] = round(1e3 * med / copies, 4)
    print(f'{"upload":>22}: {1e3 * med / copies:9.4f} ms for {end / 1e6:.2f} MB (the host path stages {r["host_path_staging_bytes"] / 1e6:.2f} MB)')

    coef = torch.empty(ncoef, dtype=torch.int16, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    d = [up.data_ptr() + o for o in offs]
    calls = 3

    def entropy():
        image_io._launch_segments(L, t, d[2:], B, coef, ncoef, status)

    def reconstruct():
        st = L.yv4_jpeg_reconstruct(table, d[0], B, coef.data_ptr(), ncoef, d[1], work.data_ptr(), work_bytes, out.data_ptr(),
                                    out_bytes, 0, stream_ptr())
        assert st == 0

    def timed(*steps):
        def window():
            ev0.record()
            for _ in range(calls):
                for step in steps:
                    step()
            ev1.record()
            ev1.synchronize()
            return ev0.elapsed_time(ev1) * 1e-3
        return window

    for name, fn in (('entropy', timed(entropy)), ('entropy_reconstruct', timed(entropy, reconstruct))):
        med, lo, hi = windows(fn, repeats)
        r[name + '_ms'] = round(1e3 * med / calls, 4)
        r[name + '_spread_ms'] = [round(1e3 * lo / calls, 4), round(1e3 * hi / calls, 4)]
        print(f'{name:>22}: {1e3 * med / calls:9.4f} ms per batch of {B}   ({B * calls / med:.0f} files/s; windows '
              f'{1e3 * lo / calls:.4f} .. {1e3 * hi / calls:.4f} ms)')
    assert not status.cpu().any()
    symbols = None
    if kind == 'plain':      # the single-lane symbol rate: coded symbols of the slowest file over the batch's time
        per_file = []
        for b in src[:len(src)]:
            c = image_io.jpeg_entropy_decode(b)[1].reshape(-1, 64)
            # per block: one DC symbol, one symbol per nonzero AC coefficient, ZRLs not counted, one EOB unless it ends at 63
            per_file.append(int(c.shape[0] + (c[:, 1:] != 0).sum() + (c[:, 63] == 0).sum()))
        symbols = max(per_file)
        r['symbols_of_largest_file'] = symbols
        r['ns_per_symbol_one_lane'] = round(1e6 * r['entropy_ms'] / symbols, 2)
        print(f'{"one lane":>22}: {symbols} symbols in the largest file -> at most {r["ns_per_symbol_one_lane"]} ns per symbol')

    def end_to_end(mode):
        def window():
            t0 = time.perf_counter()
            for _ in range(2):
                pkg.imdecode(bufs, device=dev, entropy=mode)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 2
        return window

    keep = image_io.MAX_DECODE_THREADS
    for name, mode, threads in (('imdecode_device', 'device', keep), ('imdecode_host_16_threads', 'host', 16),
                                ('imdecode_host_2_threads', 'host', 2)):
        image_io.MAX_DECODE_THREADS = threads
        try:
            med, lo, hi = windows(end_to_end(mode), repeats)
        finally:
            image_io.MAX_DECODE_THREADS = keep
        r[name + '_ms'] = round(1e3 * med, 3)
        r[name + '_files_per_s'] = round(B / med, 1)
        print(f'{name:>26}: {1e3 * med:9.3f} ms per batch of {B}   ({B / med:.0f} files/s; windows {1e3 * lo:.3f} .. {1e3 * hi:.3f} ms)')
    a = pkg.imdecode(bufs[:len(src)], device=dev, entropy='device')
    b = pkg.imdecode(bufs[:len(src)], device=dev, entropy='host')
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the device path differs from the host path'
    return r


_ROUNDS = {}      # (files, chunk size, count) -> rounds each image's chains need to close


def sync_phases(kind, src, B, repeats, dev, chunk_bytes, max_rounds):
    """The chunk decode (``entropy='device_sync'``) of the first ``B`` files of ``src`` repeated, at one chunk size."""
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import image_io
    from mmdet_yolov4_amd._lib import JpegEntry
    bufs = [src[i % len(src)] for i in range(B)]
    r = dict(chunk_bytes=chunk_bytes, max_rounds=max_rounds)
    print(f'--- chunk decode: {kind}, batch of {B}, chunks of {chunk_bytes} bytes, {max_rounds} rounds ---')
    # rounds to convergence: the CPU run of the same core over the distinct files (a repeated file needs the same)
    key = (kind, chunk_bytes, min(B, len(src)))
    if key not in _ROUNDS:
        _ROUNDS[key] = [image_io.jpeg_entropy_decode_sync([b], chunk_bytes, pkg._lib.JPEG_MAX_ROUNDS)[6] for b in src[:key[2]]]
    per_image = _ROUNDS[key]
    r['rounds_to_convergence'] = max(per_image)
    r['rounds_per_image_median'], r['rounds_per_image_max'] = int(statistics.median(per_image)), max(per_image)
    t = image_io.ScanTables(bufs)
    ch = image_io.ChunkTables(t, chunk_bytes)
    r['chunks'], r['workgroups'] = ch.nchunk, ch.nwg
    stage, offs = image_io._stage(t.sections() + ch.sections())
    up = stage.to(dev)
    r['staging_bytes'] = stage.numel()
    coef = torch.empty(t.ncoef, dtype=torch.int16, device=dev)
    flags = torch.empty(2 * B, dtype=torch.int32, device=dev)
    entries = torch.empty(ch.nchunk * C.sizeof(JpegEntry), dtype=torch.uint8, device=dev)
    d = [up.data_ptr() + o for o in offs]
    L = pkg._lib.lib()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 3

    def kernels(rounds):
        def window():
            ev0.record()
            for _ in range(calls):
                image_io._launch_sync(L, t, ch, d, B, rounds, entries, coef, t.ncoef, flags[:B], flags[B:])
            ev1.record()
            ev1.synchronize()
            return ev0.elapsed_time(ev1) * 1e-3
        return window

    for name, rounds in (('kernels', max_rounds), ('kernels_0_rounds', 0)):
        med, lo, hi = windows(kernels(rounds), repeats)
        r[name + '_ms'] = round(1e3 * med / calls, 4)
        r[name + '_spread_ms'] = [round(1e3 * lo / calls, 4), round(1e3 * hi / calls, 4)]
        print(f'{name:>22}: {1e3 * med / calls:9.4f} ms per batch of {B}   (windows {1e3 * lo / calls:.4f} .. {1e3 * hi / calls:.4f} ms)')
        if rounds == max_rounds:
            codes = flags.cpu().numpy()
            assert not codes[:B].any()
            r['undecided_images'] = int((codes[B:] != 0).sum())
            r['undecided_share'] = round(r['undecided_images'] / B, 4)
    print(f'{"chains":>22}: {ch.nchunk} chunks in {ch.nwg} workgroups; closed after {r["rounds_to_convergence"]} rounds (per image: '
          f'median {r["rounds_per_image_median"]}, max {r["rounds_per_image_max"]}); {r["undecided_images"]} of {B} images '
          f'undecided at {max_rounds} rounds')

    def end_to_end():
        t0 = time.perf_counter()
        for _ in range(2):
            pkg.imdecode(bufs, device=dev, entropy='device_sync', chunk_bytes=chunk_bytes, max_rounds=max_rounds)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 2

    med, lo, hi = windows(end_to_end, repeats)
    r['imdecode_device_sync_ms'] = round(1e3 * med, 3)
    r['imdecode_device_sync_files_per_s'] = round(B / med, 1)
    print(f'{"imdecode_device_sync":>26}: {1e3 * med:9.3f} ms per batch of {B}   ({B / med:.0f} files/s; windows {1e3 * lo:.3f} .. '
          f'{1e3 * hi:.3f} ms)')
    a = pkg.imdecode(bufs[:len(src)], device=dev, entropy='device_sync', chunk_bytes=chunk_bytes, max_rounds=max_rounds)
    b = pkg.imdecode(bufs[:len(src)], device=dev, entropy='host')
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the chunk decode differs from the host path'
    return r


if __name__ == '__main__':
    sys.exit(main())
