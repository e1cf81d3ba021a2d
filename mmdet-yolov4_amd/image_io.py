"""Image files onto the GPU: ``imread`` / ``imdecode`` for baseline JPEG, and the ``LoadImageFromFile`` transform.

The decoder is a hybrid (``include/yv4.h``, "baseline JPEG decoding"): the host parses the file and runs the Huffman
decode (``yv4_jpeg_parse`` / ``yv4_jpeg_entropy_decode``, sequential by nature, one thread per image), the device does
everything from the quantised coefficients to interleaved pixels (``yv4_jpeg_reconstruct``: dequantisation, libjpeg's
"islow" integer IDCT, fancy chroma upsampling, integer YCbCr conversion).  A batch is one reconstruct call; its
coefficients, quantisation tables and per-image table go up through one pinned staging buffer.  With ``entropy='device'``
the Huffman decode runs on the device as well (``yv4_jpeg_scan_prepare`` / ``yv4_jpeg_entropy_decode_device``, one lane per
restart segment): the files and their segment tables go up instead of the coefficients, and the host only parses.
``entropy='device_sync'`` cuts every segment into chunks that many lanes decode at once from self-synchronised entry
points (``yv4_jpeg_entropy_decode_device_sync``), which is what gives a file without restart markers more than one lane;
whatever that path cannot prove goes through the ``'device'`` kernel again.

The pixels equal libjpeg-turbo's default decode bit for bit, which is what ``cv2.imdecode``, turbojpeg and Pillow -- every
backend of ``mmcv.imfrombytes`` -- return.  EXIF orientation (``cv2.imdecode(IMREAD_COLOR)`` and
``mmcv.imread(flag='color')`` rotate by it; turbojpeg and a bare Pillow decode do not) is read by the header parse
(``JpegInfo.orientation``) and applied by the pixel stage where the caller asks: ``orientation=True`` of ``imdecode`` /
``imread`` / ``decode_into``, ``apply_orientation=True`` of ``LoadImageFromFile``.  The default is off; the training
loader (``datasets.TrainLoader``) turns it on for ``color_type='color'``, as the reference's reader does.

Accepted: 8-bit baseline (SOF0 / SOF1 Huffman) files, grayscale or YCbCr in 4:4:4, 4:2:2 or 4:2:0.  Progressive,
arithmetic-coded, 12-bit, lossless, CMYK and multi-scan files and every other format raise ``NotImplementedError``.

The other direction is at the end of the module: ``imencode`` / ``imwrite`` / ``encode_into`` write baseline JPEG on the
device (``include/yv4.h``, "baseline JPEG encoding"): libjpeg's default encoder restated in integer arithmetic, so the
file equals what libjpeg-turbo -- ``cv2.imwrite``, and so ``mmcv.imwrite`` -- writes for the same pixels, quality and
sampling, byte for byte.  The scan bytes are compacted on the device before the read-back, so what crosses to the host
is the size of the files.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import JpegChunk, JpegEntry, JpegHuff, JpegImage, JpegInfo, JpegScan, JpegSegment, JpegWg, check
from .ops import stream_ptr
from .registry import PIPELINES

#: the host entropy decodes of a batch run on at most this many threads (never sized from the machine's CPU count)
MAX_DECODE_THREADS = 16

_MAGIC = ((b'\x89PNG\r\n\x1a\n', 'PNG'), (b'GIF87a', 'GIF'), (b'GIF89a', 'GIF'), (b'BM', 'BMP'), (b'II*\x00', 'TIFF'),
          (b'MM\x00*', 'TIFF'), (b'\x00\x00\x00\x0cjP  ', 'JPEG 2000'), (b'\xff\x4f\xff\x51', 'JPEG 2000'),
          (b'P5', 'PNM'), (b'P6', 'PNM'))


def image_format(buf):
    """The format of an encoded image by its magic bytes: ``'JPEG'``, ``'PNG'``, ... or ``'unknown'``."""
    head = bytes(buf[:16])
    if head[:2] == b'\xff\xd8':
        return 'JPEG'
    if head[:4] == b'RIFF' and head[8:12] == b'WEBP':
        return 'WebP'
    for magic, name in _MAGIC:
        if head.startswith(magic):
            return name
    return 'unknown'


def _raise(status, what):
    msg = _lib.lib().yv4_last_error().decode('utf-8', 'replace')      # thread-local: read on the thread that made the call
    if status == _lib.E_UNSUPPORTED:
        raise NotImplementedError(f'{what}: {msg}')
    if status == _lib.E_INVALID:
        raise ValueError(f'{what}: {msg}')
    raise _lib.Yv4Error(f'{what} failed with status {status}: {msg}')


def _as_bytes(buf):
    if isinstance(buf, np.ndarray):
        buf = buf.tobytes()
    if not isinstance(buf, (bytes, bytearray, memoryview)):
        raise TypeError(f'an encoded image is a bytes object, not {type(buf).__name__}')
    buf = bytes(buf)
    fmt = image_format(buf)
    if fmt != 'JPEG':
        raise NotImplementedError(f'{fmt} images are not built: the decoder reads baseline JPEG only')
    return buf


def jpeg_parse(buf):
    """The host half's header parse -> ``JpegInfo`` (``yv4_jpeg_info``).  Needs no GPU."""
    info = JpegInfo()
    st = _lib.lib().yv4_jpeg_parse(buf, len(buf), C.byref(info))
    if st != 0:
        _raise(st, 'yv4_jpeg_parse')
    return info


def jpeg_entropy_decode(buf):
    """The host half on its own -> ``(JpegInfo, int16 coefficient array)``.  Needs no GPU."""
    info = jpeg_parse(buf)
    coef = np.empty(int(info.ncoef), np.int16)
    st = _lib.lib().yv4_jpeg_entropy_decode(buf, len(buf), C.byref(info), coef.ctypes.data, coef.size)
    if st != 0:
        _raise(st, 'yv4_jpeg_entropy_decode')
    return info, coef


def _align(n, a=256):
    return (n + a - 1) // a * a


#: where the Huffman scan of a file is decoded when a call does not say: ``'host'`` (``yv4_jpeg_entropy_decode`` on a
#: thread pool), ``'device'`` (``yv4_jpeg_entropy_decode_device``, one lane per restart segment) or ``'device_sync'``
#: (``yv4_jpeg_entropy_decode_device_sync``, one lane per chunk of a segment).  ``set_default_entropy`` changes it.
DEFAULT_ENTROPY = 'host'
ENTROPY_MODES = ('host', 'device', 'device_sync')

#: ``entropy='device_sync'``: the raw bytes of a segment one lane decodes, and the synchronisation rounds after the
#: first pass, when a call does not say (DESIGN 19.2 has the sweep they come from)
DEFAULT_CHUNK_BYTES = 64
DEFAULT_MAX_ROUNDS = 48


def set_default_entropy(mode):
    """Sets the module's default for ``entropy=`` (``'host'``, ``'device'`` or ``'device_sync'``) and returns the
    previous one."""
    global DEFAULT_ENTROPY
    if mode not in ENTROPY_MODES:
        raise ValueError(f"entropy {mode!r} is not 'host', 'device' or 'device_sync'")
    prev, DEFAULT_ENTROPY = DEFAULT_ENTROPY, mode
    return prev


def _entropy_mode(entropy):
    mode = DEFAULT_ENTROPY if entropy is None else entropy
    if mode not in ENTROPY_MODES:
        raise ValueError(f"entropy {mode!r} is not 'host', 'device' or 'device_sync'")
    return mode


def _sync_params(chunk_bytes, max_rounds):
    """The validated ``(chunk_bytes, max_rounds)`` of a ``'device_sync'`` decode; ``None``: the module's defaults."""
    cb = DEFAULT_CHUNK_BYTES if chunk_bytes is None else chunk_bytes
    mr = DEFAULT_MAX_ROUNDS if max_rounds is None else max_rounds
    for name, v, lo, hi in (('chunk_bytes', cb, _lib.JPEG_MIN_CHUNK_BYTES, _lib.JPEG_MAX_CHUNK_BYTES),
                            ('max_rounds', mr, 0, _lib.JPEG_MAX_ROUNDS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{name} {v!r} is not an integer in {lo} .. {hi}')
    return int(cb), int(mr)


def _parse_all(bufs, what):
    """``yv4_jpeg_parse`` of every file -> the ``JpegInfo`` array.  A refused or malformed file raises as ``jpeg_parse``
    does, naming the image."""
    L = _lib.lib()
    infos = (JpegInfo * len(bufs))()
    for n, b in enumerate(bufs):
        st = L.yv4_jpeg_parse(b, len(b), C.byref(infos[n]))
        if st != 0:
            _raise(st, f'{what}: image {n}')
    return infos


def _host_decode_all(bufs, infos, base, coef_offs, what):
    """The host Huffman decode of every file (``yv4_jpeg_entropy_decode``) straight to host address ``base``, image n at
    int16 element ``coef_offs[n]``, on at most ``MAX_DECODE_THREADS`` threads."""
    L = _lib.lib()

    def one(n):
        info = JpegInfo()
        st = L.yv4_jpeg_entropy_decode(bufs[n], len(bufs[n]), C.byref(info), base + 2 * int(coef_offs[n]), int(infos[n].ncoef))
        if st != 0:
            _raise(st, f'{what}: image {n}')

    if len(bufs) == 1:
        one(0)
    else:
        with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, len(bufs))) as pool:      # ctypes releases the GIL
            list(pool.map(one, range(len(bufs))))


class ScanTables:
    """The host tables of a device Huffman decode (``include/yv4.h``, "the Huffman scan on the device") for a list of
    files: ``infos``, ``scans`` (one per image, placed: files back to back at 4-byte aligned offsets, segments and packed
    tables dense, ``coef_off`` as given), ``segs``, ``wgs``, ``huff``; ``nseg``, ``nwg``, ``nhuff``, ``nbytes``.  Needs
    no GPU.  A refused or malformed file raises as ``jpeg_parse`` does, naming the image."""

    def __init__(self, bufs, coef_offs=None, what='jpeg_scan_tables'):
        L = _lib.lib()
        N = len(bufs)
        self.bufs = bufs
        self.infos = _parse_all(bufs, what)
        counts = [-(-f.mcus_x * f.mcus_y // f.restart_interval) if f.restart_interval else 1 for f in self.infos]
        self.nseg = sum(counts)
        self.scans = (JpegScan * N)()
        self.segs = (JpegSegment * self.nseg)()
        self.huff = (JpegHuff * (_lib.JPEG_MAX_HUFF * N))()
        seg = nhuff = off = coef = 0
        info = JpegInfo()
        for n, b in enumerate(bufs):
            sc = self.scans[n]
            st = L.yv4_jpeg_scan_prepare(b, len(b), C.byref(info), C.addressof(sc),
                                         C.addressof(self.huff) + nhuff * C.sizeof(JpegHuff),
                                         C.addressof(self.segs) + seg * C.sizeof(JpegSegment), counts[n])
            if st != 0:
                _raise(st, f'{what}: image {n}')
            sc.data_off, sc.seg_base, sc.huff_base = off, seg, nhuff
            sc.coef_off = coef if coef_offs is None else int(coef_offs[n])
            off += _align(len(b), 4)
            seg += sc.nseg
            nhuff += sc.nhuff
            coef += int(sc.ncoef)
        self.nhuff, self.nbytes, self.ncoef = nhuff, off, coef
        count = C.c_int64()
        scans = C.addressof(self.scans)
        check(L.yv4_jpeg_entropy_workgroups(scans, N, None, 0, C.byref(count)), 'yv4_jpeg_entropy_workgroups')
        self.nwg = int(count.value)
        self.wgs = (JpegWg * self.nwg)()
        check(L.yv4_jpeg_entropy_workgroups(scans, N, C.addressof(self.wgs), self.nwg, C.byref(count)),
              'yv4_jpeg_entropy_workgroups')

    def sections(self):
        """``(source, byte count)`` of each table in upload order (``_stage``): scans, segs, wgs, huff, file bytes."""
        return ((self.scans, C.sizeof(self.scans)), (self.segs, C.sizeof(self.segs)), (self.wgs, C.sizeof(self.wgs)),
                (self.huff, self.nhuff * C.sizeof(JpegHuff)), (self.write_bytes, self.nbytes))

    def write_bytes(self, base):
        """The files to host address ``base`` at their ``data_off``."""
        for sc, b in zip(self.scans, self.bufs):
            C.memmove(base + int(sc.data_off), b, len(b))

    def cpu_buffers(self, flags):
        """What a CPU run of the core decodes from and into: the files in a zeroed byte array, the int16 coefficient
        array, and ``flags`` arrays of one int32 per image."""
        data = np.zeros(max(self.nbytes, 1), np.uint8)
        self.write_bytes(data.ctypes.data)
        return (data, np.empty(self.ncoef, np.int16)) + tuple(np.empty(len(self.bufs), np.int32) for _ in range(flags))


class ChunkTables:
    """The chunk tables of a ``'device_sync'`` decode (``include/yv4.h``, "self-synchronising chunks") over a
    ``ScanTables``: ``chunks``, ``seg_first``, ``wgs``; ``nchunk``, ``nwg``, ``chunk_bytes``.  Needs no GPU."""

    def __init__(self, scan, chunk_bytes):
        L = _lib.lib()
        self.scan, self.chunk_bytes = scan, chunk_bytes
        nchunk, nwg = C.c_int64(), C.c_int64()
        args = (C.addressof(scan.scans), C.addressof(scan.segs), len(scan.bufs), scan.nseg, chunk_bytes)
        check(L.yv4_jpeg_chunks_build(*args, None, 0, None, None, 0, C.byref(nchunk), C.byref(nwg)), 'yv4_jpeg_chunks_build')
        self.nchunk, self.nwg = int(nchunk.value), int(nwg.value)
        self.chunks = (JpegChunk * self.nchunk)()
        self.seg_first = (C.c_int32 * (scan.nseg + 1))()
        self.wgs = (JpegWg * self.nwg)()
        check(L.yv4_jpeg_chunks_build(*args, C.addressof(self.chunks), self.nchunk, C.addressof(self.seg_first),
                                      C.addressof(self.wgs), self.nwg, C.byref(nchunk), C.byref(nwg)),
              'yv4_jpeg_chunks_build')

    def sections(self):
        """``(source, byte count)`` of each table in upload order: chunks, seg_first, wgs."""
        return ((self.chunks, C.sizeof(self.chunks)), (self.seg_first, C.sizeof(self.seg_first)),
                (self.wgs, C.sizeof(self.wgs)))


def jpeg_entropy_decode_sync(bufs, chunk_bytes=None, max_rounds=None):
    """The whole ``'device_sync'`` method on the CPU (``yv4_jpeg_entropy_decode_sync``: the core the kernels run, then the
    one lane per segment decode of the undecided images) -> ``(ScanTables, ChunkTables, JpegEntry array, int16
    coefficients, int32 status per image, int32 undecided per image, last round that changed an entry)``.  Needs no
    GPU."""
    chunk_bytes, max_rounds = _sync_params(chunk_bytes, max_rounds)
    t = ScanTables(bufs)
    ch = ChunkTables(t, chunk_bytes)
    data, coef, status, undecided = t.cpu_buffers(2)
    entries = (JpegEntry * ch.nchunk)()
    rounds = C.c_int32()
    check(_lib.lib().yv4_jpeg_entropy_decode_sync(
        C.addressof(t.scans), C.addressof(t.segs), C.addressof(ch.chunks), C.addressof(ch.seg_first), C.addressof(ch.wgs),
        len(bufs), t.nseg, ch.nchunk, ch.nwg, data.ctypes.data, t.nbytes, C.addressof(t.huff), t.nhuff, chunk_bytes,
        max_rounds, C.addressof(entries), coef.ctypes.data, coef.size, status.ctypes.data, undecided.ctypes.data,
        C.addressof(rounds)), 'yv4_jpeg_entropy_decode_sync')
    return t, ch, entries, coef, status, undecided, int(rounds.value)


def jpeg_entropy_decode_segments(bufs):
    """The device decode's tables and core run on the CPU (``yv4_jpeg_entropy_decode_segments``) -> ``(ScanTables, int16
    coefficients of the batch, int32 status per image)``.  Needs no GPU."""
    t = ScanTables(bufs)
    data, coef, status = t.cpu_buffers(1)
    check(_lib.lib().yv4_jpeg_entropy_decode_segments(
        C.addressof(t.scans), C.addressof(t.segs), C.addressof(t.wgs), len(bufs), t.nseg, t.nwg, data.ctypes.data, t.nbytes,
        C.addressof(t.huff), t.nhuff, coef.ctypes.data, coef.size, status.ctypes.data), 'yv4_jpeg_entropy_decode_segments')
    return t, coef, status


def _stage(sections):
    """One pinned staging buffer holding ``sections``, each at the next 256-byte boundary -> ``(uint8 tensor, offsets)``.
    A section is ``(source, byte count)``; a source is a ctypes object to copy, or a function that writes the section
    at the host address it is given (the files, the quantisation tables, the host decode's coefficients)."""
    offs, end = [], 0
    for _, size in sections:
        offs.append(end)
        end += _align(size)
    stage = torch.empty(end, dtype=torch.uint8, pin_memory=True)
    for (src, size), off in zip(sections, offs):
        if callable(src):
            src(stage.data_ptr() + off)
        else:
            C.memmove(stage.data_ptr() + off, src, size)
    return stage, offs


def _quant_section(infos):
    """The quantisation tables of a batch as a ``_stage`` section: (N, 4, 64) uint16."""
    def write(base):
        for n, f in enumerate(infos):
            C.memmove(base + n * 512, f.quant, 512)
    return write, len(infos) * 512


def _launch_segments(L, scan, d, N, coef, ncoef, status):
    """``yv4_jpeg_entropy_decode_device`` over uploaded tables: ``d`` holds the device addresses of ``scan.sections()``."""
    check(L.yv4_jpeg_entropy_decode_device(
        C.addressof(scan.scans), C.addressof(scan.segs), C.addressof(scan.wgs), d[0], d[1], d[2], N, scan.nseg, scan.nwg,
        d[4], scan.nbytes, d[3], scan.nhuff, coef.data_ptr(), ncoef, status.data_ptr(), stream_ptr()),
        'yv4_jpeg_entropy_decode_device')


def _launch_sync(L, scan, ch, d, N, max_rounds, entries, coef, ncoef, status, undecided):
    """``yv4_jpeg_entropy_decode_device_sync`` over uploaded tables: ``d`` holds the device addresses of scans, segs, the
    segment workgroups (unused here), huff, the files, chunks, seg_first and the chunk workgroups."""
    check(L.yv4_jpeg_entropy_decode_device_sync(
        C.addressof(scan.scans), C.addressof(scan.segs), C.addressof(ch.chunks), C.addressof(ch.seg_first),
        C.addressof(ch.wgs), d[0], d[1], d[5], d[6], d[7], N, scan.nseg, ch.nchunk, ch.nwg, d[4], scan.nbytes, d[3],
        scan.nhuff, ch.chunk_bytes, max_rounds, entries.data_ptr(), coef.data_ptr(), ncoef, status.data_ptr(),
        undecided.data_ptr(), stream_ptr()), 'yv4_jpeg_entropy_decode_device_sync')


def jpeg_entropy_decode_device_sync(bufs, chunk_bytes=None, max_rounds=None, device=None, coef=None, status=None,
                                    undecided=None, tables=None):
    """The chunk kernels on their own, without the second decode of undecided images -> ``(ScanTables, ChunkTables, int16
    coefficient tensor, int32 status tensor, int32 undecided tensor)`` on the GPU, nothing read back.  ``coef`` /
    ``status`` / ``undecided``: the caller's tensors to decode into, as in ``jpeg_entropy_decode_device``."""
    chunk_bytes, max_rounds = _sync_params(chunk_bytes, max_rounds)
    _lib.require('jpeg_sync')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    t = ScanTables(bufs) if tables is None else tables
    ch = ChunkTables(t, chunk_bytes)
    stage, offs = _stage(t.sections() + ch.sections())
    with torch.cuda.device(dev):
        up = stage.to(dev, non_blocking=True)
        coef = torch.empty(t.ncoef, dtype=torch.int16, device=dev) if coef is None else coef
        status = torch.empty(len(bufs), dtype=torch.int32, device=dev) if status is None else status
        undecided = torch.empty(len(bufs), dtype=torch.int32, device=dev) if undecided is None else undecided
        entries = torch.empty(ch.nchunk * C.sizeof(JpegEntry), dtype=torch.uint8, device=dev)
        _launch_sync(_lib.lib(), t, ch, [up.data_ptr() + o for o in offs], len(bufs), max_rounds, entries, coef,
                     coef.numel(), status, undecided)
    return t, ch, coef, status, undecided


def jpeg_entropy_decode_device(bufs, device=None, coef=None, status=None, tables=None):
    """The device Huffman decode on its own -> ``(ScanTables, int16 coefficient tensor, int32 status tensor)`` on the GPU,
    nothing read back.  ``coef`` / ``status``: the caller's tensors to decode into (``tables.ncoef`` / ``len(bufs)``
    elements, views into larger buffers say); ``tables``: a ``ScanTables`` of ``bufs`` made before."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    t = ScanTables(bufs) if tables is None else tables
    stage, offs = _stage(t.sections())
    with torch.cuda.device(dev):
        up = stage.to(dev, non_blocking=True)
        coef = torch.empty(t.ncoef, dtype=torch.int16, device=dev) if coef is None else coef
        status = torch.empty(len(bufs), dtype=torch.int32, device=dev) if status is None else status
        _launch_segments(_lib.lib(), t, [up.data_ptr() + o for o in offs], len(bufs), coef, coef.numel(), status)
    return t, coef, status


class HostHalf:
    """What the host does for a batch before any GPU call, so that a worker thread can do it ahead of time
    (``decode_into(host=...)``): the header parses (``infos``), with a device mode the scan and chunk tables, with
    ``'host'`` the Huffman decodes into ``coef`` (int16, the images back to back as ``yv4_jpeg_layout`` places them).
    Makes no HIP and no torch call.  A refused or malformed file raises as ``imdecode`` does, naming the image.
    ``run=False`` only validates the parameters: ``tables()`` then does the parses and the tables, and ``decode()`` the
    ``'host'`` mode's Huffman decodes (``decode_into`` decodes into its staging buffer instead)."""

    def __init__(self, bufs, entropy=None, chunk_bytes=None, max_rounds=None, what='imdecode', run=True):
        self.mode = _entropy_mode(entropy)
        self.chunk_bytes, self.max_rounds = chunk_bytes, max_rounds
        if self.mode == 'device_sync' or chunk_bytes is not None or max_rounds is not None:
            self.chunk_bytes, self.max_rounds = _sync_params(chunk_bytes, max_rounds)
        self.bufs, self.what = bufs, what
        self.infos = self.scan = self.chunks = self.coef = None
        if run:
            self.tables()
            self.decode()

    def tables(self):
        """The table half: the parses, and with a device mode the scan and chunk tables.  No Huffman decode."""
        if self.mode == 'host':
            self.infos = _parse_all(self.bufs, self.what)
            return
        self.scan = ScanTables(self.bufs, what=self.what)
        self.infos = self.scan.infos
        # chunks add no lane to a batch whose every segment is at most one chunk long: it is decoded as 'device'
        if self.mode == 'device_sync' and any(g.end - g.begin > self.chunk_bytes for g in self.scan.segs):
            self.chunks = ChunkTables(self.scan, self.chunk_bytes)

    def decode(self):
        """The ``'host'`` mode's Huffman decodes into ``coef``; nothing in a device mode."""
        if self.mode == 'host':
            offs = np.concatenate([[0], np.cumsum([int(f.ncoef) for f in self.infos])])
            self.coef = np.empty(int(offs[-1]), np.int16)
            _host_decode_all(self.bufs, self.infos, self.coef.ctypes.data, offs, self.what)


def oriented_size(t):
    """``(height, width)`` of the picture a ``JpegImage`` entry writes: swapped for orientations 5 to 8."""
    return (int(t.width), int(t.height)) if t.orientation >= 5 else (int(t.height), int(t.width))


def image_views(out, table):
    """The (h, w, 3) views of the images ``table`` places in the flat buffer ``out`` (``decode_into``'s results)."""
    views = []
    for t in table:
        (h, w), off = oriented_size(t), int(t.out_off)
        views.append(out[off:off + h * w * 3].view(h, w, 3))
    return views


def refusals(bufs):
    """The files of ``bufs`` the decoder refuses -> ``{position: NotImplementedError}``: another format, or a JPEG that
    ``jpeg_parse`` refuses.  A malformed header raises as ``jpeg_parse`` does."""
    refused = {}
    for k, b in enumerate(bufs):
        try:
            jpeg_parse(_as_bytes(b))
        except NotImplementedError as e:
            refused[k] = e
    return refused


def decode_into(bufs, channel_order='bgr', device=None, out=None, placement=None, entropy=None, chunk_bytes=None,
                max_rounds=None, orientation=False, host=None):
    """The batch decode behind ``imdecode``: ``bufs`` (a list of JPEG byte strings) -> ``(out, table)``, ``out`` the flat
    ``torch.uint8`` device buffer and ``table`` the ``JpegImage`` array saying where each image lies in it.  With ``out``
    and ``placement`` (``(byte offset, row pitch)`` per image) the pixels go into the caller's buffer instead -- rows of
    a larger canvas, say; the library checks every image against the buffer's size before the launch.

    ``entropy``: ``'host'`` decodes the Huffman scans on a thread pool and uploads coefficients; ``'device'`` uploads the
    files and their segment tables and decodes them in one launch (``yv4_jpeg_entropy_decode_device``), the coefficients
    never leaving device memory; ``'device_sync'`` does the same with one lane per ``chunk_bytes`` raw bytes of a segment,
    entered through at most ``max_rounds`` synchronisation rounds (``None``: ``DEFAULT_CHUNK_BYTES`` /
    ``DEFAULT_MAX_ROUNDS``); ``None``: ``DEFAULT_ENTROPY``.  All give the same pixels.  With the device modes the scan's
    errors are known only after the batch: one read-back of a status word per image, then ``ValueError`` naming the first
    bad image -- by then the batch's pixels have been written (a caller's ``out`` included).  ``'device_sync'`` reads a
    second word per image in that read-back: the images its chunks could not prove, damaged ones among them, are then
    decoded by the ``'device'`` kernel, which decides their status, and the batch is reconstructed again.  A batch whose
    segments are all at most one chunk long takes the ``'device'`` path directly.

    ``orientation=True`` applies each file's EXIF orientation in the pixel stage (``yv4_jpeg_layout_oriented``): the table
    then carries it, ``oriented_size`` gives the picture's size, and a ``placement`` pitch counts against the oriented
    width -- one that is too narrow raises ``ValueError`` before any launch.  It is the same in every entropy mode.
    ``host``: a ``HostHalf`` of ``bufs`` made before, on another thread say; its mode and chunk parameters are used."""
    if not torch.cuda.is_available():
        raise RuntimeError('the JPEG decoder reconstructs the pixels on the GPU through libyv4_hip.so (there is no CPU '
                           'fallback)')
    own = host is None      # no host half made ahead: its table half here, its Huffman decodes straight into the stage
    if own:
        host = HostHalf(bufs, entropy, chunk_bytes, max_rounds, run=False)
    mode = host.mode
    if orientation:
        _lib.require('jpeg_orientation', 'orientation=True')
    if mode != 'host':
        _lib.require('jpeg_sync' if mode == 'device_sync' else 'jpeg_entropy', f'entropy={mode!r}')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    L = _lib.lib()
    N = len(bufs)
    if own:
        host.tables()
    infos, scan, chunks = host.infos, host.scan, host.chunks
    table = (JpegImage * N)()
    totals = (C.c_int64 * 3)()
    if orientation:
        check(L.yv4_jpeg_layout_oriented(infos, N, 1, table, totals), 'yv4_jpeg_layout_oriented')
    else:
        check(L.yv4_jpeg_layout(infos, N, table, totals), 'yv4_jpeg_layout')
    ncoef, work_bytes, out_bytes = (int(t) for t in totals)
    if placement is not None:
        if out is None or out.dtype != torch.uint8 or not out.is_contiguous() or out.device.type != 'cuda':
            raise ValueError('placement needs out=: a contiguous torch.uint8 tensor on the GPU')
        out_bytes = out.numel()
        for n, (off, pitch) in enumerate(placement):
            table[n].out_off, table[n].out_pitch = int(off), int(pitch)
            if orientation and int(pitch) < 3 * oriented_size(table[n])[1]:      # before the scan decode's launch
                raise ValueError(f'imdecode: image {n}: pitch {int(pitch)} is narrower than its oriented row of '
                                 f'{3 * oriented_size(table[n])[1]} bytes')

    # one pinned staging buffer: [per-image table | quantisation tables | ...
    if scan is not None:      # ... scans | segments | workgroups | packed Huffman tables | the files | chunk tables]
        tail = scan.sections() + (chunks.sections() if chunks is not None else ())
    elif own:                 # ... coefficients int16], decoded in place
        tail = ((lambda p: _host_decode_all(bufs, infos, p, [t.coef_off for t in table], 'imdecode'), 2 * ncoef),)
    else:                     # ... coefficients int16], decoded ahead
        tail = ((lambda p: C.memmove(p, host.coef.ctypes.data, 2 * ncoef), 2 * ncoef),)
    stage, offs = _stage(((table, C.sizeof(table)), _quant_section(infos)) + tail)

    def reconstruct(coef_ptr):
        check(L.yv4_jpeg_reconstruct(table, up.data_ptr(), N, coef_ptr, ncoef, up.data_ptr() + offs[1],
                                     work.data_ptr(), work_bytes, out.data_ptr(), out_bytes,
                                     int(channel_order == 'rgb'), stream_ptr()), 'yv4_jpeg_reconstruct')

    status = undecided = None
    with torch.cuda.device(dev):
        up = stage.to(dev, non_blocking=True)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        if placement is None:
            out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        if scan is None:
            coef_ptr = up.data_ptr() + offs[2]
        else:
            coef = torch.empty(ncoef, dtype=torch.int16, device=dev)
            flags = torch.empty(2 * N, dtype=torch.int32, device=dev)      # status | undecided: one read-back
            status = flags[:N]
            d = [up.data_ptr() + o for o in offs[2:]]
            if chunks is None:
                _launch_segments(L, scan, d, N, coef, ncoef, status)
            else:
                undecided = flags[N:]
                entries = torch.empty(chunks.nchunk * C.sizeof(JpegEntry), dtype=torch.uint8, device=dev)
                _launch_sync(L, scan, chunks, d, N, host.max_rounds, entries, coef, ncoef, status, undecided)
            coef_ptr = coef.data_ptr()
        reconstruct(coef_ptr)
        if status is not None:
            codes = (flags if undecided is not None else status).cpu().tolist()      # the batch's one read-back
            again = [n for n in range(N) if codes[N + n]] if undecided is not None else []
            if again:
                # what the chunks did not prove: the one lane per segment kernel, a run of neighbouring images a launch
                # (it zero-fills from its first image's coefficients to its last's), then the pixels once more
                runs = [[again[0]]]
                for n in again[1:]:
                    if n == runs[-1][-1] + 1:
                        runs[-1].append(n)
                    else:
                        runs.append([n])
                for run in runs:
                    a, b = run[0], run[-1] + 1
                    sub = ScanTables(bufs[a:b], coef_offs=[int(scan.scans[n].coef_off) for n in run], what='imdecode')
                    jpeg_entropy_decode_device(bufs[a:b], dev, coef=coef, status=status[a:b], tables=sub)
                reconstruct(coef_ptr)
                codes = status.cpu().tolist()
            for n, code in enumerate(codes[:N]):
                if code:
                    raise ValueError(f'imdecode: image {n}: jpeg: ' + L.yv4_jpeg_entropy_strerror(code).decode())
    return out, table


def imdecode(buffers, channel_order='bgr', device=None, entropy=None, chunk_bytes=None, max_rounds=None,
             orientation=False):
    """``buffers``: the bytes of one JPEG file or a list of them -> a ``torch.uint8`` (h, w, 3) tensor on ``device``
    (default: the current GPU), or a list of them.  ``channel_order``: ``'bgr'`` (what ``mmcv.imread`` returns) or
    ``'rgb'``; a grayscale file gives its plane three times, like ``flag='color'``.  A list is decoded as one batch:
    the entropy decodes on a thread pool, then one upload and one reconstruct call -- or, with ``entropy='device'``, the
    files go up and a kernel decodes their scans, one lane per restart segment, or with ``entropy='device_sync'`` one lane
    per ``chunk_bytes`` of a segment after at most ``max_rounds`` synchronisation rounds (``decode_into``; ``None``:
    ``DEFAULT_ENTROPY``, which starts as ``'host'``).  ``orientation=True`` applies the EXIF orientation, as
    ``mmcv.imread(flag='color')`` does: the tensor is then (w, h, 3) for orientations 5 to 8.  The default leaves it
    alone."""
    if channel_order not in ('bgr', 'rgb'):
        raise ValueError(f"channel_order {channel_order!r} is not 'bgr' or 'rgb'")
    single = not isinstance(buffers, (list, tuple))
    bufs = [_as_bytes(b) for b in ([buffers] if single else buffers)]
    if not bufs:
        return []
    out, table = decode_into(bufs, channel_order, device, entropy=entropy, chunk_bytes=chunk_bytes, max_rounds=max_rounds,
                             orientation=orientation)
    imgs = image_views(out, table)
    return imgs[0] if single else imgs


def imread(paths, channel_order='bgr', device=None, entropy=None, chunk_bytes=None, max_rounds=None, orientation=False):
    """``paths``: a file name (``str`` / ``os.PathLike``) or a list of them -> what ``imdecode`` returns for their bytes."""
    single = not isinstance(paths, (list, tuple))
    bufs = []
    for p in ([paths] if single else paths):
        with open(os.fspath(p), 'rb') as f:
            bufs.append(f.read())
    return imdecode(bufs[0] if single else bufs, channel_order=channel_order, device=device, entropy=entropy,
                    chunk_bytes=chunk_bytes, max_rounds=max_rounds, orientation=orientation)


@PIPELINES.register_module()
class LoadImageFromFile:
    """``LoadImageFromFile`` of the reference's pipelines (``mmdet/datasets/pipelines/loading.py:12-86``): reads
    ``img_prefix`` / ``img_info['filename']`` and fills ``filename``, ``ori_filename``, ``img``, ``img_shape``,
    ``ori_shape`` and ``img_fields``.  ``img`` is a (h, w, 3) BGR tensor on the GPU -- ``torch.uint8``, or
    ``torch.float32`` with ``to_float32``.  ``im_decode_backend`` is accepted and ignored: every backend the reference
    offers for JPEG runs libjpeg-turbo's default decode, which is what ``imread`` computes.  ``color_type``: ``'color'`` or
    ``'color_ignore_orientation'``.  EXIF orientation is applied with ``apply_orientation=True`` and never with
    ``'color_ignore_orientation'``; the default is off (``mmcv.imread(flag='color')`` applies it: the training loader,
    ``datasets.build_train_loader``, turns it on for ``'color'``).  ``entropy``, ``chunk_bytes``, ``max_rounds``: where and how the
    Huffman scan is decoded (``imdecode``)."""

    def __init__(self, to_float32=False, color_type='color', file_client_args=dict(backend='disk'), im_decode_backend=None,
                 device=None, entropy=None, chunk_bytes=None, max_rounds=None, apply_orientation=False):
        if color_type not in ('color', 'color_ignore_orientation'):
            raise NotImplementedError(f"LoadImageFromFile(color_type={color_type!r}) is not built ('color' and "
                                      "'color_ignore_orientation' only)")
        if apply_orientation and color_type == 'color_ignore_orientation':
            raise ValueError("apply_orientation=True contradicts color_type='color_ignore_orientation'")
        if dict(file_client_args) != dict(backend='disk'):
            raise NotImplementedError(f'LoadImageFromFile(file_client_args={dict(file_client_args)!r}) is not built '
                                      "(dict(backend='disk') only)")
        self.to_float32 = to_float32
        self.color_type = color_type
        self.file_client_args = dict(file_client_args)
        self.im_decode_backend = im_decode_backend
        self.device = device
        self.apply_orientation = bool(apply_orientation)
        self.entropy = None if entropy is None else _entropy_mode(entropy)
        self.chunk_bytes = self.max_rounds = None
        if chunk_bytes is not None or max_rounds is not None:
            self.chunk_bytes, self.max_rounds = _sync_params(chunk_bytes, max_rounds)

    def __call__(self, results):
        if results['img_prefix'] is not None:
            filename = os.path.join(results['img_prefix'], results['img_info']['filename'])
        else:
            filename = results['img_info']['filename']
        img = imread(filename, device=self.device, entropy=self.entropy, chunk_bytes=self.chunk_bytes,
                     max_rounds=self.max_rounds, orientation=self.apply_orientation)
        if self.to_float32:
            img = img.float()
        results['filename'] = filename
        results['ori_filename'] = results['img_info']['filename']
        results['img'] = img
        results['img_shape'] = tuple(img.shape)
        results['ori_shape'] = tuple(img.shape)
        results['img_fields'] = ['img']
        return results

    def __repr__(self):
        return (f'{self.__class__.__name__}(to_float32={self.to_float32}, color_type={self.color_type!r}, '
                f'file_client_args={self.file_client_args})')


# ---- the other direction: pixels -> baseline JPEG files (include/yv4.h, "baseline JPEG encoding") ---------------------
#: ``subsampling=`` -> the luma sampling factors (chroma is 1x1); ``'gray'``: one component, for a (h, w) image
ENCODE_SAMPLINGS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'gray': (1, 1)}


class EncodeTable:
    """The host table of a JPEG encode (``yv4_jpeg_encode_layout``) for images of the given ``shapes`` -- ``(h, w, 3)``
    or ``(h, w)`` -- ``qualities`` and ``subsamplings`` (one value, or one per image): ``table`` (``JpegEncImage`` array,
    placed densely) and the batch's ``pixel_bytes``, ``ncoef``, ``work_bytes``, ``out_bytes``.  Needs no GPU.
    ``ValueError`` by name for a quality outside 1 .. 100, an unknown sampling, an empty image or a side above 65 535."""

    def __init__(self, shapes, quality=95, subsampling='420', what='imencode'):
        N = len(shapes)
        quals = list(quality) if isinstance(quality, (list, tuple)) else [quality] * N
        samps = list(subsampling) if isinstance(subsampling, (list, tuple)) else [subsampling] * N
        if len(quals) != N or len(samps) != N:
            raise ValueError(f'{what}: {N} images, {len(quals)} qualities and {len(samps)} samplings')
        self.table = (_lib.JpegEncImage * N)()
        self.subsamplings = []
        for n, (shape, q, s) in enumerate(zip(shapes, quals, samps)):
            shape = tuple(int(v) for v in shape)
            if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
                raise ValueError(f'{what}: image {n}: shape {shape} is not (h, w, 3) or (h, w)')
            if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 100:
                raise ValueError(f'{what}: image {n}: quality {q!r} is not an integer in 1 .. 100')
            if s not in ENCODE_SAMPLINGS:
                raise ValueError(f"{what}: image {n}: subsampling {s!r} is not '444', '422', '420' or 'gray'")
            if len(shape) == 2:
                s = 'gray'                      # a single plane is one component, whatever the batch's sampling says
            elif s == 'gray':
                raise ValueError(f"{what}: image {n}: subsampling 'gray' needs a (h, w) image, not {shape}")
            if shape[0] < 1 or shape[1] < 1:
                raise ValueError(f'{what}: image {n} is empty: shape {shape}')
            if shape[0] > 65535 or shape[1] > 65535:
                raise ValueError(f'{what}: image {n}: a side above 65535: shape {shape}')
            t = self.table[n]
            t.height, t.width, t.channels, t.quality = shape[0], shape[1], 1 if len(shape) == 2 else 3, int(q)
            t.hs, t.vs = ENCODE_SAMPLINGS[s]
            self.subsamplings.append(s)
        totals = (C.c_int64 * 6)()
        st = _lib.lib().yv4_jpeg_encode_layout(self.table, N, totals)
        if st != 0:
            _raise(st, what)
        self.pixel_bytes, self.ncoef, self.work_bytes, self.out_bytes = (int(v) for v in totals[:4])

    def __len__(self):
        return len(self.table)

    def work_region_bytes(self, n):
        """The bytes of image ``n``'s work region (csrc/jpeg_enc_core.h ``work_bytes``): two totals, the running sums of
        both grids' workgroups, the bits per block, the packed words of the bound."""
        nb, per = int(self.table[n].nblocks), _lib.JPEG_ENC_WG_BLOCKS
        words = ((nb * _lib.JPEG_ENC_BLOCK_BITS + 7) // 8 + 3) // 4
        return 16 + 8 * (-(-nb // per)) + 8 * (-(-words // per)) + 4 * ((nb + 1) & ~1) + 4 * ((words + 1) & ~1)

    def header(self, n):
        """SOI .. SOS of image ``n`` (``yv4_jpeg_encode_header``)."""
        buf = (C.c_uint8 * _lib.JPEG_ENC_HEADER_MAX)()
        length = C.c_int64()
        check(_lib.lib().yv4_jpeg_encode_header(C.byref(self.table[n]), C.addressof(buf), len(buf), C.byref(length)),
              'yv4_jpeg_encode_header')
        return bytes(buf[:length.value])

    def files(self, out, sizes, offsets=None):
        """The files of the batch from the scan bytes (``out``: a host uint8 array, ``sizes``: the byte counts; image n's
        bytes start at ``offsets[n]``, default: the table's ``out_off``)."""
        offs = [int(t.out_off) for t in self.table] if offsets is None else offsets
        return [self.header(n) + out[int(o):int(o) + int(sizes[n])].tobytes() + b'\xff\xd9' for n, o in enumerate(offs)]


def jpeg_encode_host(imgs, quality=95, subsampling='420', channel_order='bgr'):
    """The whole encoder on the CPU (``yv4_jpeg_encode_host``: the core the kernels run) -> ``(EncodeTable, int16
    coefficients, scan bytes of the batch, int64 sizes)``.  ``imgs``: numpy uint8 arrays.  Needs no GPU; for tests and
    tools -- ``imencode`` never takes this path."""
    imgs = [np.ascontiguousarray(a, np.uint8) for a in imgs]
    et = EncodeTable([a.shape for a in imgs], quality, subsampling, 'jpeg_encode_host')
    pix = np.zeros(max(et.pixel_bytes, 1), np.uint8)
    for t, a in zip(et.table, imgs):
        pix[int(t.src_off):int(t.src_off) + a.size] = a.reshape(-1)
    coef = np.empty(et.ncoef, np.int16)
    work = np.empty(et.work_bytes // 8 + 1, np.uint64)
    out = np.empty(et.out_bytes, np.uint8)
    sizes = np.empty(len(imgs), np.int64)
    check(_lib.lib().yv4_jpeg_encode_host(et.table, len(imgs), 3, pix.ctypes.data, pix.size, int(channel_order == 'rgb'),
                                          coef.ctypes.data, coef.size, work.ctypes.data, et.work_bytes, out.ctypes.data,
                                          out.size, sizes.ctypes.data), 'yv4_jpeg_encode_host')
    return et, coef, out, sizes


def encode_stages(et, pixels, channel_order='bgr', coef=None, work=None, out=None, sizes=None, stages=3):
    """The two device stages over a placed table: ``yv4_jpeg_encode_coefficients`` (``stages & 1``) and
    ``yv4_jpeg_encode_scan`` (``stages & 2``) on the current stream -> ``(coef, work, out, sizes)`` device tensors, nothing
    read back.  ``pixels``: the flat uint8 device buffer the table's ``src_off`` / ``src_pitch`` point into.  ``coef`` /
    ``work`` / ``out`` / ``sizes``: the caller's tensors (larger ones with the table's offsets moved, say); the library
    checks every region against their sizes before any launch."""
    _lib.require('jpeg_encode')
    L, N, dev = _lib.lib(), len(et), pixels.device
    with torch.cuda.device(dev):
        stage = torch.empty(C.sizeof(et.table), dtype=torch.uint8, pin_memory=True)
        C.memmove(stage.data_ptr(), et.table, C.sizeof(et.table))
        up = stage.to(dev, non_blocking=True)
        coef = torch.empty(et.ncoef, dtype=torch.int16, device=dev) if coef is None else coef
        if stages & 1:
            st = L.yv4_jpeg_encode_coefficients(et.table, up.data_ptr(), N, pixels.data_ptr(), pixels.numel(),
                                                int(channel_order == 'rgb'), coef.data_ptr(), coef.numel(), stream_ptr())
            if st != 0:
                _raise(st, 'yv4_jpeg_encode_coefficients')
        if stages & 2:
            work = torch.empty(et.work_bytes, dtype=torch.uint8, device=dev) if work is None else work
            out = torch.empty(et.out_bytes, dtype=torch.uint8, device=dev) if out is None else out
            sizes = torch.empty(N, dtype=torch.int64, device=dev) if sizes is None else sizes
            st = L.yv4_jpeg_encode_scan(et.table, up.data_ptr(), N, coef.data_ptr(), coef.numel(), work.data_ptr(),
                                        work.numel(), out.data_ptr(), out.numel(), sizes.data_ptr(), stream_ptr())
            if st != 0:
                _raise(st, 'yv4_jpeg_encode_scan')
    return coef, work, out, sizes


def _read_back(et, out, sizes):
    """The files of a finished encode.  Two read-backs: the N byte counts; then the scan bytes alone -- the images'
    exact slices of the bound-sized output gathered into one dense device buffer (``torch.cat``) and copied through
    pinned memory, ``sum(counts)`` bytes.  The unused part of every image's bound never leaves the device."""
    counts = sizes.cpu().numpy()
    dense = torch.cat([out[int(t.out_off):int(t.out_off) + int(c)] for t, c in zip(et.table, counts)])
    host = torch.empty(dense.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(dense)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return et.files(host.numpy(), counts, starts)


def encode_into(pixels, placement, quality=95, subsampling='420', channel_order='bgr'):
    """The batch encode behind ``imencode`` and ``imwrite``: images already lying in the flat ``torch.uint8`` device
    buffer ``pixels`` -> the list of their JPEG files (``bytes``).  ``placement``: per image ``(shape, byte offset, row
    pitch)`` -- or ``decode_into``'s ``JpegImage`` table, so that a decode -> draw -> encode chain never copies pixels.
    One call per stage for the whole batch, one read-back of the byte counts and one of the scan bytes, compacted on the
    device first (what crosses to the host is the files' size, not the bound the output buffer is sized by); the headers
    are written on the host."""
    if not torch.cuda.is_available() or pixels.device.type != 'cuda':
        raise RuntimeError('the JPEG encoder runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
    if channel_order not in ('bgr', 'rgb'):
        raise ValueError(f"channel_order {channel_order!r} is not 'bgr' or 'rgb'")
    if pixels.dtype != torch.uint8 or not pixels.is_contiguous():
        raise ValueError('pixels must be a contiguous torch.uint8 tensor')
    if isinstance(placement, C.Array) and placement._type_ is JpegImage:
        placement = [(oriented_size(t) + (3,), int(t.out_off), int(t.out_pitch)) for t in placement]
    et = EncodeTable([p[0] for p in placement], quality, subsampling)
    for t, (_, off, pitch) in zip(et.table, placement):
        t.src_off, t.src_pitch = int(off), int(pitch)
    with torch.cuda.device(pixels.device):
        _, _, out, sizes = encode_stages(et, pixels.view(-1), channel_order)
        return _read_back(et, out, sizes)


def imencode(imgs, quality=95, subsampling='420', channel_order='bgr', device=None):
    """``imgs``: one image or a list -- each a ``torch.uint8`` (h, w, 3) or (h, w) tensor on the GPU, or a numpy array of
    that shape, which is uploaded -> the bytes of its baseline JPEG file, or a list of them.  The file is what
    libjpeg-turbo writes for the same pixels: ``cv2.imwrite``'s at its defaults, quality 95 and 4:2:0, which are the
    defaults here.  ``quality`` (1 .. 100) and ``subsampling`` (``'444'``, ``'422'``, ``'420'``; a (h, w) image is always
    one gray component) may be lists, one value per image.  ``channel_order``: what the three channels are, ``'bgr'``
    (what ``imread`` returns) or ``'rgb'``.  A list is one batch: the images are placed in one flat device buffer (the
    host ones through one pinned upload of their own bytes), then one call per stage and the two read-backs of
    ``encode_into``."""
    if not torch.cuda.is_available():
        raise RuntimeError('the JPEG encoder runs on the GPU through libyv4_hip.so (there is no CPU fallback)')
    if channel_order not in ('bgr', 'rgb'):
        raise ValueError(f"channel_order {channel_order!r} is not 'bgr' or 'rgb'")
    single = not isinstance(imgs, (list, tuple))
    imgs = [imgs] if single else list(imgs)
    if not imgs:
        return []
    for n, a in enumerate(imgs):
        if not isinstance(a, (np.ndarray, torch.Tensor)) or (a.dtype != np.uint8 if isinstance(a, np.ndarray) else a.dtype != torch.uint8):
            raise ValueError(f'imencode: image {n} is not a uint8 array or tensor')
    et = EncodeTable([tuple(a.shape) for a in imgs], quality, subsampling)       # validates before any upload
    dev = torch.device(device) if device is not None else next(
        (a.device for a in imgs if isinstance(a, torch.Tensor) and a.device.type == 'cuda'),
        torch.device('cuda', torch.cuda.current_device()))
    with torch.cuda.device(dev):
        pixels = torch.empty(et.pixel_bytes, dtype=torch.uint8, device=dev)
        where = [(int(t.src_off), int(t.src_pitch) * int(t.height)) for t in et.table]
        hosts = [k for k, a in enumerate(imgs) if isinstance(a, np.ndarray)]
        if hosts:                                   # the host images back to back in one pinned buffer, one copy each
            stage = torch.empty(sum(where[k][1] for k in hosts), dtype=torch.uint8, pin_memory=True)
            at = 0
            for k in hosts:
                n = where[k][1]
                stage[at:at + n] = torch.from_numpy(np.ascontiguousarray(imgs[k]).reshape(-1))
                pixels[where[k][0]:where[k][0] + n].copy_(stage[at:at + n], non_blocking=True)
                at += n
        for (off, n), a in zip(where, imgs):
            if isinstance(a, torch.Tensor):
                pixels[off:off + n].view(a.shape).copy_(a)
        _, _, out, sizes = encode_stages(et, pixels, channel_order)
        files = _read_back(et, out, sizes)
    return files[0] if single else files


def _write_files(files, paths, auto_mkdir):
    def one(k):
        p = os.fspath(paths[k])
        if auto_mkdir and os.path.dirname(p):
            os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, 'wb') as f:
            f.write(files[k])

    if len(files) == 1:
        one(0)
    else:
        with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, len(files))) as pool:
            list(pool.map(one, range(len(files))))


def check_jpeg_paths(paths, what='imwrite'):
    """``NotImplementedError`` naming the format for a path that does not end in ``.jpg`` / ``.jpeg`` (any case)."""
    for p in paths:
        ext = os.path.splitext(os.fspath(p))[1]
        if ext.lower() not in ('.jpg', '.jpeg'):
            raise NotImplementedError(f'{what}: {os.fspath(p)!r}: the {ext.lstrip(".").upper() or "extensionless"} format is '
                                      'not built: the encoder writes baseline JPEG (.jpg / .jpeg) only')


def imwrite(imgs, paths, quality=95, subsampling='420', channel_order='bgr', auto_mkdir=True):
    """``mmcv.imwrite`` for JPEG: ``imencode`` of one image or a list (one batch), then the files written on at most
    ``MAX_DECODE_THREADS`` threads.  ``paths``: one file name or a list, each ending in ``.jpg`` / ``.jpeg``; the
    directories are made with ``auto_mkdir``.  Returns ``True``, as ``mmcv.imwrite`` does."""
    single = not isinstance(imgs, (list, tuple))
    imgs, paths = ([imgs], [paths]) if single else (list(imgs), list(paths))
    if len(imgs) != len(paths):
        raise ValueError(f'imwrite: {len(imgs)} images and {len(paths)} paths')
    check_jpeg_paths(paths)
    if imgs:
        _write_files(imencode(imgs, quality, subsampling, channel_order), paths, auto_mkdir)
    return True
