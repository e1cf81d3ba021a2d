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
    if status == -2:
        raise NotImplementedError(f'{what}: {msg}')
    if status == -1:
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


def _need(have, symbol, what=None):
    """``RuntimeError`` unless the loaded library exports ``symbol``, which ``what`` (an argument as written) asks for."""
    if not have:
        why = f'{symbol} is not exported by the loaded libyv4_hip.so' if what is None else \
            f'{what} needs {symbol}, which the loaded libyv4_hip.so does not export (there is no fallback)'
        raise RuntimeError(why + ': rebuild it')


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
    _need(_lib.has_jpeg_sync(), 'yv4_jpeg_entropy_decode_device_sync')
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
    _need(not orientation or _lib.has_jpeg_orientation(), 'yv4_jpeg_layout_oriented', 'orientation=True')
    _need(mode == 'host' or _lib.has_jpeg_entropy(), 'yv4_jpeg_entropy_decode_device', "entropy='device'")
    _need(mode != 'device_sync' or _lib.has_jpeg_sync(), 'yv4_jpeg_entropy_decode_device_sync', "entropy='device_sync'")
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
