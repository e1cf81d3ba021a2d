"""The self-synchronising chunk decode of the Huffman scan without a GPU: the chunk tables
(``yv4_jpeg_chunks_build``) and the whole method -- synchronisation rounds, sums, checks, storing decode, second decode
of what is not proven -- run on the CPU by the core the kernels run (``yv4_jpeg_entropy_decode_sync``) against the host
decoder ``yv4_jpeg_entropy_decode``, the oracle."""
import ctypes

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -4
L = pkg._lib
MIN = L.JPEG_MIN_CHUNK_BYTES
#: enough rounds for every chain of the fixtures to close (a chain of c chunks closes after at most c - 1)
ALL_ROUNDS = L.JPEG_MAX_ROUNDS
NOISE = '72x80_444_noise_q100_rst1'


@pytest.fixture(scope='module')
def cases(golden):
    a, b = golden('jpeg'), golden('jpeg_entropy')
    valid = {str(n): a['jpg_' + str(n)].tobytes() for n in a['names']}
    valid.update({str(n): b['jpg_' + str(n)].tobytes() for n in b['names']})
    damaged = {str(n): (b['jpg_' + str(n)].tobytes(), int(b['status_' + str(n)])) for n in b['damaged']}
    return valid, damaged


@pytest.fixture(scope='module')
def oracle(cases):
    """name -> the host decoder's coefficients of every valid file, computed once"""
    return {name: _host(buf)[2] for name, buf in cases[0].items()}


def _host(buf):
    info = L.JpegInfo()
    st = L.lib().yv4_jpeg_parse(buf, len(buf), ctypes.byref(info))
    if st != OK:
        return st, info, None
    coef = np.empty(int(info.ncoef), np.int16)
    st = L.lib().yv4_jpeg_entropy_decode(buf, len(buf), ctypes.byref(info), coef.ctypes.data, coef.size)
    return st, info, coef


def _sync(buf, chunk_bytes, max_rounds):
    """-> (status class, result tuple of image_io.jpeg_entropy_decode_sync or None)"""
    try:
        r = image_io.jpeg_entropy_decode_sync([buf], chunk_bytes, max_rounds)
    except NotImplementedError:
        return UNSUPPORTED, None
    except ValueError:
        return INVALID, None
    return (INVALID if r[4][0] else OK), r


def _state(word):
    """a packed state -> (byte, bit, block index, k)"""
    return word >> 19, (word >> 16) & 7, (word >> 8) & 255, word & 255


def _blocks_in_scan_order(sc, sg):
    """(component, first coefficient) of every block of a segment, in the order the scan codes them"""
    nluma = sc.hs * sc.vs
    bw0 = sc.mcus_x * sc.hs
    nb0, nb1 = bw0 * sc.mcus_y * sc.vs, sc.mcus_x * sc.mcus_y
    out = []
    for mcu in range(sg.first_mcu, sg.first_mcu + sg.mcu_count):
        my, mx = divmod(mcu, sc.mcus_x)
        for bi in range(nluma):
            v, h = divmod(bi, sc.hs)
            out.append((0, 64 * ((my * sc.vs + v) * bw0 + mx * sc.hs + h)))
        for c in range(1, sc.ncomp):
            out.append((c, 64 * (nb0 + (c - 1) * nb1 + my * sc.mcus_x + mx)))
    return out


def _check_entry_table(name, t, ch, entries, want, fin):
    """The invariants of an accepted table: the chain closes, the block ordinals follow from the block counts and
    agree with the block index, the predictors are the host decoder's running DC at that block."""
    sc = t.scans[0]
    bpm = sc.hs * sc.vs + (2 if sc.ncomp == 3 else 0)
    for s, sg in enumerate(t.segs):
        blocks = _blocks_in_scan_order(sc, sg)
        first = 0
        for g in range(ch.seg_first[s], ch.seg_first[s + 1]):
            e, k = entries[g], ch.chunks[g]
            assert (k.image, k.seg, k.index, k.count) == (0, s, g - ch.seg_first[s], ch.seg_first[s + 1] - ch.seg_first[s])
            byte, bit, blk, zz = _state(e.entry)
            if k.index == 0:
                assert (byte, bit, blk, zz) == (sg.begin, 0, 0, 0), (name, s)
            else:
                assert entries[g - 1].exit[fin] == e.entry, (name, s, k.index)
                assert sg.begin <= byte <= sg.end      # (in front of the chunk only where the pass before ended at the padding)
            assert e.first_block == first and blk == first % bpm, (name, s, k.index)
            done = first + (1 if zz else 0)       # blocks whose DC term lies in front of the entry
            pred = [0, 0, 0]
            for comp, off in blocks[:done]:
                pred[comp] = int(want[off])
            assert list(e.pred) == pred, (name, s, k.index)
            first += e.nblk
        assert first == len(blocks) and entries[ch.seg_first[s + 1] - 1].exit[fin] & 0xFFFF == 0, (name, s)


def test_abi_exports_the_sync_entries():
    names = ('yv4_jpeg_chunks_build', 'yv4_jpeg_entropy_decode_sync', 'yv4_jpeg_entropy_decode_device_sync')
    assert set(names) == set(L.FEATURES['jpeg_sync'].symbols) and set(names) <= set(L.SIGNATURES)
    assert all(hasattr(L.lib(), n) for n in names) and L.has('jpeg_sync')
    assert L.lib().yv4_abi_version() == 8
    assert (ctypes.sizeof(L.JpegChunk), ctypes.sizeof(L.JpegEntry), ctypes.sizeof(L.JpegSegment)) == (16, 48, 40)
    assert L.JpegEntry.nblk.offset == 24 and L.JpegEntry.dc.offset == 32 and L.JpegEntry.pred.offset == 40


@pytest.mark.parametrize('chunk_bytes', [MIN, 16, 64, 256])
def test_every_file_equals_the_host_decoder_with_nothing_undecided(cases, oracle, chunk_bytes):
    for name, buf in cases[0].items():
        t, ch, entries, coef, status, undecided, rounds = image_io.jpeg_entropy_decode_sync([buf], chunk_bytes, ALL_ROUNDS)
        assert status[0] == 0 and undecided[0] == 0 and rounds < ALL_ROUNDS, (name, rounds)
        np.testing.assert_array_equal(coef, oracle[name], err_msg=name)
        _check_entry_table(name, t, ch, entries, oracle[name], ALL_ROUNDS & 1)


@pytest.mark.parametrize('chunk_bytes', [MIN, 16, 64, 256])
def test_without_rounds_every_multi_chunk_image_takes_the_second_decode(cases, oracle, chunk_bytes):
    for name, buf in cases[0].items():
        t, ch, entries, coef, status, undecided, rounds = image_io.jpeg_entropy_decode_sync([buf], chunk_bytes, 0)
        multi = ch.nchunk > t.nseg
        # a guess that happens to be the true state is accepted as what it is: only a chain that does not close is not
        closes = all(entries[g].entry == entries[g - 1].exit[0] for g in range(ch.nchunk) if ch.chunks[g].index)
        assert status[0] == 0 and rounds == 0 and bool(undecided[0]) == (multi and not closes), name
        np.testing.assert_array_equal(coef, oracle[name], err_msg=name)
    t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([cases[0][NOISE]], chunk_bytes, 0)
    assert undecided[0] != 0 and ch.nchunk > t.nseg


def test_one_round_on_the_noise_file(cases, oracle):
    """How many images converge in one round is reported, not asserted: the outcome is the host decoder's either way."""
    names = [n for n in cases[0] if 'noise_q100' in n]
    assert NOISE in names
    for chunk_bytes in (MIN, 16, 64, 256):
        converged = 0
        for name in names:
            _, _, _, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([cases[0][name]], chunk_bytes, 1)
            assert status[0] == 0
            np.testing.assert_array_equal(coef, oracle[name], err_msg=name)
            converged += int(undecided[0] == 0)
        print(f'chunk_bytes {chunk_bytes}, max_rounds 1: {converged} of {len(names)} quality-100 noise files converged')


def test_a_chunk_that_begins_on_the_zero_of_a_stuffed_pair(cases, oracle):
    buf = cases[0][NOISE]
    t = image_io.ScanTables([buf])
    assert sum(buf[i] == 0xFF and buf[i + 1] == 0 for i in range(t.segs[0].begin, len(buf) - 1)) == 198
    hits = {}
    for cb in range(MIN, 33):
        for s, sg in enumerate(t.segs):
            for i in range(1, -(-(sg.end - sg.begin) // cb)):
                at = sg.begin + i * cb
                if buf[at] == 0 and buf[at - 1] == 0xFF:
                    hits.setdefault(cb, []).append((s, i, at))
    assert hits
    for cb in list(hits)[:3]:
        t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([buf], cb, ALL_ROUNDS)
        assert status[0] == 0 and undecided[0] == 0
        np.testing.assert_array_equal(coef, oracle[NOISE])
        for s, i, at in hits[cb]:
            assert _state(entries[ch.seg_first[s] + i].entry)[0] != at      # never on the stuffed zero
    # the guess itself looks one byte back: with no round it starts behind the zero
    cb = next(iter(hits))
    s, i, at = hits[cb][0]
    t, ch, entries, *_ = image_io.jpeg_entropy_decode_sync([buf], cb, 0)
    assert _state(entries[ch.seg_first[s] + i].entry) == (at + 1, 0, 0, 0)


def test_a_chunk_in_which_no_symbol_starts(cases, oracle):
    found = 0
    for name in [n for n in cases[0] if 'noise_q100' in n]:
        t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([cases[0][name]], MIN, ALL_ROUNDS)
        assert status[0] == 0 and undecided[0] == 0
        np.testing.assert_array_equal(coef, oracle[name])
        for g in range(ch.nchunk):
            k, e = ch.chunks[g], entries[g]
            end = min(t.segs[k.seg].begin + (k.index + 1) * MIN, t.segs[k.seg].end)
            if k.index + 1 < k.count and _state(e.entry)[0] >= end:
                assert e.nblk == 0 and e.exit[0] == e.entry and list(e.dc) == [0, 0, 0]
                found += 1
    assert found > 0


def _single_segment_files(cases):
    out = []
    for name, buf in cases[0].items():
        t = image_io.ScanTables([buf])
        if t.nseg == 1:
            out.append((name, buf, t.segs[0].end - t.segs[0].begin))
    return out


def test_chunk_counts_that_must_be_hit(cases, oracle):
    """A last chunk of one byte, a segment of exactly one chunk, a segment of 65 chunks (one past a workgroup) and one
    of more than 128."""
    files = _single_segment_files(cases)
    seen = set()
    for name, buf, n in files:
        plans = {}
        for cb in range(MIN, min(n, 4096) + 1):
            if n % cb == 1 and n > cb:
                plans.setdefault('last chunk of one byte', cb)
            if -(-n // cb) == 65:
                plans.setdefault('65 chunks', cb)
        if MIN <= n:
            plans['exactly one chunk'] = n
        if n > 128 * MIN:
            plans['more than 128 chunks'] = MIN
        for what, cb in plans.items():
            if what in seen and what != 'exactly one chunk':
                continue
            t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([buf], cb, ALL_ROUNDS)
            assert status[0] == 0 and undecided[0] == 0, (name, what)
            np.testing.assert_array_equal(coef, oracle[name], err_msg=f'{name}: {what}')
            want = {'last chunk of one byte': ch.nchunk == n // cb + 1, '65 chunks': ch.nchunk == 65 and ch.nwg == 2,
                    'exactly one chunk': ch.nchunk == 1, 'more than 128 chunks': ch.nchunk > 128 and ch.nwg > 2}[what]
            assert want, (name, what, ch.nchunk)
            seen.add(what)
    assert seen == {'last chunk of one byte', '65 chunks', 'exactly one chunk', 'more than 128 chunks'}


def test_restart_files_chunk_every_segment_on_its_own(cases, oracle):
    names = [n for n in cases[0] if '_rst' in n]
    assert len(names) >= 5
    for name in names:
        for cb in (MIN, 16):
            t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([cases[0][name]], cb, ALL_ROUNDS)
            assert t.nseg > 1 and status[0] == 0 and undecided[0] == 0, name
            np.testing.assert_array_equal(coef, oracle[name], err_msg=name)
            for s, sg in enumerate(t.segs):      # each segment starts anew: true state, predictors zero
                e = entries[ch.seg_first[s]]
                assert _state(e.entry) == (sg.begin, 0, 0, 0) and list(e.pred) == [0, 0, 0] and e.first_block == 0
                assert ch.seg_first[s + 1] - ch.seg_first[s] == max(1, -(-(sg.end - sg.begin) // cb))


def test_a_batch_equals_the_single_files(cases, oracle):
    names = list(cases[0])[::7] + ['72x80_444_grad_q90_rst1', '8x8_gray_block_q90', NOISE]
    for rounds in (0, 2, ALL_ROUNDS):
        t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([cases[0][n] for n in names], 16, rounds)
        assert not status.any() and (rounds != ALL_ROUNDS or not undecided.any())
        for n, sc in zip(names, t.scans):
            np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], oracle[n], err_msg=n)
        at = 0
        for w in ch.wgs:      # runs of at most 64 chunks of one image tile the table
            assert w.first_seg == at and 1 <= w.count <= 64 and {ch.chunks[g].image for g in range(at, at + w.count)} == {w.image}
            assert w.count == 64 or at + w.count == ch.nchunk or ch.chunks[at + w.count].image == w.image + 1
            at += w.count
        assert at == ch.nchunk


def test_damaged_files_end_with_the_host_decoders_class(cases):
    valid, damaged = cases
    for name, (buf, recorded) in damaged.items():
        assert _host(buf)[0] == recorded == INVALID
        for cb in (MIN, 64):
            assert _sync(buf, cb, None)[0] == INVALID, name
    for name, code in (('cut_last', 1), ('inserted', 5)):      # what only the bits show: the second decode's code
        r = image_io.jpeg_entropy_decode_sync([valid['8x8_gray_block_q90'], damaged[name][0], valid[NOISE]], 16, ALL_ROUNDS)
        assert list(r[4]) == [0, code, 0] and r[5][1] != 0 and r[5][0] == 0 and r[5][2] == 0
        sc = r[0].scans[2]
        np.testing.assert_array_equal(r[3][sc.coef_off:sc.coef_off + sc.ncoef], _host(valid[NOISE])[2])


def test_every_prefix_and_scan_byte_flip_gives_the_host_decoders_class(cases):
    valid = cases[0]
    seen, fallbacks = set(), 0
    for name in ('17x33_420_grad_q90_rst2', '9x7_420_grad_q90'):
        buf = valid[name]
        scan = _host(buf)[1].scan_offset
        variants = [buf[:n] for n in range(len(buf))]
        for off in range(scan, len(buf)):
            b = bytearray(buf)
            b[off] ^= 1 << (off & 7)
            variants.append(bytes(b))
        for v in variants:
            st, _, want = _host(v)
            for cb in (MIN, 16):
                got_st, r = _sync(v, cb, None)
                assert got_st == st, (name, len(v), cb)
                if st == OK:
                    np.testing.assert_array_equal(r[3], want)
                if r is not None:
                    fallbacks += int(r[5][0] != 0)
            seen.add(st)
    assert seen == {OK, INVALID}
    print(f'{fallbacks} of the variants took the second decode')


def test_bad_parameters_and_tables_are_refused_before_anything_is_decoded(cases):
    valid = cases[0]
    bufs = [valid['72x80_444_grad_q90_rst1'], valid['17x33_gray_grad_q90'], valid[NOISE]]
    t = image_io.ScanTables(bufs)
    lib, err = L.lib(), L.lib().yv4_last_error
    nchunk, nwg = ctypes.c_int64(), ctypes.c_int64()

    def build(cb, chunks=None, cap=0, first=None, wgs=None, wcap=0):
        return lib.yv4_jpeg_chunks_build(ctypes.addressof(t.scans), ctypes.addressof(t.segs), 3, t.nseg, cb,
                                         chunks, cap, first, wgs, wcap, ctypes.byref(nchunk), ctypes.byref(nwg))

    for cb in (0, -1, MIN - 1, L.JPEG_MAX_CHUNK_BYTES + 1):
        assert build(cb) == INVALID and b'chunk_bytes' in err()
        with pytest.raises(ValueError, match='chunk_bytes'):
            image_io.jpeg_entropy_decode_sync(bufs, cb, 1)
    for mr in (-1, L.JPEG_MAX_ROUNDS + 1, 1.5, 'x', True):
        with pytest.raises(ValueError, match='max_rounds'):
            image_io.jpeg_entropy_decode_sync(bufs, 16, mr)
    assert build(16) == OK and nchunk.value > t.nseg
    n, w = nchunk.value, nwg.value
    chunks, first, wgs = (L.JpegChunk * n)(), (ctypes.c_int32 * (t.nseg + 1))(), (L.JpegWg * w)()
    ptr = ctypes.addressof
    assert build(16, ptr(chunks), n - 1, ptr(first), ptr(wgs), w) == CAPACITY
    assert build(16, ptr(chunks), n, ptr(first), ptr(wgs), w - 1) == CAPACITY
    assert build(16, ptr(chunks), n, None, ptr(wgs), w) == INVALID

    good = image_io.ChunkTables(t, 16)
    fake = ctypes.c_void_p(1 << 20)             # never dereferenced: validation returns first

    def call(c, cb=16, mr=4, nchunk=good.nchunk, nwg=good.nwg, scan=t):
        return lib.yv4_jpeg_entropy_decode_device_sync(
            ptr(scan.scans), ptr(scan.segs), ptr(c.chunks), ptr(c.seg_first), ptr(c.wgs), fake, fake, fake, fake, fake, 3,
            scan.nseg, nchunk, nwg, fake, scan.nbytes, fake, scan.nhuff, cb, mr, fake, fake, scan.ncoef, fake, fake, None)

    assert call(good, cb=MIN - 1) == INVALID and b'chunk_bytes' in err()
    assert call(good, mr=-1) == INVALID and b'max_rounds' in err()
    assert call(good, mr=L.JPEG_MAX_ROUNDS + 1) == INVALID
    assert call(good, cb=32) == INVALID                      # tables built for another chunk size
    assert call(good, nchunk=good.nchunk - 1) == INVALID and call(good, nwg=good.nwg + 1) == INVALID
    for where, index, field, val in (('chunks', 0, 'image', 1), ('chunks', 1, 'seg', 1), ('chunks', 1, 'index', 0),
                                     ('chunks', 0, 'count', 99), ('chunks', good.nchunk - 1, 'index', 0),
                                     ('wgs', 0, 'count', 65), ('wgs', 0, 'first_seg', 1), ('wgs', 1, 'image', 2),
                                     ('wgs', good.nwg - 1, 'count', 0)):
        bad = image_io.ChunkTables(t, 16)
        setattr(getattr(bad, where)[index], field, val)
        assert call(bad) == INVALID, (where, index, field, val)
    for index in (0, 1, t.nseg):
        bad = image_io.ChunkTables(t, 16)
        bad.seg_first[index] += 1
        assert call(bad) == INVALID, index
    for where, field, val in (('scans', 'data_len', 1 << 40), ('scans', 'coef_off', 32), ('scans', 'nseg', 91),
                              ('segs', 'end', 1 << 20), ('segs', 'begin', -1), ('segs', 'mcu_count', 2),
                              ('segs', 'bit_off', 3)):
        bad = image_io.ScanTables(bufs)
        setattr(getattr(bad, where)[0], field, val)
        assert call(good, scan=bad) == INVALID, (where, field, val)
    # the CPU run validates the same way, before it writes anything
    coef = np.full(t.ncoef, 0x5a5a, np.int16)
    flags = np.full(6, -7, np.int32)
    entries = (L.JpegEntry * good.nchunk)()
    bad = image_io.ChunkTables(t, 16)
    bad.chunks[5].index = 0
    data = np.zeros(t.nbytes, np.uint8)
    t.write_bytes(data.ctypes.data)
    assert lib.yv4_jpeg_entropy_decode_sync(
        ptr(t.scans), ptr(t.segs), ptr(bad.chunks), ptr(bad.seg_first), ptr(bad.wgs), 3, t.nseg, bad.nchunk, bad.nwg,
        data.ctypes.data, t.nbytes, ptr(t.huff), t.nhuff, 16, 4, ptr(entries), coef.ctypes.data, coef.size,
        flags.ctypes.data, flags.ctypes.data + 12, None) == INVALID
    assert (coef == 0x5a5a).all() and (flags == -7).all()


def test_entropy_setting_and_arguments():
    assert image_io.DEFAULT_ENTROPY == 'host'
    assert pkg.set_default_entropy('device_sync') == 'host' and image_io.DEFAULT_ENTROPY == 'device_sync'
    assert pkg.set_default_entropy('host') == 'device_sync' and image_io.DEFAULT_ENTROPY == 'host'
    with pytest.raises(ValueError, match='entropy'):
        pkg.set_default_entropy('device_async')
    with pytest.raises(ValueError, match='entropy'):
        pkg.LoadImageFromFile(entropy='sync')
    load = pkg.PIPELINES.build(dict(type='LoadImageFromFile', entropy='device_sync', chunk_bytes=64, max_rounds=3))
    assert (load.entropy, load.chunk_bytes, load.max_rounds) == ('device_sync', 64, 3)
    assert pkg.LoadImageFromFile(entropy='device_sync').chunk_bytes is None
    with pytest.raises(ValueError, match='chunk_bytes'):
        pkg.LoadImageFromFile(entropy='device_sync', chunk_bytes=MIN - 1)
    with pytest.raises(ValueError, match='max_rounds'):
        pkg.LoadImageFromFile(entropy='device_sync', max_rounds=-1)
    assert image_io._sync_params(None, None) == (image_io.DEFAULT_CHUNK_BYTES, image_io.DEFAULT_MAX_ROUNDS)
    assert MIN <= image_io.DEFAULT_CHUNK_BYTES <= L.JPEG_MAX_CHUNK_BYTES and 0 < image_io.DEFAULT_MAX_ROUNDS <= L.JPEG_MAX_ROUNDS
