"""A baseline JPEG writer for streams that no encoder writes: the second, independent witness of the JPEG decoders.

Pure Python / numpy, and it shares no code with ``_jpeg_ref.py`` (it keeps its own zigzag literal; a host test holds the
two equal).  ``write`` takes coefficient planes in the decoder's own layout -- int16, natural order, one plane of blocks
per component over the MCU-padded grid, the planes concatenated: what ``_jpeg_ref.entropy_decode`` returns -- together
with quantisation tables, Huffman tables given as ``{symbol: code length}`` per (class, slot) and the selectors, and
returns the file's bytes and the coefficients a decoder has to produce.  So the ground truth of every case is what was
written, not what another decoder read.

``CASES`` maps a name to a builder of ``write``'s arguments, ``INVALID`` a name to (builder, the ``YV4_JPEG_ERR_*`` code
the file has to end with).  Every case is seeded and at most 48x64 pixels, with three exceptions: the basis files
(64x128, 128 blocks: coefficient k alone at +A and -A) and ``rst_1_gray`` (8x520: a restart interval of one MCU gives
more than 64 segments only with more than 64 blocks).

Table helpers (a table's dict order is the order of the symbols within a length, so it decides the codes):
  unary     symbol i at length i + first: with 16 symbols from length 1 every length 1..16 carries one code, each a run
            of ones ending in 0 -- the only shape a table with a code at every length can have (``deep``)
  flat      every symbol at one length; what does not fit below the all-ones code goes to the next length
  at_length one symbol at exactly length L, the shorter lengths filled so that its code is L - 1 ones and a 0 (``ones``)
"""
import math

import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63)
SAMPLINGS = {'gray': (1, 1, 1), '444': (3, 1, 1), '422': (3, 2, 1), '420': (3, 2, 2)}      # components, luma h, luma v
EOB, ZRL = 0x00, 0xF0
ERR_CODE, ERR_DC_CATEGORY, ERR_INDEX = 2, 3, 4      # YV4_JPEG_ERR_* of include/yv4.h


class Layout:
    """The block grid of a picture: per component ``bw`` / ``bh`` / ``off`` (first block of its plane in the flat block
    list), ``nblocks``, and ``order``: the flat block index of every block in the order the scan codes them, ``bpm`` per
    MCU."""

    def __init__(self, width, height, sampling):
        self.width, self.height, self.sampling = width, height, sampling
        self.ncomp, self.hs, self.vs = SAMPLINGS[sampling]
        self.mx, self.my = -(-width // (8 * self.hs)), -(-height // (8 * self.vs))
        f = [(self.hs, self.vs)] + [(1, 1)] * (self.ncomp - 1)
        self.bw = [self.mx * h for h, _ in f]
        self.bh = [self.my * v for _, v in f]
        self.off = [0]
        for i in range(self.ncomp):
            self.off.append(self.off[-1] + self.bw[i] * self.bh[i])
        self.nblocks = self.off[-1]
        self.bpm = self.hs * self.vs + self.ncomp - 1
        self.order, self.comp = [], []
        for y in range(self.my):
            for x in range(self.mx):
                for i, (h, v) in enumerate(f):
                    for b in range(v):
                        for a in range(h):
                            self.order.append(self.off[i] + (y * v + b) * self.bw[i] + x * h + a)
                            self.comp.append(i)

    def visible(self, i):
        """(rows, columns) of real samples of component i: what the picture covers, not the MCU padding"""
        if i == 0:
            return self.height, self.width
        return -(-self.height // self.vs), -(-self.width // self.hs)


def canonical(lengths):
    """{symbol: length} -> (16 counts, values, {symbol: (length, code)}): canonical codes, shortest first, symbols of one
    length in the dict's order.  The Kraft sum holds and no code is all ones."""
    items = sorted(lengths.items(), key=lambda kv: kv[1])      # stable: the dict's order within a length
    assert items and len(items) <= 256 and all(1 <= n <= 16 and 0 <= s <= 255 for s, n in items)
    counts, vals, codes, code, at = [0] * 16, [], {}, 0, 1
    for sym, n in items:
        code <<= n - at
        at = n
        assert code < (1 << n) - 1, f'symbol {sym:#x}: no code of length {n} below the all-ones code is left'
        codes[sym] = (n, code)
        counts[n - 1] += 1
        vals.append(sym)
        code += 1
    assert sum(c * 2.0 ** -(i + 1) for i, c in enumerate(counts)) < 1.0
    return counts, vals, codes


def unary(symbols, first=1):
    """symbol i at length first + i"""
    return {s: first + i for i, s in enumerate(symbols)}


def flat(symbols, length):
    """every symbol at ``length``; the ones that do not fit below the all-ones code at ``length + 1``"""
    # a codes of ``length`` and b of the next: 2 a + b <= 2^(length + 1) - 1 keeps the all-ones code free
    spill = max(0, 2 * len(symbols) - (2 << length) + 1)
    assert spill <= len(symbols)
    return {s: length if i < len(symbols) - spill else length + 1 for i, s in enumerate(symbols)}


def at_length(target, length, others):
    """``target`` at exactly ``length`` with the code 1..10: ``others`` fill the lengths below one by one, the next of
    them follows at ``length + 1``"""
    t = unary(others[:length - 1])
    t[target] = length
    if length < 16 and len(others) >= length:
        t[others[length - 1]] = length + 1
    return t


class _Bits:
    """MSB-first bits into bytes, a 0x00 stuffed behind every 0xFF"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        assert 0 <= value < 1 << nbits
        for i in range(nbits - 1, -1, -1):
            self.acc = (self.acc << 1) | ((value >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc = self.n = 0

    def flush(self, pad):
        while self.n:
            self.put(pad, 1)


def _magnitude(v):
    """-> (size, the size's bits): T.81 F.1.2.1"""
    s = abs(v).bit_length()
    return s, (v if v > 0 else v + (1 << s) - 1)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def _wrap16(v):
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def write(width, height, sampling, coef, quant, tq, huff, td, ta, sof=0xC0, restart=0, dc_diffs=None, zrl_eob=0, fill=None,
          dht='joined', decoy=None, pad=1, override=None):
    """-> (file bytes, expected int16 coefficients).

    coef       flat int16 coefficients (see the module's docstring)
    quant      {slot: 64 entries in natural order, 1..255}; tq: slot per component
    huff       {(class, slot): {symbol: length}}; td / ta: slot per component
    sof        0xC0 or 0xC1;  restart: the restart interval in MCUs, 0 for none
    dc_diffs   one DC difference per block (flat, in the planes' layout) written instead of the differences of coef's DC
               terms; the expected DC term is then the running sum reduced to int16, as libjpeg keeps it
    zrl_eob    this many ZRL symbols in front of every EOB that leaves room for them
    fill       {restart marker ordinal: number of 0xFF fill bytes in front of it}
    dht        'joined': one DHT segment holding all tables; 'split': one per table
    decoy      {(class, slot): {symbol: length}}: a first definition of the table, written before the real one
    pad        the bit that pads a segment to the byte boundary
    override   {ordinal of a block in scan order: [('dc' | 'ac', symbol, bits, nbits) | ('raw', bits, nbits), ...]}: the
               block's symbols as given, for files that must not decode; expected is then None
    """
    lay = Layout(width, height, sampling)
    coef = np.asarray(coef, np.int16).reshape(lay.nblocks, 64)
    expected = coef.copy()
    assert sof in (0xC0, 0xC1) and dht in ('joined', 'split') and len(tq) == len(td) == len(ta) == lay.ncomp
    out = bytearray(b'\xff\xd8')
    body = bytearray()
    for slot, q in sorted(quant.items()):
        q = [int(v) for v in q]
        assert len(q) == 64 and all(1 <= v <= 255 for v in q) and 0 <= slot <= 3
        body += bytes([slot]) + bytes(q[ZIGZAG[k]] for k in range(64))
    out += _segment(0xDB, body)
    frame = bytes([8]) + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + bytes([lay.ncomp])
    for i in range(lay.ncomp):
        frame += bytes([i + 1, (lay.hs << 4 | lay.vs) if i == 0 else 0x11, tq[i]])
    out += _segment(sof, frame)
    codes, tables = {}, []
    for stage in (decoy or {}, huff):
        for (cls, slot), lengths in sorted(stage.items()):
            counts, vals, c = canonical(lengths)
            tables.append(bytes([cls << 4 | slot]) + bytes(counts) + bytes(vals))
            if stage is huff:
                codes[(cls, slot)] = c
    if dht == 'joined':
        out += _segment(0xC4, b''.join(tables))
    else:
        for t in tables:
            out += _segment(0xC4, t)
    if restart:
        out += _segment(0xDD, restart.to_bytes(2, 'big'))
    scan = bytes([lay.ncomp])
    for i in range(lay.ncomp):
        scan += bytes([i + 1, td[i] << 4 | ta[i]])
    out += _segment(0xDA, scan + bytes([0, 63, 0]))

    bits, pred, marker = _Bits(), [0] * lay.ncomp, 0

    def put(cls, comp, sym, value=0, nbits=0):
        n, code = codes[(cls, (ta if cls else td)[comp])][sym]
        bits.put(code, n)
        if nbits:
            bits.put(value, nbits)

    zrl_used = 0
    for ordinal, (b, comp) in enumerate(zip(lay.order, lay.comp)):
        if restart and ordinal and ordinal % (restart * lay.bpm) == 0:
            bits.flush(pad)
            bits.out += b'\xff' * (fill or {}).get(marker, 0) + bytes([0xFF, 0xD0 + (marker & 7)])
            marker += 1
            pred = [0] * lay.ncomp
        if override and ordinal in override:
            for item in override[ordinal]:
                if item[0] == 'raw':
                    bits.put(item[1], item[2])
                else:
                    put(int(item[0] == 'ac'), comp, *item[1:])
            continue
        if dc_diffs is None:
            d = int(coef[b, 0]) - pred[comp]
            pred[comp] = int(coef[b, 0])
        else:
            d = int(dc_diffs[b])
            pred[comp] = _wrap16(pred[comp] + d)
            expected[b, 0] = pred[comp]
        s, m = _magnitude(d)
        assert s <= 11, f'DC difference {d} of block {b}'
        put(0, comp, s, m, s)
        zz = [int(coef[b, ZIGZAG[k]]) for k in range(64)]
        last = max((k for k in range(1, 64) if zz[k]), default=0)
        run = 0
        for k in range(1, last + 1):
            if zz[k] == 0:
                run += 1
                continue
            while run > 15:
                put(1, comp, ZRL)
                run -= 16
            s, m = _magnitude(zz[k])
            assert s <= 15, f'AC term {zz[k]}'
            put(1, comp, run << 4 | s, m, s)
            run = 0
        if last < 63:
            for _ in range(zrl_eob):
                if last + 1 + 16 <= 63:      # behind the ZRL the index is still below 64: the EOB is read
                    put(1, comp, ZRL)
                    last += 16
                    zrl_used += 1
            put(1, comp, EOB)
    assert not zrl_eob or zrl_used
    assert not fill or all(0 <= m < marker for m in fill)
    bits.flush(pad)
    return bytes(out) + bytes(bits.out) + b'\xff\xd9', (None if override else expected.reshape(-1))


# ---- coefficient generators -------------------------------------------------------------------------------------------

def _value(rng, s, sign=None, largest=False):
    v = (1 << s) - 1 if largest else int(rng.integers(1 << (s - 1), 1 << s))
    return v if (sign if sign is not None else rng.integers(2)) else -v


def generate(rng, lay, dc_cats, ac_syms, restart=0, largest=False):
    """Coefficients whose coding uses the given alphabets: ``dc_cats`` / ``ac_syms`` hold one list per component, walked
    round-robin (a symbol that does not fit into the block is skipped; EOB in the list ends the block early).  The sign
    of a DC difference pulls the running value towards zero, so it never leaves int16.  ``largest``: every magnitude is
    2^s - 1."""
    coef = np.zeros((lay.nblocks, 64), np.int16)
    pred, at_dc, at_ac = [0] * lay.ncomp, [0] * lay.ncomp, [0] * lay.ncomp
    for ordinal, (b, c) in enumerate(zip(lay.order, lay.comp)):
        if restart and ordinal % (restart * lay.bpm) == 0:
            pred = [0] * lay.ncomp
        s = dc_cats[c][at_dc[c] % len(dc_cats[c])]
        at_dc[c] += 1
        if s:
            pred[c] += _value(rng, s, sign=pred[c] <= 0, largest=largest)
        coef[b, 0] = pred[c]
        syms, k = ac_syms[c], 1
        terms = [x for x in syms if x not in (EOB, ZRL)]
        while k < 64 and terms:
            for _ in range(len(syms)):
                sym = syms[at_ac[c] % len(syms)]
                at_ac[c] += 1
                skip = 0
                if sym == ZRL:      # a ZRL needs a term behind it: the next one of the list
                    skip, sym = 16, terms[int(rng.integers(len(terms)))]
                if sym == EOB or k + skip + (sym >> 4) <= 63:
                    break
            else:
                break
            if sym == EOB:
                break
            k += skip + (sym >> 4)
            coef[b, ZIGZAG[k]] = _value(rng, sym & 15, largest=largest)
            k += 1
    return coef.reshape(-1)


def _dct_matrix():
    return np.array([[math.sqrt((1 if u == 0 else 2) / 8) * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
                     for u in range(8)])


def from_samples(planes):
    """Level-shifted sample planes (one (bh * 8, bw * 8) float array per component) -> flat coefficients for tables of
    all ones: the rounded forward DCT of every block."""
    m, out = _dct_matrix(), []
    for p in planes:
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        out.append(np.rint(m @ blocks @ m.T).astype(np.int16).reshape(-1))
    return np.concatenate(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------

Q1 = [1] * 64
DC_PLAIN = unary([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
AC_SMALL = {EOB: 2, 0x01: 2, 0x02: 3, 0x11: 3, 0x03: 4, ZRL: 5, 0x21: 5}
#: sixteen AC symbols, one per length 1..16
AC_DEEP = [0x01, EOB, 0x02, 0x11, 0x03, 0x21, 0x12, 0x31, 0x04, 0x41, ZRL, 0x51, 0x22, 0x13, 0x61, 0x05]
AC_DEEP2 = [EOB, 0x11, 0x01, 0x21, 0x02, 0x12, 0x31, 0x03, ZRL, 0x41, 0x04, 0x22, 0x71, 0x13, 0x05, 0x81]
AC_OTHERS = [EOB, 0x02, 0x11, 0x03, 0x12, 0x21, 0x04, 0x31, 0x13, 0x41, 0x22, 0x05, 0x51, 0x14, 0x61]
DC_OTHERS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def _base(w, h, sampling, coef, huff, **kw):
    n = SAMPLINGS[sampling][0]
    args = dict(width=w, height=h, sampling=sampling, coef=coef, quant={0: Q1}, tq=[0] * n, huff=huff,
                td=[0, 1, 1][:n], ta=[0, 1, 1][:n])
    args.update(kw)
    return args


def _len_dc(L):
    def build():
        coef = np.zeros((2, 64), np.int16)
        coef[:, 0] = (5, -1)                        # differences +5 and -6: category 3 both times
        coef[0, 1], coef[1, 8] = 2, -1
        return _base(16, 8, 'gray', coef, {(0, 0): at_length(3, L, DC_OTHERS), (1, 0): AC_SMALL})
    return build


def _len_ac(L):
    def build():
        rng = _rng(f'len_ac_{L}')
        coef = np.zeros((2, 64), np.int16)
        coef[0, 1:] = rng.choice([-1, 1], 63)       # 63 times the symbol 0x01, no EOB
        coef[1, [ZIGZAG[k] for k in range(1, 41)]] = rng.choice([-1, 1], 40)
        coef[:, 0] = (3, -2)
        return _base(16, 8, 'gray', coef, {(0, 0): DC_PLAIN, (1, 0): at_length(0x01, L, AC_OTHERS)})
    return build


def _look_9_10():
    rng = _rng('look_9_10')
    lay = Layout(64, 48, 'gray')
    wide = [r << 4 | s for s in range(1, 6) for r in range(14)]
    table = {EOB: 2, ZRL: 2, 0xE1: 3}
    table.update({s: 9 for s in wide[:40]})
    table.update({s: 10 for s in wide[40:]})
    # the last code of length 9 and the first of length 10 come first, so that no statistic can leave them out
    alphabet = [wide[39], wide[40]] + wide + [EOB]
    return _base(64, 48, 'gray', generate(rng, lay, [[0, 2, 4, 6]], [alphabet]), {(0, 0): DC_PLAIN, (1, 0): table})


def _deep(sampling):
    def build():
        rng = _rng('deep_' + sampling)
        lay = Layout(33, 17, sampling)
        huff = {(0, 0): unary(range(12)), (1, 0): unary(AC_DEEP)}
        dc, ac = [list(range(12))], [AC_DEEP]
        if lay.ncomp == 3:      # chroma: DC codes of length 5..16, another order of the AC symbols
            huff.update({(0, 1): unary(range(12), 5), (1, 1): unary(AC_DEEP2)})
            # six chroma blocks per plane at 4:2:0: the two planes share the categories between them
            dc, ac = dc + [dc[0][::-1], dc[0][5::-1] + dc[0][:5:-1]], ac + [AC_DEEP2] * 2
        quant = {0: [1 + (k % 3) for k in range(64)]}
        return _base(33, 17, sampling, generate(rng, lay, dc, ac), huff, quant=quant)
    return build


def _flat8_444():
    rng = _rng('flat8_444')
    lay = Layout(40, 24, '444')
    syms = [r << 4 | s for s in range(1, 5) for r in range(16)] + [EOB, ZRL]
    huff = {(0, 0): flat(list(range(12)), 8), (1, 0): flat(syms, 8), (0, 1): flat(list(range(12)), 9), (1, 1): flat(syms, 9)}
    cats = [[0, 1, 2, 3, 4, 5, 6, 7, 8]] * 3
    return _base(40, 24, '444', generate(rng, lay, cats, [syms] * 3), huff)


def _single_gray():
    lay = Layout(33, 17, 'gray')
    return _base(33, 17, 'gray', np.zeros(lay.nblocks * 64, np.int16), {(0, 0): {0: 1}, (1, 0): {EOB: 1}})


def _sym256_ac():
    rng = _rng('sym256_ac')
    lay = Layout(64, 48, 'gray')
    used = [r << 4 | s for s in range(1, 5) for r in range(16)] + [EOB, ZRL]
    table = flat(used + [s for s in range(256) if s not in used], 8)      # 255 codes of length 8, one of length 9
    assert len(table) == 256
    return _base(64, 48, 'gray', generate(rng, lay, [[0, 1, 3, 5]], [used]), {(0, 0): DC_PLAIN, (1, 0): table})


def _slots23_444():
    rng = _rng('slots23_444')
    lay = Layout(33, 17, '444')
    a, b, c = AC_DEEP, AC_DEEP2, [EOB, 0x01, 0x11, 0x02, 0x21, 0x31, 0x12, ZRL, 0x03]
    huff = {(0, 0): unary(range(12)), (0, 2): unary(range(12), 4), (0, 3): flat(list(range(12)), 4),
            (1, 1): unary(a), (1, 2): unary(b), (1, 3): flat(c, 4)}
    quant = {1: [1 + k % 2 for k in range(64)], 2: [2] * 64, 3: [3 - k % 3 for k in range(64)]}
    coef = generate(rng, lay, [list(range(10))] * 3, [a, b, c])
    return _base(33, 17, '444', coef, huff, quant=quant, tq=[1, 2, 3], td=[0, 2, 3], ta=[1, 2, 3], sof=0xC1)


def _picture_420(name, **kw):
    def build():
        rng = _rng('picture_420')
        lay = Layout(33, 17, '420')
        huff = {(0, 0): unary(range(12)), (1, 0): unary(AC_DEEP), (0, 1): flat(list(range(12)), 5), (1, 1): unary(AC_DEEP2)}
        coef = generate(rng, lay, [list(range(9))] * 3, [AC_DEEP, AC_DEEP2, AC_DEEP2])
        return _base(33, 17, '420', coef, huff, **kw)
    return build


#: first definitions that decode the real stream to something else: the real tables' symbols at other lengths
_DECOY = {(0, 0): unary(list(range(11, -1, -1))), (1, 1): unary(AC_DEEP2[::-1]), (1, 0): flat(AC_DEEP, 5)}


def _dc_cat11():
    rng = _rng('dc_cat11')
    lay = Layout(24, 16, '444')
    coef = generate(rng, lay, [[11]] * 3, [[0x01, EOB]] * 3)
    return _base(24, 16, '444', coef, {(0, 0): {11: 1, 0: 2}, (1, 0): AC_SMALL, (0, 1): at_length(11, 12, DC_OTHERS),
                                       (1, 1): AC_SMALL})


def _dc_wrap(restart):
    def build():
        lay = Layout(64, 48, '444')
        diffs = np.zeros(lay.nblocks, np.int32)
        up = np.array([2047] * 24 + [-2047] * 24)
        diffs[np.array(lay.order)[np.array(lay.comp) == 0]] = up
        diffs[np.array(lay.order)[np.array(lay.comp) == 1]] = -up
        huff = {(0, 0): {11: 1, 0: 2}, (1, 0): {EOB: 1, 0x01: 2}, (0, 1): unary(range(12)), (1, 1): {EOB: 1, 0x01: 2}}
        return _base(64, 48, '444', np.zeros(lay.nblocks * 64, np.int16), huff, dc_diffs=diffs, restart=restart)
    return build


def _ac_wide():
    rng = _rng('ac_wide')
    lay = Layout(16, 16, 'gray')
    wide = [r << 4 | s for s in range(11, 16) for r in (0, 1, 3)]
    table = {EOB: 1, 0x01: 2}
    table.update({s: 16 for s in wide})
    return _base(16, 16, 'gray', generate(rng, lay, [[0, 5]], [wide + [0x01] + wide + [EOB]]),
                 {(0, 0): DC_PLAIN, (1, 0): table})


def _full_block():
    rng = _rng('full_block')
    coef = rng.integers(1, 8, (6, 64)) * rng.choice([-1, 1], (6, 64))
    return _base(24, 16, 'gray', coef, {(0, 0): DC_PLAIN, (1, 0): {0x01: 1, 0x02: 2, 0x03: 3, EOB: 4}})


def _only_k63():
    coef = np.zeros((6, 64), np.int16)
    coef[:, 63] = (1, -1, 3, -2, 1, 1)              # three ZRL, then a run of 14 in front of the last term
    coef[:, 0] = (4, 4, -3, 0, 9, 9)
    return _base(24, 16, 'gray', coef, {(0, 0): DC_PLAIN, (1, 0): {ZRL: 1, 0xE1: 2, 0xE2: 3, EOB: 4}})


def _zrl_eob():
    rng = _rng('zrl_eob')
    lay = Layout(24, 16, '422')
    coef = generate(rng, lay, [[0, 2, 3]] * 3, [[0x01, 0x11, 0x02, EOB, 0x21, 0x01, 0x31]] * 3)
    huff = {(0, 0): DC_PLAIN, (1, 0): {EOB: 2, 0x01: 2, 0x02: 3, 0x11: 3, ZRL: 4, 0x21: 5, 0x31: 6},
            (0, 1): DC_PLAIN, (1, 1): {ZRL: 1, EOB: 2, 0x01: 3, 0x11: 4, 0x02: 5, 0x21: 6, 0x31: 7}}
    return _base(24, 16, '422', coef, huff, zrl_eob=2)


def _runs():
    rng = _rng('runs')
    lay = Layout(48, 32, 'gray')
    syms = [r << 4 | s for r in range(16) for s in (1, 10)]
    table = flat(syms + [EOB, ZRL], 6)
    coef = np.zeros((lay.nblocks, 64), np.int16)
    b, k = 0, 1
    for sym in list(rng.permutation(syms)) * 3:      # every pair three times, placed one behind the other
        if k + (sym >> 4) > 63:
            b, k = b + 1, 1
        k += sym >> 4
        coef[b, ZIGZAG[k]] = _value(rng, int(sym) & 15)
        k += 1
    coef[:, 0] = rng.integers(-4, 5, lay.nblocks)
    return _base(48, 32, 'gray', coef, {(0, 0): DC_PLAIN, (1, 0): table})


_AC_ONES = unary([EOB, 0x01, 0x08, 0x0A, 0x09, 0x07])       # 0x08 is 110: with 255 behind it, 110 11111111
_DC_ONES = unary([0, 1, 8, 9])


def _ones_dense(restart):
    def build():
        rng = _rng('ones_dense')
        lay = Layout(24, 16, '444')
        ac = [0x08] * 30 + [0x0A, 0x09, 0x08, 0x07]
        coef = generate(rng, lay, [[8, 8, 9, 8]] * 3, [ac, ac, ac + [EOB]], restart=restart, largest=True)
        huff = {(0, 0): _DC_ONES, (1, 0): _AC_ONES, (0, 1): _DC_ONES, (1, 1): _AC_ONES}
        return _base(24, 16, '444', coef, huff, restart=restart)
    return build


def _wide_ones():
    coef = np.zeros((2, 64), np.int16)
    coef[0, 1:] = 32767                             # 1111111111111110 and fifteen one bits, 63 times
    coef[1, [ZIGZAG[k] for k in range(1, 51)]] = 32767
    coef[:, 0] = (255, 510)
    table = unary([EOB, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F])
    return _base(16, 8, 'gray', coef, {(0, 0): _DC_ONES, (1, 0): table})


def _rst(w, h, sampling, restart, **kw):
    def build():
        rng = _rng(f'rst_{w}_{h}_{sampling}')
        lay = Layout(w, h, sampling)
        n = lay.ncomp
        coef = generate(rng, lay, [[0, 1, 2, 3, 4, 5]] * n, [AC_DEEP[:9], AC_DEEP2[:9], AC_DEEP2[:9]][:n], restart=restart)
        huff = {(0, 0): DC_PLAIN, (1, 0): flat(AC_DEEP[:9], 4), (0, 1): DC_PLAIN, (1, 1): unary(AC_DEEP2[:9])}
        return _base(w, h, sampling, coef, {k: v for k, v in huff.items() if k[1] < min(n, 2)}, restart=restart, **kw)
    return build


def _pad_zero():
    """Zero padding bits in front of every restart marker.  The DC code 0 is category 9: no symbol fits into padding."""
    rng = _rng('pad_zero')
    lay = Layout(33, 17, '420')
    dc = {9: 1, 0: 2, 1: 3, 2: 4, 3: 5}
    coef = generate(rng, lay, [[0, 1, 2, 3, 9]] * 3, [AC_DEEP[:9]] * 3, restart=1)
    return _base(33, 17, '420', coef, {(0, 0): dc, (1, 0): unary(AC_DEEP[:9]), (0, 1): dc, (1, 1): flat(AC_DEEP[:9], 4)},
                 restart=1, pad=0)


def loud_terms(lay):
    """block index -> True where the block lies wholly in the MCU padding"""
    out = np.zeros(lay.nblocks, bool)
    for i in range(lay.ncomp):
        rows, cols = lay.visible(i)
        for y in range(lay.bh[i]):
            for x in range(lay.bw[i]):
                out[lay.off[i] + y * lay.bw[i] + x] = 8 * y >= rows or 8 * x >= cols
    return out


def _padding_loud(sampling, w, h):
    def build():
        rng = _rng(f'padding_loud_{sampling}_{h}x{w}')
        lay = Layout(w, h, sampling)
        planes = []
        for i in range(lay.ncomp):      # a gentle gradient where the picture is, +-110 wherever a sample is padding
            rows, cols = lay.visible(i)
            yy, xx = np.mgrid[0:lay.bh[i] * 8, 0:lay.bw[i] * 8]
            p = (3.0 * xx + 2.0 * yy - 40.0) * (1 if i != 1 else -1) / (1 if i == 0 else 2)
            loud = 110.0 * rng.choice([-1, 1], p.shape)
            planes.append(np.where((yy < rows) & (xx < cols), p, loud))
        coef = from_samples(planes).reshape(lay.nblocks, 64)
        for b in np.flatnonzero(loud_terms(lay)):      # wholly padding: DC +-1000 and strong AC
            coef[b] = 0
            coef[b, 0] = 1000 if b % 2 else -1000
            coef[b, rng.choice(np.arange(1, 64), 4, replace=False)] = rng.choice([-200, 200], 4)
        syms = sorted({EOB, ZRL} | {r << 4 | s for r in range(16) for s in range(1, 11)})
        huff = {(0, 0): DC_PLAIN, (1, 0): flat(syms, 8), (0, 1): flat(list(range(12)), 4), (1, 1): flat(syms, 8)}
        return _base(w, h, sampling, coef.reshape(-1), huff)
    return build


def _basis(q, amp):
    def build():
        coef = np.zeros((128, 64), np.int16)
        for k in range(64):
            coef[2 * k, k], coef[2 * k + 1, k] = amp, -amp
        size = abs(amp).bit_length()
        huff = {(0, 0): {0: 1, size: 2}, (1, 0): flat([r << 4 | size for r in range(16)] + [EOB, ZRL], 5)}
        return _base(128, 64, 'gray', coef, huff, quant={0: [q] * 64}, restart=1)      # the DC terms are not differenced
    return build


def _invalid(kind):
    def build():
        rng = _rng('invalid')
        lay = Layout(16, 16, 'gray')
        coef = generate(rng, lay, [[2, 3]], [[0x01, 0x11, EOB]])
        dc = dict(DC_PLAIN)
        dc[12] = 13
        ac = {EOB: 1, 0x01: 3, 0x11: 5, 0xF1: 6}      # 0, 100, 11000, 110010: 101 is in no table
        block = {'bad_dc_category': [('dc', 12, 0xABC, 12), ('ac', EOB)],
                 'bad_index': [('dc', 2, 3, 2)] + [('ac', 0xF1, 1, 1)] * 4 + [('ac', EOB)],
                 'bad_code': [('dc', 2, 3, 2), ('ac', 0x01, 1, 1), ('raw', 0b101, 3), ('raw', 0x0A5A, 13)]}[kind]
        return _base(16, 16, 'gray', coef, {(0, 0): dc, (1, 0): ac}, override={1: block})
    return build


CASES = {}
for _L in range(1, 17):
    CASES[f'len_dc_{_L}'] = _len_dc(_L)
    CASES[f'len_ac_{_L}'] = _len_ac(_L)
CASES['look_9_10'] = _look_9_10
for _s in SAMPLINGS:
    CASES['deep_' + _s] = _deep(_s)
CASES.update({
    'flat8_444': _flat8_444, 'single_gray': _single_gray, 'sym256_ac': _sym256_ac, 'slots23_444': _slots23_444,
    'redefined_420': _picture_420('redefined_420', decoy=_DECOY, dht='split'),
    'dht_split': _picture_420('dht_split', dht='split'), 'dht_joined': _picture_420('dht_joined'),
    'redefined_joined_420': _picture_420('redefined_joined_420', decoy=_DECOY),
    'dc_cat11': _dc_cat11, 'dc_wrap': _dc_wrap(0), 'dc_wrap_rst': _dc_wrap(22), 'ac_wide': _ac_wide,
    'full_block': _full_block, 'only_k63': _only_k63, 'zrl_eob': _zrl_eob, 'runs': _runs,
    'ones_dense_plain': _ones_dense(0), 'ones_dense_rst': _ones_dense(1), 'wide_ones': _wide_ones,
    'rst_1_gray': _rst(520, 8, 'gray', 1), 'rst_1_444': _rst(64, 48, '444', 1),
    'rst_short_last_420': _rst(33, 17, '420', 4), 'rst_larger_than_scan_422': _rst(33, 17, '422', 1000),
    'rst_fill_444': _rst(33, 17, '444', 2, fill={1: 1, 4: 3}), 'pad_zero_rst_420': _pad_zero,
    'padding_loud_422_9x7': _padding_loud('422', 7, 9), 'padding_loud_422_17x33': _padding_loud('422', 33, 17),
    'padding_loud_420_9x7': _padding_loud('420', 7, 9), 'padding_loud_420_17x33': _padding_loud('420', 33, 17),
    # even sizes: the last column and row are odd ones, whose fancy-upsampling neighbour would be the first padded sample
    'padding_loud_422_10x6': _padding_loud('422', 6, 10), 'padding_loud_420_10x6': _padding_loud('420', 6, 10),
    'basis_q1': _basis(1, 2040), 'basis_q255': _basis(255, 8),
})
INVALID = {'bad_dc_category': (_invalid('bad_dc_category'), ERR_DC_CATEGORY), 'bad_index': (_invalid('bad_index'), ERR_INDEX),
           'bad_code': (_invalid('bad_code'), ERR_CODE)}


def make(name):
    """-> (file bytes, expected coefficients or None, the arguments ``write`` was given)"""
    args = (CASES[name] if name in CASES else INVALID[name][0])()
    data, expected = write(**args)
    return data, expected, args
