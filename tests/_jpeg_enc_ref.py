"""libjpeg's default baseline encoder restated in numpy: the definition the device encoder (``imencode``) is held to.

Integer arithmetic from the colour conversion to the last stuffed byte: jccolor.c's 16-bit fixed-point YCbCr, jcsample.c's
h2v1 / h2v2 box filters with their alternating bias, jccoefct.c's edge rules (replicated columns and rows, dummy blocks
that repeat the previous block's quantised DC), jfdctint.c's "islow" forward DCT, jcdctmgr.c's rounding division,
``jpeg_set_quality(force_baseline=TRUE)``'s tables, the four Annex K Huffman tables, one interleaved scan.  For every case
of tests/golden/jpeg_encode.npz, ``encode`` gives the file Pillow / libjpeg-turbo wrote, byte for byte.  Plain loops,
written to be read; ``tests/_jpeg_ref.py`` is the decoder's counterpart.
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63]

# Annex K.1: luminance and chrominance quantisation tables, natural order
STD_Q = (
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
     95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
     99, 99] + [99] * 32)

# Annex K.3: (counts of codes of length 1 .. 16, symbols in code order) for DC0, AC0, DC1, AC1
_AC0 = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
        0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
        0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
        0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
        0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
        0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
        0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa]
_AC1 = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
        0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
        0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
        0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
        0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
        0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
        0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
        0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa]
HUFF = (
    ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC0),
    ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC1))
HUFF_CLASS_ID = (0x00, 0x10, 0x01, 0x11)

SAMPLINGS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'gray': (1, 1)}


def quant_table(which, quality):
    """``jpeg_set_quality(quality, force_baseline=TRUE)``: table ``which`` (0 luminance, 1 chrominance), natural order."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((q * s + 50) // 100, 1), 255) for q in STD_Q[which]]


def code_table(bits, vals):
    """symbol -> (code, length): the canonical codes of T.81 Annex C."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def ycc(rgb):
    """jccolor.c rgb_ycc_convert: (h, w, 3) R, G, B -> three int planes."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _grow(plane, rows, cols):
    """Replicates the last row / column out to (rows, cols)."""
    h, w = plane.shape
    return np.pad(plane, ((0, rows - h), (0, cols - w)), mode='edge')


def component_plane(full, fh, fv):
    """One component's samples on its REAL block grid: ``full`` is the full-resolution plane, ``fh`` x ``fv`` the
    downsampling factors (hs / h_c, vs / v_c).  The four steps of the edge rule, in order."""
    h, w = full.shape
    wb = -(-(-(-w // fh)) // 8)
    hb = -(-(-(-h // fv)) // 8)
    p = _grow(full, h, wb * 8 * fh)                         # 1. columns out to the block grid, at full resolution
    p = _grow(p, -(-h // fv) * fv, p.shape[1])              # 2. rows to a multiple of the vertical factor, not further
    if fh == 2 and fv == 1:                                 # 3. jcsample.c h2v1_downsample: bias 0, 1, 0, 1 ...
        bias = np.arange(p.shape[1] // 2) & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif fh == 2 and fv == 2:                               #    h2v2_downsample: bias 1, 2, 1, 2 ...
        bias = 1 + (np.arange(p.shape[1] // 2) & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    else:
        assert fh == 1 and fv == 1
    return _grow(p, hb * 8, wb * 8), wb, hb                 # 4. the DOWNSAMPLED last row out to the block grid


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_islow(block):
    """jfdctint.c jpeg_fdct_islow over an (8, 8) int array of samples minus 128 -> (8, 8), scaled by 8."""
    C = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137,
             c1_961=16069, c2_053=16819, c2_562=20995, c3_072=25172)
    d = block.astype(np.int64).copy()
    for p in range(2):                                      # pass 0: rows; pass 1: columns
        for k in range(8):
            v = d[k, :] if p == 0 else d[:, k]
            t0, t7 = v[0] + v[7], v[0] - v[7]
            t1, t6 = v[1] + v[6], v[1] - v[6]
            t2, t5 = v[2] + v[5], v[2] - v[5]
            t3, t4 = v[3] + v[4], v[3] - v[4]
            t10, t13 = t0 + t3, t0 - t3
            t11, t12 = t1 + t2, t1 - t2
            o = [0] * 8
            if p == 0:
                o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
                n = 11
            else:
                o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
                n = 15
            z1 = (t12 + t13) * C['c0_541']
            o[2] = _descale(z1 + t13 * C['c0_765'], n)
            o[6] = _descale(z1 - t12 * C['c1_847'], n)
            z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
            z5 = (z3 + z4) * C['c1_175']
            t4, t5, t6, t7 = t4 * C['c0_298'], t5 * C['c2_053'], t6 * C['c3_072'], t7 * C['c1_501']
            z1, z2 = -z1 * C['c0_899'], -z2 * C['c2_562']
            z3, z4 = -z3 * C['c1_961'] + z5, -z4 * C['c0_390'] + z5
            o[7] = _descale(t4 + z1 + z3, n)
            o[5] = _descale(t5 + z2 + z4, n)
            o[3] = _descale(t6 + z2 + z3, n)
            o[1] = _descale(t7 + z1 + z4, n)
            if p == 0:
                d[k, :] = o
            else:
                d[:, k] = o
    return d


def quantise(coef, q):
    """jcdctmgr.c: divisor 8 q, rounded half away from zero by a truncating division of the magnitude."""
    d = 8 * np.asarray(q, np.int64).reshape(8, 8)
    mag = (np.abs(coef) + (d >> 1)) // d
    return np.where(coef < 0, -mag, mag)


def coefficients(img, quality=95, subsampling='420', channel_order='rgb'):
    """Pixels -> ``(planes, hs, vs)``: per component the quantised coefficients as an int16 (blocks_h, blocks_w, 64)
    array in natural order over the MCU-padded grid, dummy blocks filled -- the decoder's coefficient layout."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if subsampling == 'gray':
        assert img.ndim == 2
        fulls, hs, vs = [img.astype(np.int64)], 1, 1
    else:
        assert img.ndim == 3 and img.shape[2] == 3
        fulls = ycc(img if channel_order == 'rgb' else img[..., ::-1])
        hs, vs = SAMPLINGS[subsampling]
    h, w = img.shape[:2]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    planes = []
    for c, full in enumerate(fulls):
        ch, cv = (hs, vs) if c == 0 else (1, 1)                # this component's sampling factors
        p, wb, hb = component_plane(full, hs // ch, vs // cv)
        q = quant_table(0 if c == 0 else 1, quality)
        out = np.zeros((my * cv, mx * ch, 64), np.int16)
        for by in range(hb):
            for bx in range(wb):
                blk = p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128
                out[by, bx] = quantise(fdct_islow(blk), q).reshape(64)
        # jccoefct.c: dummy blocks, visited in each MCU's block order so that a dummy may repeat a dummy
        for m_y in range(my):
            for m_x in range(mx):
                for yi in range(cv):
                    for xi in range(ch):
                        by, bx = m_y * cv + yi, m_x * ch + xi
                        if by < hb and bx < wb:
                            continue
                        if by < hb:                     # a real row: the block to the left
                            out[by, bx, 0] = out[by, bx - 1, 0]
                        else:                           # a dummy row: the MCU's block before this row
                            out[by, bx, 0] = out[by - 1, m_x * ch + ch - 1, 0]
        planes.append(out)
    return planes, hs, vs


def scan_order(planes, hs, vs):
    """The blocks in the order of the interleaved scan -> ``[(component, block)]``."""
    my, mx = planes[0].shape[0] // vs, planes[0].shape[1] // hs
    order = []
    for m_y in range(my):
        for m_x in range(mx):
            for c, pl in enumerate(planes):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                for yi in range(cv):
                    for xi in range(ch):
                        order.append((c, pl[m_y * cv + yi, m_x * ch + xi]))
    return order


def block_symbols(block, pred, dc, ac):
    """One block -> ``([(bits, length)], ZRL count)``: the DC difference, then the AC runs with ZRL and EOB."""
    def magnitude(v):
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v + (1 << n) - 1)

    out = []
    n, bits = magnitude(int(block[0]) - pred)
    out.append(dc[n])
    if n:
        out.append((bits, n))
    run = zrl = 0
    for k in range(1, 64):
        v = int(block[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
            zrl += 1
        n, bits = magnitude(v)
        out.append(ac[(run << 4) | n])
        out.append((bits, n))
        run = 0
    if run:
        out.append(ac[0x00])
    return out, zrl


def scan_bytes(planes, hs, vs, stats=None):
    """The entropy-coded segment: packed MSB first, padded with 1-bits, every 0xFF followed by 0x00.  ``stats``: a dict
    that receives what the fixture's coverage test asks about (pad length, ZRLs, stuffed bytes, blocks ending at 63)."""
    tabs = [code_table(*t) for t in HUFF]
    pred = [0] * len(planes)
    acc = nbits = 0
    zrl = last63 = 0
    for c, block in scan_order(planes, hs, vs):
        dc, ac = (tabs[0], tabs[1]) if c == 0 else (tabs[2], tabs[3])
        syms, nz = block_symbols(block, pred[c], dc, ac)
        pred[c] = int(block[0])
        zrl += nz
        last63 += int(block[63] != 0)
        for bits, length in syms:
            acc = (acc << length) | bits
            nbits += length
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, 'big')
    if stats is not None:
        stats.update(pad=pad, zrl=zrl, stuffed=raw.count(b'\xff'), last63=last63, blocks=sum(p.shape[0] * p.shape[1] for p in planes))
    return raw.replace(b'\xff', b'\xff\x00')


def header(width, height, quality, subsampling):
    """SOI .. SOS as libjpeg writes them with its defaults."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)

    gray = subsampling == 'gray'
    hs, vs = SAMPLINGS[subsampling]
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(1 if gray else 2):
        q = quant_table(t, quality)
        out += seg(0xDB, [t] + [q[ZIGZAG[k]] for k in range(64)])
    comps = [(1, hs, vs, 0)] if gray else [(1, hs, vs, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    sof = [8] + list(height.to_bytes(2, 'big')) + list(width.to_bytes(2, 'big')) + [len(comps)]
    for cid, h, v, tq in comps:
        sof += [cid, (h << 4) | v, tq]
    out += seg(0xC0, sof)
    for t in range(2 if gray else 4):
        bits, vals = HUFF[t]
        out += seg(0xC4, [HUFF_CLASS_ID[t]] + bits + vals)
    sos = [len(comps)]
    for cid, _, _, tq in comps:
        sos += [cid, (tq << 4) | tq]
    return out + seg(0xDA, sos + [0, 63, 0])


def encode(img, quality=95, subsampling='420', channel_order='rgb', stats=None):
    """The whole file."""
    planes, hs, vs = coefficients(img, quality, subsampling, channel_order)
    h, w = np.asarray(img).shape[:2]
    return header(w, h, quality, subsampling) + scan_bytes(planes, hs, vs, stats) + b'\xff\xd9'


def flat_coefficients(planes):
    """The planes as one int16 array in the decoder's coefficient layout (component 0 first)."""
    return np.concatenate([p.reshape(-1) for p in planes]).astype(np.int16)
