"""Baseline JPEG decoding restated in numpy: the definition ``csrc/jpeg_host.cpp`` and ``csrc/jpeg.hip`` are held to.

It states libjpeg's default decode -- Huffman decode (ITU T.81 annex F), the ``jidctint`` "islow" integer IDCT, fancy
chroma upsampling and the 16-bit fixed-point YCbCr conversion -- from their definitions, and is itself held byte for
byte against libjpeg-turbo's output (``tests/golden/jpeg.npz``, written by Pillow).  Slow and plain on purpose: one
bit at a time in the entropy decoder, whole planes at a time afterwards.  Integer arithmetic is int32 and wraps, as
the kernel's does.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unsupported(Exception):
    """A valid file of a kind that is not built (``YV4_E_UNSUPPORTED``)."""


class Invalid(Exception):
    """A malformed file (``YV4_E_INVALID``)."""


def _huff_table(counts, vals):
    """{(length, code): symbol} of a DHT table: canonical codes, shortest first."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                raise Invalid('Huffman table overflow')
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def parse(data):
    """The headers up to SOS -> dict with the fields of ``yv4_jpeg_info`` plus the Huffman tables."""
    d = bytes(data)
    if len(d) < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Invalid('no SOI')
    pos, info = 2, None
    quant, dc, ac, ri = {}, {}, {}, 0
    adobe = None
    while True:
        if pos + 2 > len(d):
            raise Invalid('truncated')
        if d[pos] != 0xFF:
            raise Invalid('no marker')
        pos += 1
        while pos < len(d) and d[pos] == 0xFF:
            pos += 1
        if pos >= len(d):
            raise Invalid('truncated')
        m = d[pos]
        pos += 1
        if m in (0xD8, 0xD9, 0x00, 0x01) or 0xD0 <= m <= 0xD7:
            raise Invalid('stray marker')
        if pos + 2 > len(d):
            raise Invalid('truncated')
        seglen = (d[pos] << 8) | d[pos + 1]
        if seglen < 2 or pos + seglen > len(d):
            raise Invalid('segment past the end')
        seg, pos = d[pos + 2:pos + seglen], pos + seglen
        if m in (0xC0, 0xC1):
            if info is not None or len(seg) < 6:
                raise Invalid('frame header')
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise Unsupported('precision')
            if w == 0 or h == 0 or nc == 0:
                raise Invalid('zero size')
            if nc not in (1, 3):
                raise Unsupported('components')
            if len(seg) != 6 + 3 * nc:
                raise Invalid('frame header length')
            ids = [seg[6 + 3 * i] for i in range(nc)]
            hs = [seg[7 + 3 * i] >> 4 for i in range(nc)]
            vs = [seg[7 + 3 * i] & 15 for i in range(nc)]
            tq = [seg[8 + 3 * i] for i in range(nc)]
            for i in range(nc):      # component by component, in the order a reader meets them
                if not (1 <= hs[i] <= 4 and 1 <= vs[i] <= 4):
                    raise Invalid('sampling factor')
                if tq[i] > 3:
                    raise Invalid('quant selector')
            if nc == 1:
                hs, vs = [1], [1]
            else:
                if (hs[0], vs[0]) not in ((1, 1), (2, 1), (2, 2)) or (hs[1], vs[1], hs[2], vs[2]) != (1, 1, 1, 1):
                    raise Unsupported('sampling')
                if ids == [ord('R'), ord('G'), ord('B')]:
                    raise Unsupported('RGB')
            mx, my = -(-w // (8 * hs[0])), -(-h // (8 * vs[0]))
            info = dict(width=w, height=h, ncomp=nc, hs=hs, vs=vs, tq=tq, ids=ids, mcus_x=mx, mcus_y=my,
                        blocks_w=[mx * a for a in hs], blocks_h=[my * a for a in vs])
            info['ncoef'] = 64 * sum(a * b for a, b in zip(info['blocks_w'], info['blocks_h']))
        elif m == 0xC4:
            while seg:
                if len(seg) < 17:
                    raise Invalid('short DHT')
                tc, th = seg[0] >> 4, seg[0] & 15
                if tc > 1 or th > 3:
                    raise Invalid('DHT slot')
                counts = list(seg[1:17])
                n = sum(counts)
                if n > 256 or 17 + n > len(seg):
                    raise Invalid('DHT size')
                (ac if tc else dc)[th] = _huff_table(counts, list(seg[17:17 + n]))
                seg = seg[17 + n:]
        elif m == 0xDB:
            while seg:
                pq, t = seg[0] >> 4, seg[0] & 15
                if pq == 1:
                    raise Unsupported('16-bit quant table')
                if pq > 1 or t > 3 or len(seg) < 65:
                    raise Invalid('DQT')
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = list(seg[1:65])
                quant[t] = q
                seg = seg[65:]
        elif m == 0xDD:
            if len(seg) != 2:
                raise Invalid('DRI')
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                adobe = seg[11]
        elif m == 0xDA:
            if info is None or len(seg) < 1:
                raise Invalid('scan before frame')
            ns = seg[0]
            if not 1 <= ns <= 4 or len(seg) != 4 + 2 * ns:
                raise Invalid('scan header')
            if ns != info['ncomp']:
                raise Unsupported('multi-scan')
            td, ta = [], []
            for i in range(ns):
                if seg[1 + 2 * i] != info['ids'][i]:
                    raise Unsupported('component order')
                if seg[2 + 2 * i] >> 4 > 3 or seg[2 + 2 * i] & 15 > 3:
                    raise Invalid('Huffman selector')
                td.append(seg[2 + 2 * i] >> 4)
                ta.append(seg[2 + 2 * i] & 15)
            if tuple(seg[1 + 2 * ns:]) != (0, 63, 0):
                raise Invalid('spectral selection')
            for i in range(ns):
                if info['tq'][i] not in quant or td[i] not in dc or ta[i] not in ac:
                    raise Invalid('missing table')
            if adobe is not None and ns == 3 and adobe != 1:
                raise Unsupported('Adobe transform')
            info.update(td=td, ta=ta, restart_interval=ri, scan_offset=pos,
                        quant=np.stack([quant.get(t, np.zeros(64, np.uint16)) for t in range(4)]), dc=dc, ac=ac)
            return info
        elif m == 0xC2:
            raise Unsupported('progressive')
        elif 0xC3 <= m <= 0xCF:
            raise Unsupported('lossless / hierarchical / arithmetic')


class _Bits:
    """The entropy-coded segment one bit at a time: 0xFF00 is the byte 0xFF, any other marker ends the data."""

    def __init__(self, d, pos):
        self.d, self.pos, self.cur, self.left = d, pos, 0, 0

    def bit(self):
        if self.left == 0:
            d, p = self.d, self.pos
            if p >= len(d):
                raise Invalid('truncated scan')
            if d[p] == 0xFF:
                if p + 1 < len(d) and d[p + 1] == 0:
                    self.pos = p + 2
                else:
                    raise Invalid('marker inside a block')
            else:
                self.pos = p + 1
            self.cur, self.left = d[p], 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Invalid('code in no table')

    def value(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy_decode(data, info=None):
    """-> (info, coefficients): int16, natural order, each component a plane of blocks over the MCU-padded grid."""
    d = bytes(data)
    info = info or parse(d)
    nc = info['ncomp']
    planes = [np.zeros((info['blocks_h'][i], info['blocks_w'][i], 64), np.int16) for i in range(nc)]
    bits = _Bits(d, info['scan_offset'])
    pred = [0] * nc
    ri, rst, n = info['restart_interval'], 0, 0
    for my in range(info['mcus_y']):
        for mx in range(info['mcus_x']):
            if ri and n and n % ri == 0:
                p = bits.pos
                while p + 1 < len(d) and d[p] == 0xFF and d[p + 1] == 0xFF:
                    p += 1
                if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD0 + rst:
                    raise Invalid('restart marker')
                bits.pos, bits.left, pred, rst = p + 2, 0, [0] * nc, (rst + 1) & 7
            n += 1
            for i in range(nc):
                for v in range(info['vs'][i]):
                    for h in range(info['hs'][i]):
                        blk = planes[i][my * info['vs'][i] + v, mx * info['hs'][i] + h]
                        s = bits.symbol(info['dc'][info['td'][i]])
                        if s > 11:
                            raise Invalid('DC category')
                        if s:
                            # libjpeg keeps the running DC value as a 16-bit coefficient: it wraps
                            pred[i] = ((pred[i] + bits.value(s) + 0x8000) & 0xFFFF) - 0x8000
                        blk[0] = pred[i]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(info['ac'][info['ta'][i]])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Invalid('coefficient index past 63')
                            blk[ZIGZAG[k]] = bits.value(s)
                            k += 1
    return info, np.concatenate([p.reshape(-1) for p in planes])


def _fix(x):
    return int(x * 8192 + 0.5)


def _idct8(v):
    """One 8-point pass of jidctint's islow IDCT along axis 0 of an int32 (8, ...) array, before the descale."""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * _fix(0.541196100)
    tmp2 = z1 + z3 * (-_fix(1.847759065))
    tmp3 = z1 + z2 * _fix(0.765366865)
    tmp0 = (v[0] + v[4]) << 13
    tmp1 = (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * _fix(1.175875602)
    tmp0 = tmp0 * _fix(0.298631336)
    tmp1 = tmp1 * _fix(2.053119869)
    tmp2 = tmp2 * _fix(3.072711026)
    tmp3 = tmp3 * _fix(1.501321110)
    z1 = z1 * (-_fix(0.899976223))
    z2 = z2 * (-_fix(2.562915447))
    z3 = z3 * (-_fix(1.961570560)) + z5
    z4 = z4 * (-_fix(0.390180644)) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                     tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3])


def _range_limit(v):
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def idct_plane(coef, quant, blocks_h, blocks_w):
    """(blocks_h * blocks_w * 64,) int16 coefficients x (64,) table -> (blocks_h * 8, blocks_w * 8) uint8 samples."""
    with np.errstate(over='ignore'):
        x = coef.reshape(-1, 8, 8).astype(np.int32) * quant.reshape(8, 8).astype(np.int32)
        ws = (_idct8(x.transpose(1, 2, 0)) + np.int32(1024)) >> 11                    # columns: axis 0 is the row index
        out = (_idct8(ws.transpose(1, 0, 2)) + np.int32(1 << 17)) >> 18               # rows: axis 0 is the column index
    px = _range_limit(out).transpose(2, 1, 0)                                          # (block, row, column)
    return px.reshape(blocks_h, blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(blocks_h * 8, blocks_w * 8)


def upsample_h2v1(c, width):
    """(h, cw) real samples -> (h, width): fancy (triangle) upsampling, the edge sample replicated."""
    c = c.astype(np.int32)
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int32)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :width]


def upsample_h2v2(c, height, width):
    """(ch, cw) real samples -> (height, width): 3:1 vertically (unscaled), then 3:1 horizontally, >> 4."""
    c = c.astype(np.int32)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int32)
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + down
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:height, :width]


def _fx(x):
    return int(x * 65536 + 0.5)


def ycc_to_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((_fx(1.402) * cr + 32768) >> 16)
    b = y + ((_fx(1.772) * cb + 32768) >> 16)
    g = y + ((-_fx(0.34414) * cb - _fx(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def reconstruct(info, coef, channel_order='bgr'):
    """Coefficients -> (h, w, 3) uint8."""
    h, w, planes, off = info['height'], info['width'], [], 0
    for i in range(info['ncomp']):
        bh, bw = info['blocks_h'][i], info['blocks_w'][i]
        planes.append(idct_plane(coef[off:off + 64 * bh * bw], info['quant'][info['tq'][i]], bh, bw))
        off += 64 * bh * bw
    if info['ncomp'] == 1:
        img = np.repeat(planes[0][:h, :w, None], 3, 2)
    else:
        hs, vs = info['hs'][0], info['vs'][0]
        ch, cw = -(-h // vs), -(-w // hs)
        chroma = [p[:ch, :cw] for p in planes[1:]]
        if (hs, vs) == (2, 1):
            chroma = [upsample_h2v1(c, w) for c in chroma]
        elif (hs, vs) == (2, 2):
            chroma = [upsample_h2v2(c, h, w) for c in chroma]
        img = ycc_to_bgr(planes[0][:h, :w], chroma[0], chroma[1])
    return img[:, :, ::-1].copy() if channel_order == 'rgb' else img


def decode(data, channel_order='bgr'):
    info, coef = entropy_decode(data)
    return reconstruct(info, coef, channel_order)
