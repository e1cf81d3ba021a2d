// Host half of the baseline JPEG decoder (include/yv4.h, "baseline JPEG decoding"): marker parse and Huffman decode
// of the single interleaved scan into int16 coefficients.  No HIP call: plain C++, usable without a GPU, and compiled
// on its own with sanitizers by tools/jpeg_sanitize.cpp.
//
// The bytes are untrusted.  Every read goes through a length check (Cursor, BitReader), every loop is bounded by a
// header count (at most 65535 x 65535 pixels, 10 blocks per MCU, 64 coefficients per block), and the coefficient
// buffer is written only below info->ncoef, which the caller's capacity was checked against.
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "yv4.h"
#include "jpeg_common.h"

namespace {

const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;

// One Huffman table: canonical codes by length, plus a 9-bit lookahead (code length << 8 | symbol, 0: longer code).
struct Huff {
  bool defined;
  uint8_t vals[256];
  int32_t maxcode[18];      // largest code of each length, -1: none
  int32_t valoff[17];       // vals index of a length's first code minus that code
  uint16_t look[512];
};

struct Tables {
  Huff dc[4], ac[4];
  bool quant_defined[4];
  const uint8_t* dht[2][4];      // [class][slot]: the 16 counts of the table's last definition in the file, or null
};

struct Cursor {
  const uint8_t* d;
  size_t len, pos;
  bool have(size_t n) const { return n <= len - pos; }      // pos <= len always
  unsigned u8() { return d[pos++]; }
  unsigned u16() { unsigned v = ((unsigned)d[pos] << 8) | d[pos + 1]; pos += 2; return v; }
};

int build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
  memcpy(h.vals, vals, (size_t)nvals);
  memset(h.look, 0, sizeof(h.look));
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    h.valoff[l] = k - code;
    const int n = counts[l - 1];
    if (code + n > (1 << l)) JPEG_FAIL(YV4_E_INVALID, "jpeg: a Huffman table has more codes of length %d than fit", l);
    if (l <= 9)
      for (int i = 0; i < n; ++i) {
        const int first = (code + i) << (9 - l);
        for (int j = 0; j < (1 << (9 - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | h.vals[k + i]);
      }
    h.maxcode[l] = n ? code + n - 1 : -1;
    code = (code + n) << 1;
    k += n;
  }
  h.maxcode[17] = 0x7fffffff;
  h.defined = true;
  return YV4_OK;
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// EXIF tag 0x0112 of an APP1 payload p[0 .. n): "Exif\0\0", then a TIFF header ("II" / "MM", 42, the offset of IFD0 from
// the TIFF header) and IFD0 (a count, then 12-byte entries: tag, type, count, value).  1 .. 8 when the tag is there as one
// SHORT, 0 for everything else.  Offsets count from the TIFF header and every read is checked against n.
int exif_orientation(const uint8_t* p, size_t n) {
  if (n < 14 || memcmp(p, "Exif\0\0", 6) != 0) return 0;
  const uint8_t* t = p + 6;
  const size_t tn = n - 6;      // >= 8: the TIFF header is there
  bool le;
  if (t[0] == 'I' && t[1] == 'I') le = true;
  else if (t[0] == 'M' && t[1] == 'M') le = false;
  else return 0;
  auto u16 = [&](size_t o) { return le ? (unsigned)t[o] | ((unsigned)t[o + 1] << 8) : ((unsigned)t[o] << 8) | t[o + 1]; };
  auto u32 = [&](size_t o) { return le ? u16(o) | (u16(o + 2) << 16) : (u16(o) << 16) | u16(o + 2); };
  if (u16(2) != 42) return 0;
  const size_t ifd = u32(4);
  if (ifd < 8 || ifd > tn || tn - ifd < 2) return 0;
  const size_t count = u16(ifd);
  if ((tn - ifd - 2) / 12 < count) return 0;      // an IFD that says more entries than the segment holds: inconsistent
  for (size_t i = 0; i < count; ++i) {
    const size_t e = ifd + 2 + 12 * i;
    if (u16(e) != 0x0112) continue;
    if (u16(e + 2) != 3 || u32(e + 4) != 1) return 0;      // SHORT, one value: held in the entry's first two value bytes
    const unsigned v = u16(e + 8);
    return v >= 1 && v <= 8 ? (int)v : 0;
  }
  return 0;
}

// Markers up to and including SOS.  On YV4_OK c.pos is the first byte of the entropy-coded data.
int parse_headers(Cursor& c, yv4_jpeg_info* info, Tables* t) {
  memset(info, 0, sizeof(*info));
  memset(t, 0, sizeof(*t));
  if (!c.have(2) || c.d[0] != 0xFF || c.d[1] != 0xD8) JPEG_FAIL(YV4_E_INVALID, "jpeg: no SOI marker at the start");
  c.pos = 2;
  bool have_sof = false, adobe = false, exif = false;
  int orientation = 0;
  int adobe_transform = 0;
  int comp_id[3] = {0, 0, 0};
  for (;;) {      // every turn consumes at least two bytes
    if (!c.have(2)) JPEG_FAIL(YV4_E_INVALID, "jpeg: truncated before the scan");
    if (c.u8() != 0xFF) JPEG_FAIL(YV4_E_INVALID, "jpeg: no marker where one is due (offset %zu)", c.pos - 1);
    unsigned m = c.u8();
    while (m == 0xFF) {      // fill bytes
      if (!c.have(1)) JPEG_FAIL(YV4_E_INVALID, "jpeg: truncated before the scan");
      m = c.u8();
    }
    if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7))
      JPEG_FAIL(YV4_E_INVALID, "jpeg: marker 0xFF%02X before the scan", m);
    if (!c.have(2)) JPEG_FAIL(YV4_E_INVALID, "jpeg: truncated segment");
    const unsigned seglen = c.u16();
    if (seglen < 2 || !c.have(seglen - 2)) JPEG_FAIL(YV4_E_INVALID, "jpeg: segment 0xFF%02X runs past the end of the file", m);
    const size_t next = c.pos + (seglen - 2);
    size_t left = seglen - 2;
    if (m == 0xC0 || m == 0xC1) {
      if (have_sof) JPEG_FAIL(YV4_E_INVALID, "jpeg: two frame headers");
      if (left < 6) JPEG_FAIL(YV4_E_INVALID, "jpeg: short frame header");
      const unsigned prec = c.u8(), h = c.u16(), w = c.u16(), nc = c.u8();
      if (prec != 8) JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: %u-bit samples are not built (8-bit only)", prec);
      if (w == 0 || h == 0) JPEG_FAIL(YV4_E_INVALID, "jpeg: zero width or height");
      if (nc == 0) JPEG_FAIL(YV4_E_INVALID, "jpeg: no components");
      if (nc != 1 && nc != 3)
        JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: %u components are not built (grayscale and YCbCr only, no CMYK)", nc);
      if (left != 6 + 3 * (size_t)nc) JPEG_FAIL(YV4_E_INVALID, "jpeg: frame header length");
      info->width = (int32_t)w; info->height = (int32_t)h; info->ncomp = (int32_t)nc;
      for (unsigned i = 0; i < nc; ++i) {
        comp_id[i] = (int)c.u8();
        const unsigned hv = c.u8(), tq = c.u8();
        const int hs = (int)(hv >> 4), vs = (int)(hv & 15);
        if (hs < 1 || hs > 4 || vs < 1 || vs > 4) JPEG_FAIL(YV4_E_INVALID, "jpeg: sampling factor %dx%d", hs, vs);
        if (tq > 3) JPEG_FAIL(YV4_E_INVALID, "jpeg: quantisation table selector %u", tq);
        info->hs[i] = hs; info->vs[i] = vs; info->tq[i] = (int32_t)tq;
      }
      if (nc == 1) {
        info->hs[0] = info->vs[0] = 1;      // a non-interleaved scan has one block per MCU whatever the factors say
      } else {
        const bool luma_ok = (info->hs[0] == 1 && info->vs[0] == 1) || (info->hs[0] == 2 && info->vs[0] == 1) ||
                             (info->hs[0] == 2 && info->vs[0] == 2);
        if (!luma_ok || info->hs[1] != 1 || info->vs[1] != 1 || info->hs[2] != 1 || info->vs[2] != 1)
          JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: sampling %dx%d,%dx%d,%dx%d is not built (4:4:4, 4:2:2 and 4:2:0 only)",
                    info->hs[0], info->vs[0], info->hs[1], info->vs[1], info->hs[2], info->vs[2]);
        if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
          JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: RGB components are not built (YCbCr only)");
      }
      info->mcus_x = ceil_div(info->width, 8 * info->hs[0]);
      info->mcus_y = ceil_div(info->height, 8 * info->vs[0]);
      int64_t blocks = 0;
      for (unsigned i = 0; i < nc; ++i) {
        info->blocks_w[i] = info->mcus_x * info->hs[i];
        info->blocks_h[i] = info->mcus_y * info->vs[i];
        blocks += (int64_t)info->blocks_w[i] * info->blocks_h[i];
      }
      info->ncoef = 64 * blocks;
      have_sof = true;
    } else if (m == 0xC4) {
      while (left > 0) {
        if (left < 17) JPEG_FAIL(YV4_E_INVALID, "jpeg: short Huffman table");
        const unsigned tc_th = c.u8();
        const unsigned tc = tc_th >> 4, th = tc_th & 15;
        if (tc > 1 || th > 3) JPEG_FAIL(YV4_E_INVALID, "jpeg: Huffman table class %u, slot %u", tc, th);
        const uint8_t* counts = c.d + c.pos;
        int nvals = 0;
        for (int i = 0; i < 16; ++i) nvals += counts[i];
        c.pos += 16;
        left -= 17;
        if (nvals > 256 || (size_t)nvals > left) JPEG_FAIL(YV4_E_INVALID, "jpeg: Huffman table with %d symbols", nvals);
        const int st = build_huff(tc ? t->ac[th] : t->dc[th], counts, c.d + c.pos, nvals);
        if (st != YV4_OK) return st;
        t->dht[tc][th] = counts;
        c.pos += (size_t)nvals;
        left -= (size_t)nvals;
      }
    } else if (m == 0xDB) {
      while (left > 0) {
        const unsigned pq_tq = c.u8();
        left -= 1;
        const unsigned pq = pq_tq >> 4, tq = pq_tq & 15;
        if (pq == 1) JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: 16-bit quantisation tables are not built");
        if (pq > 1 || tq > 3) JPEG_FAIL(YV4_E_INVALID, "jpeg: quantisation table precision %u, slot %u", pq, tq);
        if (left < 64) JPEG_FAIL(YV4_E_INVALID, "jpeg: short quantisation table");
        for (int k = 0; k < 64; ++k) info->quant[tq][kZigzag[k]] = (uint16_t)c.u8();
        left -= 64;
        t->quant_defined[tq] = true;
      }
    } else if (m == 0xDD) {
      if (left != 2) JPEG_FAIL(YV4_E_INVALID, "jpeg: restart interval segment length");
      info->restart_interval = (int32_t)c.u16();
    } else if (m == 0xE1) {
      if (!exif && left >= 6 && memcmp(c.d + c.pos, "Exif\0\0", 6) == 0) {      // the first Exif segment decides
        exif = true;
        orientation = exif_orientation(c.d + c.pos, left);
      }
    } else if (m == 0xEE) {
      if (left >= 12 && memcmp(c.d + c.pos, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = c.d[c.pos + 11];
      }
    } else if (m == 0xDA) {
      if (!have_sof) JPEG_FAIL(YV4_E_INVALID, "jpeg: scan before the frame header");
      if (left < 1) JPEG_FAIL(YV4_E_INVALID, "jpeg: short scan header");
      const unsigned ns = c.u8();
      if (ns < 1 || ns > 4 || left != 4 + 2 * (size_t)ns) JPEG_FAIL(YV4_E_INVALID, "jpeg: scan header length");
      if ((int)ns != info->ncomp)
        JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: a scan of %u of %d components is not built (one interleaved scan only)", ns,
                  info->ncomp);
      for (unsigned i = 0; i < ns; ++i) {
        const int id = (int)c.u8();
        const unsigned tt = c.u8();
        if (id != comp_id[i]) JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: the scan's components are not in the frame's order");
        const unsigned td = tt >> 4, ta = tt & 15;
        if (td > 3 || ta > 3) JPEG_FAIL(YV4_E_INVALID, "jpeg: Huffman table selector %u / %u", td, ta);
        info->td[i] = (int32_t)td; info->ta[i] = (int32_t)ta;
      }
      const unsigned ss = c.u8(), se = c.u8(), ahal = c.u8();
      if (ss != 0 || se != 63 || ahal != 0) JPEG_FAIL(YV4_E_INVALID, "jpeg: spectral selection in a sequential scan");
      for (int i = 0; i < info->ncomp; ++i) {
        if (!t->quant_defined[info->tq[i]]) JPEG_FAIL(YV4_E_INVALID, "jpeg: quantisation table %d is missing", info->tq[i]);
        if (!t->dc[info->td[i]].defined) JPEG_FAIL(YV4_E_INVALID, "jpeg: DC Huffman table %d is missing", info->td[i]);
        if (!t->ac[info->ta[i]].defined) JPEG_FAIL(YV4_E_INVALID, "jpeg: AC Huffman table %d is missing", info->ta[i]);
      }
      if (adobe && info->ncomp == 3 && adobe_transform != 1)
        JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: Adobe colour transform %d is not built (YCbCr only)", adobe_transform);
      info->orientation = orientation;
      info->scan_offset = (int64_t)c.pos;
      return YV4_OK;
    } else if (m == 0xC2) {
      JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: progressive files (SOF2) are not built");
    } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) {
      JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: lossless / hierarchical files (SOF%u) are not built", m - 0xC0);
    } else if (m >= 0xC8 && m <= 0xCF) {
      JPEG_FAIL(YV4_E_UNSUPPORTED, "jpeg: arithmetic coding (marker 0xFF%02X) is not built", m);
    }
    // APPn, COM and everything else with a length: skipped
    c.pos = next;
  }
}

// MSB-first bit reader over the entropy-coded segment.  0xFF00 is the data byte 0xFF; at any other marker, or at the
// end of the input, the reader stops advancing and feeds zero bits, counting them: a block whose decode reached into
// them was cut short.
struct BitReader {
  const uint8_t* d;
  size_t len, pos;
  uint64_t acc;
  int nbits, fake;
  bool stopped;

  void reset() { acc = 0; nbits = 0; fake = 0; stopped = false; }
  void fill() {
    if (nbits <= 32 && !stopped && len - pos >= 4) {      // four plain data bytes at once (pos <= len always)
      const uint32_t w = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      const uint32_t inv = ~w;
      if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {      // no byte of w is 0xFF
        acc = (acc << 32) | w;
        nbits += 32;
        pos += 4;
      }
    }
    while (nbits <= 56) {
      unsigned byte = 0;
      if (!stopped) {
        if (pos < len) {
          byte = d[pos];
          if (byte != 0xFF) ++pos;
          else if (pos + 1 < len && d[pos + 1] == 0) pos += 2;
          else stopped = true;
        } else {
          stopped = true;
        }
      }
      if (stopped) { byte = 0; if (fake < (1 << 20)) fake += 8; }
      acc = (acc << 8) | byte;
      nbits += 8;
    }
  }
  unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1u)); }      // 1 <= n <= 16 <= nbits
  void skip(int n) { nbits -= n; }
  bool overrun() const { return nbits < fake; }
  int real_bits() const { return nbits - fake; }
};

// -> symbol, or -1 for a code in no table
inline int decode_symbol(BitReader& b, const Huff& h) {
  b.fill();
  const unsigned e = h.look[b.peek(9)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int code16 = (int)b.peek(16);
  for (int l = 10; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= h.maxcode[l]) {
      b.skip(l);
      return h.vals[h.valoff[l] + code];      // 0 <= index < nvals: code >= the length's first code by construction
    }
  }
  return -1;
}

// the s-bit magnitude field -> signed value (T.81 F.2.2.1 EXTEND).  No refill: decode_symbol's left at least
// 57 - 16 bits behind the code, and s <= 15.
inline int receive_extend(BitReader& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The texts are yv4_jpeg_entropy_strerror's, so that a file fails with the same words in every entropy mode.
int decode_block(BitReader& b, const Huff& dc, const Huff& ac, int& pred, int16_t* blk) {
  int s = decode_symbol(b, dc);
  if (s < 0) JPEG_FAIL(YV4_E_INVALID, "jpeg: a code that is in no Huffman table");
  if (s > 11) JPEG_FAIL(YV4_E_INVALID, "jpeg: a DC magnitude category above 11");
  if (s) pred += receive_extend(b, s);
  pred = (int16_t)pred;      // libjpeg stores the running value as a 16-bit coefficient: wrap, do not grow
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) JPEG_FAIL(YV4_E_INVALID, "jpeg: a code that is in no Huffman table");
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;      // EOB
      k += 16;                 // ZRL
      continue;
    }
    k += r;
    if (k > 63) JPEG_FAIL(YV4_E_INVALID, "jpeg: a coefficient index past 63");
    blk[kZigzag[k]] = (int16_t)receive_extend(b, s);
    ++k;
  }
  if (b.overrun()) JPEG_FAIL(YV4_E_INVALID, "jpeg: the entropy-coded data ends inside a block");
  return YV4_OK;
}

}  // namespace

int yv4::jpeg_parse_tables(const uint8_t* data, size_t len, yv4_jpeg_info* info, const uint8_t* dht[2][4]) {
  Cursor c = {data, len, 0};
  Tables* t = new Tables;
  const int st = parse_headers(c, info, t);
  if (dht) memcpy(dht, t->dht, sizeof(t->dht));
  delete t;
  return st;
}

extern "C" int yv4_jpeg_parse(const uint8_t* data, size_t len, yv4_jpeg_info* info) {
  if (!data || !info) JPEG_FAIL(YV4_E_INVALID, "jpeg_parse: null pointer");
  return yv4::jpeg_parse_tables(data, len, info, nullptr);
}

extern "C" int yv4_jpeg_entropy_decode(const uint8_t* data, size_t len, yv4_jpeg_info* info, int16_t* coef,
                                       int64_t coef_capacity) {
  if (!data || !info || !coef) JPEG_FAIL(YV4_E_INVALID, "jpeg_entropy_decode: null pointer");
  Cursor c = {data, len, 0};
  struct Holder {      // the tables are 12 KB: off the stack of a pool thread, freed on every return path
    Tables* t;
    ~Holder() { delete t; }
  } hold = {new Tables};
  const Tables& t = *hold.t;
  const int st = parse_headers(c, info, hold.t);
  if (st != YV4_OK) return st;
  if (coef_capacity < info->ncoef) {
    ::yv4::set_error("jpeg_entropy_decode: %lld coefficients, room for %lld", (long long)info->ncoef, (long long)coef_capacity);
    return YV4_E_CAPACITY;
  }
  memset(coef, 0, (size_t)info->ncoef * sizeof(int16_t));

  const int nc = info->ncomp;
  int16_t* plane[3] = {coef, coef, coef};
  for (int i = 1; i < nc; ++i) plane[i] = plane[i - 1] + (size_t)64 * info->blocks_w[i - 1] * info->blocks_h[i - 1];
  BitReader b = {data, len, c.pos, 0, 0, 0, false};
  int pred[3] = {0, 0, 0};
  const int64_t total = (int64_t)info->mcus_x * info->mcus_y;
  const int ri = info->restart_interval;
  int64_t n = 0;
  int rst = 0, until_rst = ri;
  for (int my = 0; my < info->mcus_y; ++my) {
    for (int mx = 0; mx < info->mcus_x; ++mx, ++n) {
      if (ri && until_rst == 0) {      // RSTn is due before this MCU: byte-align, check the marker, reset the state
        if (b.real_bits() >= 8) JPEG_FAIL(YV4_E_INVALID, "jpeg: data where restart marker %d is due", rst);
        size_t p = b.pos;
        while (p + 1 < len && data[p] == 0xFF && data[p + 1] == 0xFF) ++p;
        if (!(p + 1 < len) || data[p] != 0xFF || data[p + 1] != (unsigned)(0xD0 + rst))
          JPEG_FAIL(YV4_E_INVALID, "jpeg: restart marker %d is missing (MCU %lld of %lld)", rst, (long long)n, (long long)total);
        b.pos = p + 2;
        b.reset();
        pred[0] = pred[1] = pred[2] = 0;
        rst = (rst + 1) & 7;
        until_rst = ri;
      }
      for (int i = 0; i < nc; ++i) {
        const Huff& dc = t.dc[info->td[i]];
        const Huff& ac = t.ac[info->ta[i]];
        for (int v = 0; v < info->vs[i]; ++v)
          for (int h = 0; h < info->hs[i]; ++h) {
            const size_t by = (size_t)my * info->vs[i] + v, bx = (size_t)mx * info->hs[i] + h;
            const int s = decode_block(b, dc, ac, pred[i], plane[i] + 64 * (by * info->blocks_w[i] + bx));
            if (s != YV4_OK) return s;
          }
      }
      if (ri) --until_rst;
    }
  }
  // what follows the last MCU is padding to the byte boundary and a marker (or the end of a file cut after the scan)
  b.fill();
  if (b.real_bits() >= 8 || (b.pos + 1 < len && data[b.pos] == 0xFF && data[b.pos + 1] >= 0xD0 && data[b.pos + 1] <= 0xD7))
    JPEG_FAIL(YV4_E_INVALID, "jpeg: more entropy-coded data than the header's %lld MCUs", (long long)total);
  return YV4_OK;
}

extern "C" int yv4_jpeg_layout(const yv4_jpeg_info* infos, int N, yv4_jpeg_image* table, int64_t* totals) {
  return yv4_jpeg_layout_oriented(infos, N, 0, table, totals);
}

extern "C" int yv4_jpeg_layout_oriented(const yv4_jpeg_info* infos, int N, int apply, yv4_jpeg_image* table,
                                        int64_t* totals) {
  if (!infos || !table || !totals || N <= 0) JPEG_FAIL(YV4_E_INVALID, "jpeg_layout: null pointer or no image");
  int64_t coef = 0, work = 0, out = 0, units = 0, tiles = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_info& f = infos[n];
    yv4_jpeg_image& g = table[n];
    memset(&g, 0, sizeof(g));
    if (f.width < 1 || f.width > 65535 || f.height < 1 || f.height > 65535 || (f.ncomp != 1 && f.ncomp != 3))
      JPEG_FAIL(YV4_E_INVALID, "jpeg_layout: image %d is not a parsed image", n);
    g.width = f.width; g.height = f.height; g.ncomp = f.ncomp; g.hs = f.hs[0]; g.vs = f.vs[0];
    g.coef_off = coef;
    int64_t blocks = 0;
    for (int i = 0; i < f.ncomp; ++i) {
      if (f.blocks_w[i] < 1 || f.blocks_w[i] > 8192 || f.blocks_h[i] < 1 || f.blocks_h[i] > 8192 || f.tq[i] < 0 || f.tq[i] > 3)
        JPEG_FAIL(YV4_E_INVALID, "jpeg_layout: image %d is not a parsed image", n);
      g.tq[i] = f.tq[i]; g.blocks_w[i] = f.blocks_w[i]; g.blocks_h[i] = f.blocks_h[i];
      g.plane_off[i] = work;
      const int64_t nb = (int64_t)f.blocks_w[i] * f.blocks_h[i];
      work += (nb * 64 + 255) & ~(int64_t)255;
      blocks += nb;
    }
    coef += 64 * blocks;
    if (apply) {
      if (f.orientation < 0 || f.orientation > 8) JPEG_FAIL(YV4_E_INVALID, "jpeg_layout: image %d: orientation %d", n, f.orientation);
      g.orientation = f.orientation;
    }
    g.out_off = out;
    g.out_pitch = 3 * (g.orientation >= 5 ? f.height : f.width);      // 5 .. 8: the output's rows are the picture's columns
    out += ((int64_t)3 * f.width * f.height + 255) & ~(int64_t)255;
    g.unit_base = units;
    g.tile_base = tiles;
    units += (blocks + 31) / 32;
    if (g.orientation < 2) tiles += (int64_t)((f.width + 255) / 256) * ((f.height + 3) / 4);
  }
  totals[0] = coef; totals[1] = work; totals[2] = out;
  return YV4_OK;
}
