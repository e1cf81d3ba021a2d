// The Huffman scan decode of the baseline JPEG decoder as one body for the host and the device: the bit reader and the
// block decode of jpeg_host.cpp (BitReader, decode_symbol, receive_extend, decode_block) restated over plain pointers
// and the packed table form (yv4_jpeg_huff), plus the loop over one segment's MCUs.  csrc/jpeg_entropy.hip runs it one
// lane per segment, csrc/jpeg_entropy_host.cpp on the CPU over the same tables (yv4_jpeg_entropy_decode_segments), so
// that the tests without a GPU and tools/jpeg_entropy_sanitize.cpp exercise the code the kernel runs.  jpeg_host.cpp is
// the oracle: for every file both give the same coefficients, and they fail on the same files.
//
// A segment is a run of whole MCUs whose bytes [begin, end) start on a byte boundary in the initial state (DC
// predictors zero, first block of an MCU).  The bytes are untrusted; the counts (MCU range, block grid) were validated
// by the host.  Every read stays inside [begin, end), every loop is bounded by a validated count (MCUs, at most 10
// blocks per MCU, 64 coefficients per block, 7 code lengths), every store lands on a block of the image's own grid.
#ifndef YV4_JPEG_ENTROPY_CORE_H_
#define YV4_JPEG_ENTROPY_CORE_H_
#include <stdint.h>

#include "yv4.h"

#if defined(__HIPCC__) && defined(__HIP__)
#define YV4_JPEG_HD __host__ __device__ __forceinline__
#else
#define YV4_JPEG_HD inline
#endif

namespace yv4 {
namespace jpeg {

// MSB-first bit reader over one segment.  0xFF00 is the data byte 0xFF; at any other marker, or at the end of the
// segment's bytes, the reader stops advancing and feeds zero bits, counting them: a block whose decode reached into
// them was cut short.
struct BitReader {
  const uint8_t* d;
  int64_t pos, end;
  uint64_t acc;
  int nbits, fake;
  bool stopped;

  YV4_JPEG_HD void fill() {
    while (nbits <= 56) {
      unsigned byte = 0;
      if (!stopped) {
        if (pos < end) {
          byte = d[pos];
          if (byte != 0xFF) ++pos;
          else if (pos + 1 < end && d[pos + 1] == 0) pos += 2;
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
  YV4_JPEG_HD unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1u)); }   // 1 <= n <= 16 <= nbits
  YV4_JPEG_HD void skip(int n) { nbits -= n; }
  YV4_JPEG_HD bool overrun() const { return nbits < fake; }
  YV4_JPEG_HD int real_bits() const { return nbits - fake; }
};

// -> symbol, or -1 for a code in no table.  Codes of up to 9 bits come from the lookahead; longer ones from the
// canonical bounds of lengths 10..16 (maxcode / valoff index 0 is length 10).
YV4_JPEG_HD int decode_symbol(BitReader& b, const yv4_jpeg_huff& h) {
  b.fill();
  const unsigned e = h.look[b.peek(9)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int code16 = (int)b.peek(16);
  for (int l = 10; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= h.maxcode[l - 10]) {
      b.skip(l);
      return h.vals[(h.valoff[l - 10] + code) & 255];      // in 0 .. nvals - 1 for a table yv4_jpeg_scan_prepare packed
    }
  }
  return -1;
}

// the s-bit magnitude field -> signed value (T.81 F.2.2.1 EXTEND).  No refill: decode_symbol's left at least
// 57 - 16 bits behind the code, and s <= 15.
YV4_JPEG_HD int receive_extend(BitReader& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// natural-order index of the k-th coefficient of the scan (the kernel keeps a copy in LDS, next to the Huffman tables)
#define YV4_JPEG_ZIGZAG                                                                                      \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                     \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                     \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// One block: blk[0] and the nonzero AC coefficients are written (the block was zero-filled before).  -> 0 or a
// YV4_JPEG_ERR_* code.
YV4_JPEG_HD int decode_block(BitReader& b, const yv4_jpeg_huff& dc, const yv4_jpeg_huff& ac, const uint8_t* zigzag,
                             int& pred, int16_t* blk) {
  int s = decode_symbol(b, dc);
  if (s < 0) return YV4_JPEG_ERR_CODE;
  if (s > 11) return YV4_JPEG_ERR_DC_CATEGORY;
  if (s) pred += receive_extend(b, s);
  pred = (int16_t)pred;      // libjpeg stores the running value as a 16-bit coefficient: wrap, do not grow
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return YV4_JPEG_ERR_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;      // EOB
      k += 16;                 // ZRL
      continue;
    }
    k += r;
    if (k > 63) return YV4_JPEG_ERR_INDEX;
    blk[zigzag[k]] = (int16_t)receive_extend(b, s);
    ++k;
  }
  if (b.overrun()) return YV4_JPEG_ERR_OVERRUN;
  return 0;
}

// One segment of image `sc`: `bytes` is the image's file, `tabs` its packed tables (sc.nhuff of them), `zigzag` the 64
// entries of YV4_JPEG_ZIGZAG, `coef` the image's first coefficient.  -> 0 or a YV4_JPEG_ERR_* code; on an error the
// segment stops where it is.
YV4_JPEG_HD int decode_segment(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, const uint8_t* bytes,
                               const yv4_jpeg_huff* tabs, const uint8_t* zigzag, int16_t* coef) {
  BitReader b = {bytes, sg.begin, sg.end, 0, 0, 0, false};
  const int nc = sc.ncomp;
  const int64_t bw0 = (int64_t)sc.mcus_x * sc.hs, nb0 = bw0 * ((int64_t)sc.mcus_y * sc.vs);
  const int64_t nb1 = (int64_t)sc.mcus_x * sc.mcus_y;       // a chroma plane: one block per MCU
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int my = sg.first_mcu / sc.mcus_x, mx = sg.first_mcu - my * sc.mcus_x;
  for (int m = 0; m < sg.mcu_count; ++m) {
    for (int v = 0; v < sc.vs; ++v)
      for (int h = 0; h < sc.hs; ++h) {
        const int64_t by = (int64_t)my * sc.vs + v, bx = (int64_t)mx * sc.hs + h;
        const int st = decode_block(b, tabs[sc.td[0]], tabs[sc.ta[0]], zigzag, pred0, coef + 64 * (by * bw0 + bx));
        if (st) return st;
      }
    if (nc == 3) {
      const int64_t cb = (int64_t)my * sc.mcus_x + mx;
      int st = decode_block(b, tabs[sc.td[1]], tabs[sc.ta[1]], zigzag, pred1, coef + 64 * (nb0 + cb));
      if (st) return st;
      st = decode_block(b, tabs[sc.td[2]], tabs[sc.ta[2]], zigzag, pred2, coef + 64 * (nb0 + nb1 + cb));
      if (st) return st;
    }
    if (++mx == sc.mcus_x) { mx = 0; ++my; }
  }
  // what follows the last MCU is padding to the byte boundary: a whole byte more is data where a restart marker (or
  // the end of the scan) is due
  b.fill();
  if (b.real_bits() >= 8) return YV4_JPEG_ERR_TRAILING;
  return 0;
}

}  // namespace jpeg
}  // namespace yv4
#endif  // YV4_JPEG_ENTROPY_CORE_H_
