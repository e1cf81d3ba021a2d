// The baseline JPEG encoder as one body for the host and the device: libjpeg's default encode (jccolor.c, jcsample.c,
// jccoefct.c, jfdctint.c, jcdctmgr.c, jchuff.c with the Annex K tables) restated per 8x8 block over plain pointers.
// csrc/jpeg_enc.hip runs it one lane per block, csrc/jpeg_enc_host.cpp on the CPU over the same table
// (yv4_jpeg_encode_host), so that the tests without a GPU and tools/jpeg_encode_sanitize.cpp exercise the code the
// kernels run.  tests/_jpeg_enc_ref.py is the definition: for every fixture all three give libjpeg-turbo's file.
//
// The table (yv4_jpeg_enc_image) was validated by the host (jpeg_enc_validate): every index below is derived from its
// grids, every read of a pixel is clamped to the picture, every store lands in the image's own regions.
//
// Arithmetic: 32-bit int throughout, and no product or sum leaves it.  Colour: 38470 * 255 + 19595 * 255 + 7471 * 255 +
// 32768 < 2^24.  FDCT rows: samples are -128 .. 127, sums of two at most 510, the largest product 25172 * 510.  FDCT
// columns: the row pass leaves at most 2 * 8 * 255 = 4080 in magnitude (<< PASS1_BITS included), the largest product is
// 25172 * 4080 < 2^27, and an output adds at most four such terms: < 2^31.  Nothing relies on wrap-around.
#ifndef YV4_JPEG_ENC_CORE_H_
#define YV4_JPEG_ENC_CORE_H_
#include <stdint.h>

#include "yv4.h"
#include "jpeg_common.h"      // YV4_JPEG_ZIGZAG

#if defined(__HIPCC__) && defined(__HIP__)
#define YV4_ENC_HD __host__ __device__ __forceinline__
#else
#define YV4_ENC_HD inline
#endif

namespace yv4 {
namespace jpegenc {

// ---- the Annex K Huffman tables as the encoder reads them: symbol -> (code, length) -------------------------------
struct Tables {
  uint16_t dc_code[2][16];
  uint8_t dc_len[2][16];
  uint16_t ac_code[2][256];
  uint8_t ac_len[2][256];      // 0: the symbol has no code (never emitted: values are at most 10 bits, runs at most 15)
  uint8_t zigzag[64];
};

// counts of the codes of length 1 .. 16, then the symbols in code order (T.81 K.3.3).  which: 0 DC luminance,
// 1 AC luminance, 2 DC chrominance, 3 AC chrominance -- the order the header writes them in.
YV4_ENC_HD int huff_spec(int which, uint8_t* bits16, uint8_t* vals) {
  const uint8_t kBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
  const uint8_t kAc[2][162] = {
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
       0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
       0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
       0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
       0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
       0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
       0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
       0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
       0xf9, 0xfa},
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
       0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
       0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
       0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
       0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
       0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
       0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
       0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
       0xf9, 0xfa}};
  int n = 0;
  for (int l = 0; l < 16; ++l) {
    bits16[l] = kBits[which][l];
    n += kBits[which][l];
  }
  for (int k = 0; k < n; ++k) vals[k] = (which & 1) ? kAc[which >> 1][k] : (uint8_t)k;
  return n;
}

// One of the four code tables (T.81 Annex C: canonical codes); which as in huff_spec.  A lane of its own per table on
// the device.  The AC lengths of symbols without a code are zeroed first.
YV4_ENC_HD void build_table(Tables* t, int which) {
  uint8_t bits[16], vals[162];
  huff_spec(which, bits, vals);
  const int cls = which & 1, id = which >> 1;
  if (cls) {
    for (int s = 0; s < 256; ++s) { t->ac_len[id][s] = 0; t->ac_code[id][s] = 0; }
  } else {
    for (int s = 0; s < 16; ++s) { t->dc_len[id][s] = 0; t->dc_code[id][s] = 0; }
  }
  unsigned code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
      if (cls) { t->ac_code[id][vals[k]] = (uint16_t)code; t->ac_len[id][vals[k]] = (uint8_t)l; }
      else { t->dc_code[id][vals[k] & 15] = (uint16_t)code; t->dc_len[id][vals[k] & 15] = (uint8_t)l; }
    }
    code <<= 1;
  }
  if (which == 0) {
    const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;
    for (int i = 0; i < 64; ++i) t->zigzag[i] = kZigzag[i];
  }
}

// ---- the work region of one image: [total bits (padded) | 0xFF count | block-scan workgroup sums | stuffing workgroup
// sums | bits per block | the packed words], every section 8-byte aligned.  Offsets in bytes from im.work_off.
YV4_ENC_HD int64_t enc_wgs(int64_t nblocks) { return (nblocks + YV4_JPEG_ENC_WG_BLOCKS - 1) / YV4_JPEG_ENC_WG_BLOCKS; }
YV4_ENC_HD int64_t enc_bound_bytes(int64_t nblocks) { return (nblocks * YV4_JPEG_ENC_BLOCK_BITS + 7) / 8; }
YV4_ENC_HD int64_t enc_words(int64_t nblocks) { return (enc_bound_bytes(nblocks) + 3) / 4; }
YV4_ENC_HD int64_t enc_swgs(int64_t nblocks) { return (enc_words(nblocks) + YV4_JPEG_ENC_WG_BLOCKS - 1) / YV4_JPEG_ENC_WG_BLOCKS; }

struct Work {
  uint64_t* totals;      // [0] bits of the scan with its padding, [1] 0xFF bytes among them
  uint64_t* wgsum;       // enc_wgs entries
  uint64_t* sff;         // enc_swgs entries
  uint32_t* bits;        // nblocks entries, in scan order
  uint32_t* words;       // enc_words entries: the unstuffed stream, MSB first
};
YV4_ENC_HD int64_t work_bytes(int64_t nblocks) {
  return 16 + 8 * enc_wgs(nblocks) + 8 * enc_swgs(nblocks) + 4 * ((nblocks + 1) & ~(int64_t)1) + 4 * ((enc_words(nblocks) + 1) & ~(int64_t)1);
}
YV4_ENC_HD Work work_of(uint8_t* work, const yv4_jpeg_enc_image& im) {
  Work w;
  uint8_t* p = work + im.work_off;
  w.totals = reinterpret_cast<uint64_t*>(p);
  w.wgsum = w.totals + 2;
  w.sff = w.wgsum + enc_wgs(im.nblocks);
  w.bits = reinterpret_cast<uint32_t*>(w.sff + enc_swgs(im.nblocks));
  w.words = w.bits + ((im.nblocks + 1) & ~(int64_t)1);
  return w;
}

// ---- stage 1: pixels -> quantised coefficients ------------------------------------------------------------------------
struct BlockPos { int c, bx, by; int64_t index; };      // component, position on the MCU-padded grid, block of the image

// block i of the coefficient layout (planes back to back)
YV4_ENC_HD BlockPos plane_block(const yv4_jpeg_enc_image& im, int64_t i) {
  BlockPos b;
  b.index = i;
  b.c = 0;
  for (int c = 0; c + 1 < im.ncomp; ++c) {
    const int64_t n = (int64_t)im.blocks_w[b.c] * im.blocks_h[b.c];
    if (i < n) break;
    i -= n;
    ++b.c;
  }
  b.by = (int)(i / im.blocks_w[b.c]);
  b.bx = (int)(i % im.blocks_w[b.c]);
  return b;
}

// block j of the interleaved scan
YV4_ENC_HD BlockPos scan_block(const yv4_jpeg_enc_image& im, int64_t j) {
  const int luma = im.hs * im.vs, per = luma + im.ncomp - 1;
  const int64_t m = j / per;
  const int r = (int)(j % per);
  const int mx = (int)(m % im.mcus_x), my = (int)(m / im.mcus_x);
  BlockPos b;
  if (r < luma) {
    b.c = 0;
    b.bx = mx * im.hs + r % im.hs;
    b.by = my * im.vs + r / im.hs;
    b.index = (int64_t)b.by * im.blocks_w[0] + b.bx;
  } else {
    b.c = r - luma + 1;
    b.bx = mx;
    b.by = my;
    b.index = (int64_t)im.blocks_w[0] * im.blocks_h[0] + (int64_t)(b.c - 1) * im.blocks_w[1] * im.blocks_h[1] +
              (int64_t)my * im.blocks_w[b.c] + mx;
  }
  return b;
}

// the scan index of the block whose DC predicts block j's (the previous block of the same component), -1: none
YV4_ENC_HD int64_t pred_block(const yv4_jpeg_enc_image& im, int64_t j) {
  const int luma = im.hs * im.vs, per = luma + im.ncomp - 1;
  const int r = (int)(j % per);
  if (r > 0 && r < luma) return j - 1;
  if (j < per) return -1;
  return r == 0 ? j - per + luma - 1 : j - per;
}

// jccolor.c: component c of pixel p (3 bytes, B G R or R G B)
YV4_ENC_HD int ycc(const uint8_t* p, int c, int rgb) {
  const int r = rgb ? p[0] : p[2], g = p[1], b = rgb ? p[2] : p[0];
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the full-resolution sample of component c at (x, y), clamped to the picture: the replicated last column and row
YV4_ENC_HD int full_sample(const yv4_jpeg_enc_image& im, const uint8_t* pix, int c, int x, int y, int rgb) {
  x = x < im.width ? x : im.width - 1;
  y = y < im.height ? y : im.height - 1;
  const uint8_t* row = pix + im.src_off + (int64_t)y * im.src_pitch;
  return im.channels == 1 ? row[x] : ycc(row + 3 * x, c, rgb);
}

// the sample of component c at (x, y) of its own grid: jcsample.c's box filters; the DOWNSAMPLED last row repeats below it
YV4_ENC_HD int comp_sample(const yv4_jpeg_enc_image& im, const uint8_t* pix, int c, int x, int y, int rgb) {
  const int fh = c == 0 ? 1 : im.hs, fv = c == 0 ? 1 : im.vs;
  if (fh == 1) return full_sample(im, pix, c, x, y, rgb);
  if (fv == 1) return (full_sample(im, pix, c, 2 * x, y, rgb) + full_sample(im, pix, c, 2 * x + 1, y, rgb) + (x & 1)) >> 1;
  const int rows = (im.height + 1) >> 1;
  y = y < rows ? y : rows - 1;
  return (full_sample(im, pix, c, 2 * x, 2 * y, rgb) + full_sample(im, pix, c, 2 * x + 1, 2 * y, rgb) +
          full_sample(im, pix, c, 2 * x, 2 * y + 1, rgb) + full_sample(im, pix, c, 2 * x + 1, 2 * y + 1, rgb) + 1 + (x & 1)) >> 2;
}

YV4_ENC_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one pass over 8 values at stride s: pass 0 rows, pass 1 columns
YV4_ENC_HD void fdct_1d(int* v, int s, int pass) {
  const int t0 = v[0] + v[7 * s], t7 = v[0] - v[7 * s], t1 = v[s] + v[6 * s], t6 = v[s] - v[6 * s];
  const int t2 = v[2 * s] + v[5 * s], t5 = v[2 * s] - v[5 * s], t3 = v[3 * s] + v[4 * s], t4 = v[3 * s] - v[4 * s];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = pass ? 15 : 11;
  if (pass) {
    v[0] = descale(t10 + t11, 2);
    v[4 * s] = descale(t10 - t11, 2);
  } else {
    v[0] = (t10 + t11) * 4;
    v[4 * s] = (t10 - t11) * 4;
  }
  int z1 = (t12 + t13) * 4433;
  v[2 * s] = descale(z1 + t13 * 6270, n);
  v[6 * s] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 = -z1 * 7373;
  z2 = -z2 * 20995;
  z3 = -z3 * 16069 + z5;
  z4 = -z4 * 3196 + z5;
  v[7 * s] = descale(a4 + z1 + z3, n);
  v[5 * s] = descale(a5 + z2 + z4, n);
  v[3 * s] = descale(a6 + z2 + z3, n);
  v[s] = descale(a7 + z1 + z4, n);
}

// jcdctmgr.c: divisor 8 q, the magnitude rounded by a truncating division
YV4_ENC_HD int quantise(int v, int q) {
  const int d = 8 * q;
  return v < 0 ? -((-v + (d >> 1)) / d) : (v + (d >> 1)) / d;
}

// Block i of the coefficient layout -> its 64 quantised coefficients in natural order.  A dummy block (jccoefct.c: at
// or beyond the component's real grid) is not transformed: all AC zero, the DC that of the block it repeats -- the real
// block to its left, or for a dummy row the last block of the MCU's row above, itself possibly a dummy column.
YV4_ENC_HD void block_coef(const yv4_jpeg_enc_image& im, const uint8_t* pix, int64_t i, int rgb, int16_t* out64) {
  const BlockPos b = plane_block(im, i);
  const int wb = im.real_w[b.c], hb = im.real_h[b.c];
  const int ch = b.c == 0 ? im.hs : 1;
  const bool dummy = b.bx >= wb || b.by >= hb;
  int sx = b.bx < wb ? b.bx : wb - 1, sy = b.by;
  if (b.by >= hb) {
    sy = hb - 1;
    sx = b.bx / ch * ch + ch - 1;
    sx = sx < wb ? sx : wb - 1;
  }
  int d[64];
  for (int y = 0; y < 8; ++y)
    for (int x = 0; x < 8; ++x) d[y * 8 + x] = comp_sample(im, pix, b.c, sx * 8 + x, sy * 8 + y, rgb) - 128;
  for (int y = 0; y < 8; ++y) fdct_1d(d + 8 * y, 1, 0);
  for (int x = 0; x < 8; ++x) fdct_1d(d + x, 8, 1);
  const uint16_t* q = im.quant[b.c == 0 ? 0 : 1];
  if (dummy) {
    out64[0] = (int16_t)quantise(d[0], q[0]);
    for (int k = 1; k < 64; ++k) out64[k] = 0;
  } else {
    for (int k = 0; k < 64; ++k) out64[k] = (int16_t)quantise(d[k], q[k]);
  }
}

// ---- stage 2: coefficients -> the bit stream ---------------------------------------------------------------------------
YV4_ENC_HD int nbits_of(int v) {      // bits of the magnitude (jchuff.c: the category)
  unsigned a = (unsigned)(v < 0 ? -v : v);
  int n = 0;
  while (a) { ++n; a >>= 1; }
  return n;
}

// The code words of one block, in order, to emit(code, length): the DC difference, the AC runs with ZRL (0xF0) and EOB
// (0x00; none after a block whose coefficient 63 is nonzero).  A value's bits follow its code in the same word: at most
// 16 + 10 = 26 bits.  Values are clamped to what the tables code (11 / 10 bits): the encoder's own coefficients never
// reach that, foreign ones cannot index outside the tables.
template <class Emit>
YV4_ENC_HD void block_codes(const int16_t* blk, int pred, int tab, const Tables& t, Emit& emit) {
  int v = (int)blk[0] - pred;
  v = v > 2047 ? 2047 : (v < -2047 ? -2047 : v);
  int n = nbits_of(v);
  unsigned bits = (unsigned)(v < 0 ? v + (1 << n) - 1 : v);
  emit(((unsigned)t.dc_code[tab][n] << n) | bits, t.dc_len[tab][n] + n);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    v = blk[t.zigzag[k]];
    if (v == 0) { ++run; continue; }
    while (run > 15) { emit(t.ac_code[tab][0xF0], t.ac_len[tab][0xF0]); run -= 16; }
    v = v > 1023 ? 1023 : (v < -1023 ? -1023 : v);
    n = nbits_of(v);
    bits = (unsigned)(v < 0 ? v + (1 << n) - 1 : v);
    const int sym = (run << 4) | n;
    emit(((unsigned)t.ac_code[tab][sym] << n) | bits, t.ac_len[tab][sym] + n);
    run = 0;
  }
  if (run) emit(t.ac_code[tab][0], t.ac_len[tab][0]);
}

struct CountBits {
  uint32_t total = 0;
  YV4_ENC_HD void operator()(unsigned, int len) { total += (uint32_t)len; }
};

// MSB-first writer from bit position `pos` of the word stream.  Whole and partial words alike are ORed into the
// zero-filled buffer (Or: an atomic on the device), since the first and the last word of a block are shared with its
// neighbours: the result does not depend on who arrives first.
template <class Or>
struct BitWriter {
  Or orw;
  int64_t word;
  uint64_t acc;
  int n;
  YV4_ENC_HD BitWriter(Or o, uint64_t pos) : orw(o), word((int64_t)(pos >> 5)), acc(0), n((int)(pos & 31)) {}
  YV4_ENC_HD void operator()(unsigned code, int len) {      // 1 <= len <= 26, n <= 31: at most 57 bits held
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      orw(word++, (uint32_t)(acc >> n));
      acc &= ((uint64_t)1 << n) - 1;
    }
  }
  YV4_ENC_HD void flush() {
    if (n > 0) orw(word, (uint32_t)(acc << (32 - n)));
    n = 0;
    acc = 0;
  }
};

// the DC predictor of scan block j and its table selector
YV4_ENC_HD int block_pred(const yv4_jpeg_enc_image& im, const int16_t* coef, int64_t j) {
  const int64_t p = pred_block(im, j);
  return p < 0 ? 0 : (int)coef[im.coef_off + scan_block(im, p).index * 64];
}

YV4_ENC_HD uint32_t block_bits(const yv4_jpeg_enc_image& im, const int16_t* coef, int64_t j, const Tables& t) {
  const BlockPos b = scan_block(im, j);
  CountBits c;
  block_codes(coef + im.coef_off + b.index * 64, block_pred(im, coef, j), b.c == 0 ? 0 : 1, t, c);
  return c.total;
}

// Writes scan block j at bit `pos`; the image's last block adds the 1-bits that fill the last byte.
template <class Or>
YV4_ENC_HD void block_pack(const yv4_jpeg_enc_image& im, const int16_t* coef, int64_t j, uint64_t pos, uint32_t nbits,
                           const Tables& t, Or orw) {
  const BlockPos b = scan_block(im, j);
  BitWriter<Or> w(orw, pos);
  block_codes(coef + im.coef_off + b.index * 64, block_pred(im, coef, j), b.c == 0 ? 0 : 1, t, w);
  if (j == im.nblocks - 1) {
    const int pad = (int)((8 - ((pos + nbits) & 7)) & 7);
    if (pad) w((1u << pad) - 1u, pad);
  }
  w.flush();
}

// ---- stage 3: byte stuffing ------------------------------------------------------------------------------------------
YV4_ENC_HD unsigned stream_byte(const uint32_t* words, int64_t b) { return (words[b >> 2] >> (24 - 8 * (int)(b & 3))) & 255u; }

// the 0xFF bytes among the up to four stream bytes of word k (bytes at or past nbytes do not exist)
YV4_ENC_HD uint32_t word_ffs(const uint32_t* words, int64_t k, int64_t nbytes) {
  uint32_t n = 0;
  for (int64_t b = 4 * k; b < 4 * k + 4 && b < nbytes; ++b) n += stream_byte(words, b) == 255u;
  return n;
}

// writes word k's bytes behind the `before` zero bytes stuffed in front of them
YV4_ENC_HD void word_stuff(const uint32_t* words, int64_t k, int64_t nbytes, uint64_t before, uint8_t* dst) {
  int64_t o = 4 * k + (int64_t)before;
  for (int64_t b = 4 * k; b < 4 * k + 4 && b < nbytes; ++b) {
    const unsigned v = stream_byte(words, b);
    dst[o++] = (uint8_t)v;
    if (v == 255u) dst[o++] = 0;
  }
}

}  // namespace jpegenc

// jpeg_enc_host.cpp: the table against the buffers' sizes, before anything runs
int jpeg_enc_validate(const yv4_jpeg_enc_image* table, int N, int64_t pixel_bytes, int64_t coef_elems, int64_t work_bytes,
                      int64_t out_bytes, const char* who);

}  // namespace yv4
#endif  // YV4_JPEG_ENC_CORE_H_
