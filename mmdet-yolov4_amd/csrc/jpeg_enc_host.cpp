// The JPEG encoder's host half: the per-image table (yv4_jpeg_encode_layout), its validation, the header writer and the
// whole method on the CPU over the core the kernels run (yv4_jpeg_encode_host).  Plain C++ without a HIP call:
// tools/jpeg_encode_sanitize.cpp compiles it on its own.
#include <string.h>

#include "jpeg_enc_core.h"

using namespace yv4;
using namespace yv4::jpegenc;

namespace {

// Annex K.1, natural order
const uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
     95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99}};
const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;

int64_t align_up(int64_t n, int64_t a) { return (n + a - 1) / a * a; }

// what the caller says about an image, checked; then everything that follows from it (grids, tables, counts)
int fill_derived(yv4_jpeg_enc_image* im, int n, const char* who) {
  REQUIRE(im->width >= 1 && im->height >= 1, "%s: image %d is empty (%d x %d)", who, n, im->width, im->height);
  REQUIRE(im->width <= 65535 && im->height <= 65535, "%s: image %d: a side above 65535 (%d x %d)", who, n, im->width,
          im->height);
  REQUIRE(im->quality >= 1 && im->quality <= 100, "%s: image %d: quality %d is not in 1 .. 100", who, n, im->quality);
  REQUIRE(im->channels == 1 || im->channels == 3, "%s: image %d: %d channels (1 or 3)", who, n, im->channels);
  if (im->channels == 1) {
    REQUIRE(im->hs == 1 && im->vs == 1, "%s: image %d: a gray image is one 1x1 component, not %dx%d", who, n, im->hs, im->vs);
  } else {
    REQUIRE((im->hs == 1 && im->vs == 1) || (im->hs == 2 && im->vs == 1) || (im->hs == 2 && im->vs == 2),
            "%s: image %d: luma sampling %dx%d is not 1x1, 2x1 or 2x2", who, n, im->hs, im->vs);
  }
  im->ncomp = im->channels;
  im->mcus_x = (im->width + 8 * im->hs - 1) / (8 * im->hs);
  im->mcus_y = (im->height + 8 * im->vs - 1) / (8 * im->vs);
  im->nblocks = 0;
  for (int c = 0; c < 3; ++c) {
    const int ch = c == 0 ? im->hs : 1, cv = c == 0 ? im->vs : 1;
    const bool on = c < im->ncomp;
    im->blocks_w[c] = on ? im->mcus_x * ch : 0;
    im->blocks_h[c] = on ? im->mcus_y * cv : 0;
    // ceil(ceil(w * h_c / hs) / 8) real block columns, rows likewise
    im->real_w[c] = on ? ((im->width * ch + im->hs - 1) / im->hs + 7) / 8 : 0;
    im->real_h[c] = on ? ((im->height * cv + im->vs - 1) / im->vs + 7) / 8 : 0;
    im->nblocks += (int64_t)im->blocks_w[c] * im->blocks_h[c];
  }
  // jpeg_set_quality(force_baseline = TRUE)
  const int s = im->quality < 50 ? 5000 / im->quality : 200 - 2 * im->quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int v = (kStdQuant[t][k] * s + 50) / 100;
      im->quant[t][k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return YV4_OK;
}

bool inside(int64_t off, int64_t len, int64_t cap) { return off >= 0 && len >= 0 && off <= cap && len <= cap - off; }

uint8_t* put_segment(uint8_t* p, int marker, const uint8_t* body, int n) {
  *p++ = 0xFF;
  *p++ = (uint8_t)marker;
  *p++ = (uint8_t)((n + 2) >> 8);
  *p++ = (uint8_t)((n + 2) & 255);
  memcpy(p, body, (size_t)n);
  return p + n;
}

}  // namespace

namespace yv4 {

int jpeg_enc_validate(const yv4_jpeg_enc_image* table, int N, int64_t pixel_bytes, int64_t coef_elems, int64_t work_bytes,
                      int64_t out_bytes, const char* who) {
  REQUIRE(table && N >= 1, "%s: no images", who);
  int64_t wg = 0, swg = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_enc_image& im = table[n];
    yv4_jpeg_enc_image want = im;
    const int st = fill_derived(&want, n, who);
    if (st != YV4_OK) return st;
    REQUIRE(memcmp(&want, &im, sizeof(im)) == 0, "%s: image %d: the grids or tables of the entry are not what its size, "
            "sampling and quality give", who, n);
    REQUIRE(im.wg_base == wg && im.swg_base == swg, "%s: image %d: workgroup bases %lld / %lld, expected %lld / %lld", who, n,
            (long long)im.wg_base, (long long)im.swg_base, (long long)wg, (long long)swg);
    wg += enc_wgs(im.nblocks);
    swg += enc_swgs(im.nblocks);
    // 256 lanes a workgroup: each grid's lanes stay below 2^32, the tightest launch limit among HIP runtimes
    REQUIRE(wg < ((int64_t)1 << 24) && swg < ((int64_t)1 << 24), "%s: the batch is too large for one launch (2^24 "
            "workgroups a grid; %lld and %lld up to image %d)", who, (long long)wg, (long long)swg, n);
    const int64_t row = (int64_t)im.channels * im.width;
    REQUIRE(im.src_pitch >= row, "%s: image %d: pitch %d is below its row of %lld bytes", who, n, im.src_pitch, (long long)row);
    REQUIRE(inside(im.src_off, (int64_t)(im.height - 1) * im.src_pitch + row, pixel_bytes),
            "%s: image %d: its pixels (offset %lld) lie outside the buffer of %lld bytes", who, n, (long long)im.src_off,
            (long long)pixel_bytes);
    REQUIRE(im.coef_off % 64 == 0 && inside(im.coef_off, im.nblocks * 64, coef_elems),
            "%s: image %d: its coefficients (offset %lld) lie outside the buffer of %lld elements or off a block", who, n,
            (long long)im.coef_off, (long long)coef_elems);
    REQUIRE(im.work_off % 8 == 0 && inside(im.work_off, jpegenc::work_bytes(im.nblocks), work_bytes),
            "%s: image %d: its work region (offset %lld) lies outside the workspace of %lld bytes or is not 8-byte aligned",
            who, n, (long long)im.work_off, (long long)work_bytes);
    REQUIRE(im.out_cap >= 2 * enc_bound_bytes(im.nblocks), "%s: image %d: output capacity %lld is below the bound of %lld "
            "bytes", who, n, (long long)im.out_cap, (long long)(2 * enc_bound_bytes(im.nblocks)));
    REQUIRE(inside(im.out_off, im.out_cap, out_bytes), "%s: image %d: its output (offset %lld, %lld bytes) lies outside the "
            "buffer of %lld bytes", who, n, (long long)im.out_off, (long long)im.out_cap, (long long)out_bytes);
  }
  return YV4_OK;
}

}  // namespace yv4

extern "C" int yv4_jpeg_encode_layout(yv4_jpeg_enc_image* table, int N, int64_t* totals) {
  REQUIRE(table && totals && N >= 1, "jpeg_encode_layout: null pointer or no images");
  int64_t pix = 0, coef = 0, work = 0, out = 0, wg = 0, swg = 0;
  for (int n = 0; n < N; ++n) {
    yv4_jpeg_enc_image* im = table + n;
    const int st = fill_derived(im, n, "jpeg_encode_layout");
    if (st != YV4_OK) return st;
    im->src_pitch = im->channels * im->width;
    im->src_off = pix;
    pix = align_up(pix + (int64_t)im->src_pitch * im->height, 256);
    im->coef_off = coef;
    coef += im->nblocks * 64;
    im->work_off = work;
    work = align_up(work + work_bytes(im->nblocks), 256);
    im->out_off = out;
    im->out_cap = 2 * enc_bound_bytes(im->nblocks);
    out = align_up(out + im->out_cap, 256);
    im->wg_base = wg;
    im->swg_base = swg;
    wg += enc_wgs(im->nblocks);
    swg += enc_swgs(im->nblocks);
  }
  totals[0] = pix; totals[1] = coef; totals[2] = work; totals[3] = out; totals[4] = wg; totals[5] = swg;
  return YV4_OK;
}

extern "C" int yv4_jpeg_encode_validate(const yv4_jpeg_enc_image* table, int N, int64_t pixel_bytes, int64_t coef_elems,
                                        int64_t work_bytes, int64_t out_bytes) {
  return jpeg_enc_validate(table, N, pixel_bytes, coef_elems, work_bytes, out_bytes, "jpeg_encode_validate");
}

extern "C" int yv4_jpeg_encode_header(const yv4_jpeg_enc_image* im, uint8_t* out, int64_t capacity, int64_t* length) {
  REQUIRE(im && out && length, "jpeg_encode_header: null pointer");
  yv4_jpeg_enc_image want = *im;
  const int st = fill_derived(&want, 0, "jpeg_encode_header");
  if (st != YV4_OK) return st;
  REQUIRE(memcmp(want.quant, im->quant, sizeof(want.quant)) == 0 && want.ncomp == im->ncomp,
          "jpeg_encode_header: the entry is not one yv4_jpeg_encode_layout filled");
  if (capacity < YV4_JPEG_ENC_HEADER_MAX) {
    set_error("jpeg_encode_header: room for %lld bytes, %d needed", (long long)capacity, YV4_JPEG_ENC_HEADER_MAX);
    return YV4_E_CAPACITY;
  }
  const int nc = im->ncomp;
  uint8_t* p = out;
  *p++ = 0xFF;
  *p++ = 0xD8;
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = put_segment(p, 0xE0, jfif, 14);
  uint8_t body[17 + 162];
  for (int t = 0; t < (nc == 1 ? 1 : 2); ++t) {
    body[0] = (uint8_t)t;
    for (int k = 0; k < 64; ++k) body[1 + k] = (uint8_t)im->quant[t][kZigzag[k]];
    p = put_segment(p, 0xDB, body, 65);
  }
  body[0] = 8;
  body[1] = (uint8_t)(im->height >> 8); body[2] = (uint8_t)(im->height & 255);
  body[3] = (uint8_t)(im->width >> 8); body[4] = (uint8_t)(im->width & 255);
  body[5] = (uint8_t)nc;
  for (int c = 0; c < nc; ++c) {
    body[6 + 3 * c] = (uint8_t)(c + 1);
    body[7 + 3 * c] = (uint8_t)(c == 0 ? (im->hs << 4) | im->vs : 0x11);
    body[8 + 3 * c] = (uint8_t)(c == 0 ? 0 : 1);
  }
  p = put_segment(p, 0xC0, body, 6 + 3 * nc);
  for (int t = 0; t < (nc == 1 ? 2 : 4); ++t) {
    body[0] = (uint8_t)(((t & 1) << 4) | (t >> 1));
    const int nv = huff_spec(t, body + 1, body + 17);
    p = put_segment(p, 0xC4, body, 17 + nv);
  }
  body[0] = (uint8_t)nc;
  for (int c = 0; c < nc; ++c) {
    body[1 + 2 * c] = (uint8_t)(c + 1);
    body[2 + 2 * c] = (uint8_t)(c == 0 ? 0x00 : 0x11);
  }
  body[1 + 2 * nc] = 0; body[2 + 2 * nc] = 63; body[3 + 2 * nc] = 0;
  p = put_segment(p, 0xDA, body, 4 + 2 * nc);
  *length = p - out;
  return YV4_OK;
}

// The whole method on the CPU, stage by stage as the kernels run it and over the same work regions: every block's
// coefficients; every block's bit count, the running sum in scan order, the pack (a plain OR where the device uses an
// atomic one); the 0xFF count and the stuffed write.  stage: 1 pixels -> coefficients, 2 coefficients -> scan bytes,
// 3 both.
extern "C" int yv4_jpeg_encode_host(const yv4_jpeg_enc_image* table, int N, int stage, const uint8_t* pixels,
                                    int64_t pixel_bytes, int rgb, int16_t* coef, int64_t coef_elems, uint8_t* work,
                                    int64_t work_bytes, uint8_t* out, int64_t out_bytes, int64_t* sizes) {
  REQUIRE(stage >= 1 && stage <= 3, "jpeg_encode_host: stage %d is not 1, 2 or 3", stage);
  REQUIRE(table && coef && (!(stage & 1) || pixels) && (!(stage & 2) || (work && out && sizes)),
          "jpeg_encode_host: null pointer");
  REQUIRE(((uintptr_t)coef & 1) == 0 && ((uintptr_t)work & 7) == 0, "jpeg_encode_host: coef must be 2-byte, work 8-byte aligned");
  int st = jpeg_enc_validate(table, N, (stage & 1) ? pixel_bytes : ((int64_t)1 << 62), coef_elems,
                             (stage & 2) ? work_bytes : ((int64_t)1 << 62), (stage & 2) ? out_bytes : ((int64_t)1 << 62),
                             "jpeg_encode_host");
  if (st != YV4_OK) return st;
  Tables tabs;
  for (int t = 0; t < 4; ++t) build_table(&tabs, t);
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_enc_image& im = table[n];
    if (stage & 1)
      for (int64_t i = 0; i < im.nblocks; ++i) block_coef(im, pixels, i, rgb, coef + im.coef_off + i * 64);
    if (!(stage & 2)) continue;
    const Work w = work_of(work, im);
    uint64_t pos = 0;
    for (int64_t g = 0; g < enc_wgs(im.nblocks); ++g) {
      w.wgsum[g] = pos;
      for (int64_t j = g * YV4_JPEG_ENC_WG_BLOCKS; j < im.nblocks && j < (g + 1) * YV4_JPEG_ENC_WG_BLOCKS; ++j) {
        w.bits[j] = block_bits(im, coef, j, tabs);
        pos += w.bits[j];
      }
    }
    w.totals[0] = (pos + 7) & ~(uint64_t)7;
    const int64_t nbytes = (int64_t)(w.totals[0] >> 3), nwords = enc_words(im.nblocks);
    memset(w.words, 0, (size_t)nwords * 4);
    uint32_t* words = w.words;
    auto orw = [words](int64_t k, uint32_t v) { words[k] |= v; };
    pos = 0;
    for (int64_t j = 0; j < im.nblocks; ++j) {
      block_pack(im, coef, j, pos, w.bits[j], tabs, orw);
      pos += w.bits[j];
    }
    uint64_t ff = 0;
    for (int64_t g = 0; g < enc_swgs(im.nblocks); ++g) {
      w.sff[g] = ff;
      for (int64_t k = g * YV4_JPEG_ENC_WG_BLOCKS; k < nwords && k < (g + 1) * YV4_JPEG_ENC_WG_BLOCKS; ++k) {
        word_stuff(w.words, k, nbytes, ff, out + im.out_off);
        ff += word_ffs(w.words, k, nbytes);
      }
    }
    w.totals[1] = ff;
    sizes[n] = nbytes + (int64_t)ff;
  }
  return YV4_OK;
}
