// Boxes and labels onto images in place (include/yv4.h, "drawing detections"): one launch per batch, one lane per pixel.
// A pixel takes the LAST box of its image, in input order, whose label or frame covers it -- the label over the frame --
// so no lane writes another's pixel, nothing is atomic and the result does not depend on any order.  The rule is the
// package's own (the reference renders through matplotlib with anti-aliased text, which cannot be reproduced);
// tests/_draw_ref.py restates it in numpy and the kernel equals it bit for bit.  yv4_draw_boxes_host runs the same
// per-pixel function on the CPU.
#include <hip/hip_runtime.h>

#include "yv4_common.h"

#if defined(__HIPCC__) && defined(__HIP__)
#define YV4_DRAW_HD __host__ __device__ __forceinline__
#else
#define YV4_DRAW_HD inline
#endif

namespace yv4 {
namespace draw {

constexpr int kWg = 256;

// the glyph of character c (0x20 .. 0x7E) at column x (0 .. 4), row y (0 .. 6): five column bytes a glyph, bit 0 the top row
YV4_DRAW_HD bool glyph_bit(int c, int x, int y) {
  const uint8_t kFont[95][5] = {
      {0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x5F, 0x00, 0x00}, {0x00, 0x07, 0x00, 0x07, 0x00}, {0x14, 0x7F, 0x14, 0x7F, 0x14}, {0x24, 0x2A, 0x7F, 0x2A, 0x12},  //  !"#$
      {0x23, 0x13, 0x08, 0x64, 0x62}, {0x36, 0x49, 0x55, 0x22, 0x50}, {0x00, 0x05, 0x03, 0x00, 0x00}, {0x00, 0x1C, 0x22, 0x41, 0x00}, {0x00, 0x41, 0x22, 0x1C, 0x00},  // %&'()
      {0x14, 0x08, 0x3E, 0x08, 0x14}, {0x08, 0x08, 0x3E, 0x08, 0x08}, {0x00, 0x50, 0x30, 0x00, 0x00}, {0x08, 0x08, 0x08, 0x08, 0x08}, {0x00, 0x60, 0x60, 0x00, 0x00},  // *+,-.
      {0x20, 0x10, 0x08, 0x04, 0x02}, {0x3E, 0x51, 0x49, 0x45, 0x3E}, {0x00, 0x42, 0x7F, 0x40, 0x00}, {0x42, 0x61, 0x51, 0x49, 0x46}, {0x21, 0x41, 0x45, 0x4B, 0x31},  // /0123
      {0x18, 0x14, 0x12, 0x7F, 0x10}, {0x27, 0x45, 0x45, 0x45, 0x39}, {0x3C, 0x4A, 0x49, 0x49, 0x30}, {0x01, 0x71, 0x09, 0x05, 0x03}, {0x36, 0x49, 0x49, 0x49, 0x36},  // 45678
      {0x06, 0x49, 0x49, 0x29, 0x1E}, {0x00, 0x36, 0x36, 0x00, 0x00}, {0x00, 0x56, 0x36, 0x00, 0x00}, {0x08, 0x14, 0x22, 0x41, 0x00}, {0x14, 0x14, 0x14, 0x14, 0x14},  // 9:;<=
      {0x00, 0x41, 0x22, 0x14, 0x08}, {0x02, 0x01, 0x51, 0x09, 0x06}, {0x32, 0x49, 0x79, 0x41, 0x3E}, {0x7E, 0x11, 0x11, 0x11, 0x7E}, {0x7F, 0x49, 0x49, 0x49, 0x36},  // >?@AB
      {0x3E, 0x41, 0x41, 0x41, 0x22}, {0x7F, 0x41, 0x41, 0x22, 0x1C}, {0x7F, 0x49, 0x49, 0x49, 0x41}, {0x7F, 0x09, 0x09, 0x09, 0x01}, {0x3E, 0x41, 0x49, 0x49, 0x7A},  // CDEFG
      {0x7F, 0x08, 0x08, 0x08, 0x7F}, {0x00, 0x41, 0x7F, 0x41, 0x00}, {0x20, 0x40, 0x41, 0x3F, 0x01}, {0x7F, 0x08, 0x14, 0x22, 0x41}, {0x7F, 0x40, 0x40, 0x40, 0x40},  // HIJKL
      {0x7F, 0x02, 0x0C, 0x02, 0x7F}, {0x7F, 0x04, 0x08, 0x10, 0x7F}, {0x3E, 0x41, 0x41, 0x41, 0x3E}, {0x7F, 0x09, 0x09, 0x09, 0x06}, {0x3E, 0x41, 0x51, 0x21, 0x5E},  // MNOPQ
      {0x7F, 0x09, 0x19, 0x29, 0x46}, {0x46, 0x49, 0x49, 0x49, 0x31}, {0x01, 0x01, 0x7F, 0x01, 0x01}, {0x3F, 0x40, 0x40, 0x40, 0x3F}, {0x1F, 0x20, 0x40, 0x20, 0x1F},  // RSTUV
      {0x3F, 0x40, 0x38, 0x40, 0x3F}, {0x63, 0x14, 0x08, 0x14, 0x63}, {0x07, 0x08, 0x70, 0x08, 0x07}, {0x61, 0x51, 0x49, 0x45, 0x43}, {0x00, 0x7F, 0x41, 0x41, 0x00},  // WXYZ[
      {0x02, 0x04, 0x08, 0x10, 0x20}, {0x00, 0x41, 0x41, 0x7F, 0x00}, {0x04, 0x02, 0x01, 0x02, 0x04}, {0x40, 0x40, 0x40, 0x40, 0x40}, {0x00, 0x01, 0x02, 0x04, 0x00},  // backslash ]^_`
      {0x20, 0x54, 0x54, 0x54, 0x78}, {0x7F, 0x48, 0x44, 0x44, 0x38}, {0x38, 0x44, 0x44, 0x44, 0x20}, {0x38, 0x44, 0x44, 0x48, 0x7F}, {0x38, 0x54, 0x54, 0x54, 0x18},  // abcde
      {0x08, 0x7E, 0x09, 0x01, 0x02}, {0x0C, 0x52, 0x52, 0x52, 0x3E}, {0x7F, 0x08, 0x04, 0x04, 0x78}, {0x00, 0x44, 0x7D, 0x40, 0x00}, {0x20, 0x40, 0x44, 0x3D, 0x00},  // fghij
      {0x7F, 0x10, 0x28, 0x44, 0x00}, {0x00, 0x41, 0x7F, 0x40, 0x00}, {0x7C, 0x04, 0x18, 0x04, 0x78}, {0x7C, 0x08, 0x04, 0x04, 0x78}, {0x38, 0x44, 0x44, 0x44, 0x38},  // klmno
      {0x7C, 0x14, 0x14, 0x14, 0x08}, {0x08, 0x14, 0x14, 0x18, 0x7C}, {0x7C, 0x08, 0x04, 0x04, 0x08}, {0x48, 0x54, 0x54, 0x54, 0x20}, {0x04, 0x3F, 0x44, 0x40, 0x20},  // pqrst
      {0x3C, 0x40, 0x40, 0x20, 0x7C}, {0x1C, 0x20, 0x40, 0x20, 0x1C}, {0x3C, 0x40, 0x30, 0x40, 0x3C}, {0x44, 0x28, 0x10, 0x28, 0x44}, {0x0C, 0x50, 0x50, 0x50, 0x3C},  // uvwxy
      {0x44, 0x64, 0x54, 0x4C, 0x44}, {0x00, 0x08, 0x36, 0x41, 0x00}, {0x00, 0x00, 0x7F, 0x00, 0x00}, {0x00, 0x41, 0x36, 0x08, 0x00}, {0x10, 0x08, 0x08, 0x10, 0x08},  // z{|}~
};
  return (kFont[c - 0x20][x] >> y) & 1;
}

YV4_DRAW_HD int trunc_coord(float v) {      // int32 truncation; NaN and values past +-2^30 are clamped first
  if (!(v > -1073741824.0f)) return -1073741824;
  if (!(v < 1073741824.0f)) return 1073741824;
  return (int)v;
}

// character k of box's label: the class name, then '|', then the score as d.dd (floor(score * 100 + 0.5) in float32);
// with YV4_DRAW_NO_SCORE the name is the whole label and this is never asked for k >= len.
// A name byte outside 0x20 .. 0x7E reads as '?', whoever made the table: the glyph table is never indexed outside.
YV4_DRAW_HD int label_char(const uint8_t* name, int len, float score, int k) {
  if (k < len) {
    const int c = name[1 + k];
    return c >= 0x20 && c <= 0x7E ? c : '?';
  }
  float f = floorf(score * 100.0f + 0.5f);
  f = f < 0.0f ? 0.0f : (f > 999.0f ? 999.0f : f);
  const int v = (int)f;
  switch (k - len) {
    case 0: return '|';
    case 1: return '0' + v / 100;
    case 2: return '.';
    case 3: return '0' + v / 10 % 10;
    default: return '0' + v % 10;
  }
}

enum Paint { kKeep = 0, kFrame = 1, kText = 2, kDim = 3 };      // what a pixel becomes: itself, bbox_color, text_color, itself / 5

// what pixel (x, y) of image im becomes: decided once a pixel, by the last box whose label or frame covers it
YV4_DRAW_HD Paint decide(const yv4_draw_image& im, const float* dets, const int32_t* labels, const uint8_t* names,
                         const yv4_draw_style& st, int flags, int x, int y) {
  const int s = st.font_size / 7 > 1 ? st.font_size / 7 : 1;
  const bool scored = !(flags & YV4_DRAW_NO_SCORE);
  const int tail = scored ? 5 : 0;      // the characters behind the name: '|' and d.dd
  for (int64_t k = im.box_base + im.nbox - 1; k >= im.box_base; --k) {
    const float* d = dets + 5 * k;
    const float score = scored ? d[4] : 0.0f;
    if (scored && !(score > st.score_thr)) continue;
    const int x1 = trunc_coord(d[0]), y1 = trunc_coord(d[1]), x2 = trunc_coord(d[2]), y2 = trunc_coord(d[3]);
    // the label: its top-left at (x1, y1); one scaled pixel of padding, 5 + 1 columns a character, 7 rows
    const int lab = labels[k];
    const uint8_t* name = names + (int64_t)(lab >= 0 && lab < st.num_classes ? lab : st.num_classes) * YV4_DRAW_NAME_BYTES;
    const int len = name[0] < YV4_DRAW_NAME_BYTES ? name[0] : YV4_DRAW_NAME_BYTES - 1;
    const int64_t lx = (int64_t)x - x1, ly = (int64_t)y - y1;
    if (lx >= 0 && ly >= 0 && lx < (int64_t)s * (1 + 6 * (len + tail)) && ly < 9 * s) {
      const int gx = (int)lx / s - 1, gy = (int)ly / s - 1;
      if (gx >= 0 && gy >= 0 && gy < 7 && gx % 6 < 5 && glyph_bit(label_char(name, len, score, gx / 6), gx % 6, gy))
        return kText;
      return kDim;
    }
    // the frame: `thickness` pixels inward from the rectangle [x1, x2] x [y1, y2]
    if (x >= x1 && x <= x2 && y >= y1 && y <= y2) {
      const int64_t t = st.thickness;
      if ((int64_t)x - x1 < t || (int64_t)x2 - x < t || (int64_t)y - y1 < t || (int64_t)y2 - y < t) return kFrame;
    }
  }
  return kKeep;
}

// the three bytes at p after the decision
YV4_DRAW_HD void paint(uint8_t* p, Paint what, const yv4_draw_style& st) {
  if (what == kKeep) return;
  for (int ch = 0; ch < 3; ++ch)
    p[ch] = what == kFrame ? (uint8_t)st.bbox_color[ch] : (what == kText ? (uint8_t)st.text_color[ch] : (uint8_t)(p[ch] / 5));
}

__global__ __launch_bounds__(kWg) void draw_kernel(const yv4_draw_image* __restrict__ table, int N, uint8_t* __restrict__ pixels,
                                                   const float* __restrict__ dets, const int32_t* __restrict__ labels,
                                                   const uint8_t* __restrict__ names, yv4_draw_style st, int flags) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {      // the image of this workgroup: the last one whose base is <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].wg_base <= (int64_t)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const yv4_draw_image im = table[lo];
  const int64_t i = ((int64_t)blockIdx.x - im.wg_base) * kWg + (int)threadIdx.x;
  if (im.nbox == 0 || i >= (int64_t)im.width * im.height) return;
  const int y = (int)(i / im.width), x = (int)(i % im.width);
  uint8_t* p = pixels + im.pix_off + (int64_t)y * im.pitch + 3 * x;
  paint(p, decide(im, dets, labels, names, st, flags, x, y), st);
}

static int64_t wgs_of(const yv4_draw_image& im) { return ((int64_t)im.width * im.height + kWg - 1) / kWg; }

static int validate(const char* who, const yv4_draw_image* table, int N, int64_t pixel_bytes, int64_t nbox_total,
                    const yv4_draw_style* st, int flags) {
  YV4_REQUIRE(table && st && N >= 1, "%s: null pointer or no images", who);
  YV4_REQUIRE((flags & ~YV4_DRAW_NO_SCORE) == 0, "%s: flags 0x%x holds a bit other than YV4_DRAW_NO_SCORE", who, flags);
  YV4_REQUIRE(st->thickness >= 1 && st->font_size >= 1 && st->font_size <= 7 * 64 && st->num_classes >= 0,
              "%s: thickness %d and font_size %d must be at least 1 (font_size at most 448)", who, st->thickness, st->font_size);
  for (int c = 0; c < 3; ++c)
    YV4_REQUIRE(st->bbox_color[c] >= 0 && st->bbox_color[c] <= 255 && st->text_color[c] >= 0 && st->text_color[c] <= 255,
                "%s: a colour channel outside 0 .. 255", who);
  int64_t wg = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_draw_image& im = table[n];
    YV4_REQUIRE(im.width >= 1 && im.height >= 1 && im.pitch >= 3 * (int64_t)im.width, "%s: image %d: %d x %d at pitch %d", who,
                n, im.height, im.width, im.pitch);
    YV4_REQUIRE(im.pix_off >= 0 && im.pix_off <= pixel_bytes &&
                    (int64_t)(im.height - 1) * im.pitch + 3 * (int64_t)im.width <= pixel_bytes - im.pix_off,
                "%s: image %d: its pixels (offset %lld) lie outside the buffer of %lld bytes", who, n, (long long)im.pix_off,
                (long long)pixel_bytes);
    YV4_REQUIRE(im.nbox >= 0 && im.box_base >= 0 && im.box_base <= nbox_total && im.nbox <= nbox_total - im.box_base,
                "%s: image %d: boxes %lld .. +%d of %lld", who, n, (long long)im.box_base, im.nbox, (long long)nbox_total);
    YV4_REQUIRE(im.wg_base == wg, "%s: image %d: workgroup base %lld, expected %lld", who, n, (long long)im.wg_base, (long long)wg);
    wg += wgs_of(im);
    // 256 lanes a workgroup: the grid's lanes stay below 2^32, the tightest launch limit among HIP runtimes
    YV4_REQUIRE(wg < ((int64_t)1 << 24), "%s: the batch is too large for one launch (2^24 workgroups of 256 pixels)", who);
  }
  return YV4_OK;
}

}  // namespace draw
}  // namespace yv4

using namespace yv4;

extern "C" int yv4_draw_layout(yv4_draw_image* table, int N, int64_t* workgroups) {
  YV4_REQUIRE(table && workgroups && N >= 1, "draw_layout: null pointer or no images");
  int64_t wg = 0;
  for (int n = 0; n < N; ++n) {
    YV4_REQUIRE(table[n].width >= 1 && table[n].height >= 1, "draw_layout: image %d is empty", n);
    table[n].wg_base = wg;
    wg += draw::wgs_of(table[n]);
  }
  *workgroups = wg;
  return YV4_OK;
}

extern "C" int yv4_draw_boxes_ex(const yv4_draw_image* table, const yv4_draw_image* table_dev, int N, uint8_t* pixels,
                                 int64_t pixel_bytes, const float* dets, const int32_t* labels, int64_t nbox_total,
                                 const uint8_t* names, const yv4_draw_style* style, int flags, void* stream) {
  YV4_REQUIRE(table_dev && pixels && names && (nbox_total == 0 || (dets && labels)), "draw_boxes: null pointer");
  const int st = draw::validate("draw_boxes", table, N, pixel_bytes, nbox_total, style, flags);
  if (st != YV4_OK) return st;
  const int64_t nwg = table[N - 1].wg_base + draw::wgs_of(table[N - 1]);
  hipLaunchKernelGGL(draw::draw_kernel, dim3((unsigned)nwg), dim3(draw::kWg), 0, reinterpret_cast<hipStream_t>(stream),
                     table_dev, N, pixels, dets, labels, names, *style, flags);
  YV4_CHECK_LAUNCH("draw_boxes");
  return YV4_OK;
}

extern "C" int yv4_draw_boxes(const yv4_draw_image* table, const yv4_draw_image* table_dev, int N, uint8_t* pixels,
                              int64_t pixel_bytes, const float* dets, const int32_t* labels, int64_t nbox_total,
                              const uint8_t* names, const yv4_draw_style* style, void* stream) {
  return yv4_draw_boxes_ex(table, table_dev, N, pixels, pixel_bytes, dets, labels, nbox_total, names, style, 0, stream);
}

extern "C" int yv4_draw_boxes_host_ex(const yv4_draw_image* table, int N, uint8_t* pixels, int64_t pixel_bytes,
                                      const float* dets, const int32_t* labels, int64_t nbox_total, const uint8_t* names,
                                      const yv4_draw_style* style, int flags) {
  YV4_REQUIRE(pixels && names && (nbox_total == 0 || (dets && labels)), "draw_boxes_host: null pointer");
  const int st = draw::validate("draw_boxes_host", table, N, pixel_bytes, nbox_total, style, flags);
  if (st != YV4_OK) return st;
  for (int n = 0; n < N; ++n) {
    const yv4_draw_image& im = table[n];
    for (int y = 0; y < im.height; ++y)
      for (int x = 0; x < im.width; ++x) {
        uint8_t* p = pixels + im.pix_off + (int64_t)y * im.pitch + 3 * x;
        draw::paint(p, draw::decide(im, dets, labels, names, *style, flags, x, y), *style);
      }
  }
  return YV4_OK;
}

extern "C" int yv4_draw_boxes_host(const yv4_draw_image* table, int N, uint8_t* pixels, int64_t pixel_bytes,
                                   const float* dets, const int32_t* labels, int64_t nbox_total, const uint8_t* names,
                                   const yv4_draw_style* style) {
  return yv4_draw_boxes_host_ex(table, N, pixels, pixel_bytes, dets, labels, nbox_total, names, style, 0);
}
