// Train-side input pipeline of the YOLOv3 mstrain recipe on the device, all pixels of a batch in one launch
// (configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78):
//   PhotoMetricDistortion (mmdet/datasets/pipelines/transforms.py:901-1004) -> Expand (:1007-1096) -> MinIoURandomCrop
//   (:1099-1236) -> Resize(img_scale=[(320, 320), (608, 608)], keep_ratio=True) -> RandomFlip -> Normalize ->
//   Pad(size_divisor=32) -> the collate that pads a ragged batch with zeros.
// The reference runs this per sample in CPU dataloader workers: float32 colour-space arithmetic on whole images.
//
// One thread per output pixel walks the chain BACKWARDS.  A pixel of the Pad / collate region is 0.  A pixel of the
// resized region undoes the flip (a permutation of that region), takes cv2.resize's four bilinear taps in the VIRTUAL
// source crop(expand(distort(src))) -- a tap outside the placed image is Expand's fill value, which is not distorted; a
// tap inside is the u8 source pixel -> float32 -> the pointwise photometric chain with this image's drawn parameters --
// then lerps across the row pair, then down, swaps BGR -> RGB and normalises.  No intermediate image (the float source,
// the distorted image, the canvas, the crop, the resized image) ever exists; the photometric chain runs once per tap.
// Random parameters are inputs: the draws, MinIoURandomCrop's acceptance loop and the box chain stay on the host
// (augment_v3.py), in the reference's order.
//
// mmcv and OpenCV are third party and absent from the build image: PARITY UNPINNED for the float pixel steps.  The kernel
// is held bit for bit to the numpy float32 restatement tests/_v3_aug_ref.py of these adopted definitions; the control
// flow, draw order, box arithmetic, fill, permutation and wrap rules are pinned by the reference's own classes
// (tests/golden/v3_augment.npz).  IEEE division only, no contraction (-ffp-contract=off), no fast-math intrinsics.
//
//   BGR -> HSV, float32, H in [0, 360) (OpenCV's scalar RGB2HSV_f): v = max(b, g, r); d = v - min(b, g, r);
//     s = d / (|v| + FLT_EPSILON); k = (float)(60.0 / (double)(d + FLT_EPSILON));
//     h = (g - b) * k if v == r, else (b - r) * k + 120 if v == g, else (r - g) * k + 240; if h < 0, h += 360.
//     Inputs may be negative or above 255: the reference does not clip after the brightness and contrast steps.
//   Saturation and hue (transforms.py:968-977): s *= gain, unclipped; h += delta, then > 360 -> -360, < 0 -> +360.
//   HSV -> BGR, float32 (scalar HSV2RGB_native): s == 0 -> (v, v, v).  Otherwise h *= 6 / 360, wrapped into [0, 6) by
//     repeated +-6; sector = floor(h), f = h - sector (sector outside 0..5: sector 0, f = 0);
//     tab = {v, v(1 - s), v(1 - s f), v(1 - s(1 - f))};
//     (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector].
//   cv2.resize INTER_LINEAR on float32: scale = (double)src / dst; f = (float)((x + 0.5) * scale - 0.5); sx = floor(f);
//     f -= sx; sx < 0 -> sx = 0, f = 0; sx >= src - 1 -> sx = src - 1, f = 0; S[sx] * (1 - f) + S[sx + 1] * f across rows
//     first, then down columns, each a float32 multiply-add without contraction.
//   Expand: fill is mean[::-1] if to_rgb; canvas int(h ratio) x int(w ratio).  Pad value 0; the collate pads with 0.
//   Normalize (mmcv.imnormalize): BGR -> RGB swap, (v - mean) * (1 / std), 1 / std computed in double.
#include "yv4_common.h"

#include <cfloat>

namespace yv4 {

// PhotoMetricDistortion's pointwise chain on one pixel (b, g, r) -> c[3] in the distorted image's channel order
__device__ __forceinline__ void v3_distort(const yv4_v3aug_image& g, float b, float gg, float r, float (&c)[3]) {
  if (g.bright_on) { b += g.bright_delta; gg += g.bright_delta; r += g.bright_delta; }
  if (g.contrast_mode == YV4_V3AUG_CONTRAST_FIRST) { b *= g.contrast_alpha; gg *= g.contrast_alpha; r *= g.contrast_alpha; }
  // BGR -> HSV
  const float v = fmaxf(fmaxf(b, gg), r);
  const float d = v - fminf(fminf(b, gg), r);
  float s = d / (fabsf(v) + FLT_EPSILON);
  const float k = (float)(60.0 / (double)(d + FLT_EPSILON));
  float h;
  if (v == r) h = (gg - b) * k;
  else if (v == gg) h = (b - r) * k + 120.f;
  else h = (r - gg) * k + 240.f;
  if (h < 0.f) h += 360.f;
  if (g.sat_on) s *= g.sat_alpha;
  if (g.hue_on) {
    h += g.hue_delta;
    if (h > 360.f) h -= 360.f;
    if (h < 0.f) h += 360.f;
  }
  // HSV -> BGR
  float ob, og, orr;
  if (s == 0.f) {
    ob = og = orr = v;
  } else {
    float hh = h * (6.f / 360.f);
    if (hh < 0.f) { do hh += 6.f; while (hh < 0.f); }
    else if (hh >= 6.f) { do hh -= 6.f; while (hh >= 6.f); }
    int sector = (int)floorf(hh);
    hh -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
    const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * hh), t3 = v * (1.f - s * (1.f - hh));
    // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], as selects (no runtime-indexed array)
    ob = sector == 0 || sector == 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
    og = sector == 0 ? t3 : (sector == 1 || sector == 2 ? t0 : (sector == 3 ? t2 : t1));
    orr = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  }
  if (g.contrast_mode == YV4_V3AUG_CONTRAST_LAST) { ob *= g.contrast_alpha; og *= g.contrast_alpha; orr *= g.contrast_alpha; }
  if (g.perm_on) {                                              // out[c] = in[perm[c]]
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = g.perm[q] == 0 ? ob : (g.perm[q] == 1 ? og : orr);
  } else {
    c[0] = ob; c[1] = og; c[2] = orr;
  }
}

// one pixel of crop(expand(distort(src))) at crop coordinates (cx, cy), 0 <= cx < cw, 0 <= cy < ch
__device__ __forceinline__ void v3_tap(const yv4_v3aug_image& g, int cx, int cy, float (&c)[3]) {
  const int lx = cx + g.cx - g.eleft, ly = cy + g.cy - g.etop;          // position in the placed image
  if ((unsigned)lx >= (unsigned)g.sw || (unsigned)ly >= (unsigned)g.sh) {
    c[0] = g.fill[0]; c[1] = g.fill[1]; c[2] = g.fill[2];
    return;
  }
  const uint8_t* px = reinterpret_cast<const uint8_t*>(g.src) + (size_t)ly * (size_t)g.pitch + (size_t)lx * 3;
  v3_distort(g, (float)px[0], (float)px[1], (float)px[2], c);
}

__device__ __forceinline__ void v3_lin_coef(int d, int dsize, int ssize, int& s0, int& s1, float& f) {
  const double scale = (double)ssize / (double)dsize;
  f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
  s0 = s;
  s1 = s + 1 < ssize ? s + 1 : s;
}

struct V3AugArgs {
  const yv4_v3aug_image* imgs;
  float* out;            // (N, 3, Hmax, Wmax)
  int N, Hmax, Wmax, to_rgb;
  float mean[3], stdinv[3];
};

__global__ __launch_bounds__(256) void v3_augment_kernel(V3AugArgs p) {
  const int X = blockIdx.x * 64 + (threadIdx.x & 63);
  const int Y = blockIdx.y * 4 + (threadIdx.x >> 6);       // one wave = 64 pixels of one row: coalesced planar stores
  const int n = blockIdx.z;
  if (X >= p.Wmax || Y >= p.Hmax) return;
  const yv4_v3aug_image& g = p.imgs[n];
  const size_t plane = (size_t)p.Hmax * p.Wmax;
  float* dst = p.out + (size_t)n * 3 * plane + (size_t)Y * p.Wmax + X;
  if (X >= g.rw || Y >= g.rh) {                                 // Pad(size_divisor) and the collate: zeros
    dst[0] = 0.f; dst[plane] = 0.f; dst[2 * plane] = 0.f;
    return;
  }
  const int xs = (g.flip & YV4_FLIP_HORIZONTAL) ? g.rw - 1 - X : X;
  const int ys = (g.flip & YV4_FLIP_VERTICAL) ? g.rh - 1 - Y : Y;
  int x0, x1, y0, y1;
  float fx, fy;
  v3_lin_coef(xs, g.rw, g.cw, x0, x1, fx);
  v3_lin_coef(ys, g.rh, g.ch, y0, y1, fy);
  float t00[3], t01[3], t10[3], t11[3];
  v3_tap(g, x0, y0, t00);
  if (x1 != x0) v3_tap(g, x1, y0, t01);
  else { t01[0] = t00[0]; t01[1] = t00[1]; t01[2] = t00[2]; }
  if (y1 != y0) {
    v3_tap(g, x0, y1, t10);
    if (x1 != x0) v3_tap(g, x1, y1, t11);
    else { t11[0] = t10[0]; t11[1] = t10[1]; t11[2] = t10[2]; }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { t10[c] = t00[c]; t11[c] = t01[c]; }
  }
  const float gx = 1.f - fx, gy = 1.f - fy;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = t00[c] * gx + t01[c] * fx;
    const float bot = t10[c] * gx + t11[c] * fx;
    v[c] = top * gy + bot * fy;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = p.to_rgb ? v[2 - c] : v[c];
    dst[c * plane] = (s - p.mean[c]) * p.stdinv[c];
  }
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_v3_augment_u8(const yv4_v3aug_image* imgs, int N, float* out_nchw, int Hmax, int Wmax,
                                 const float* mean3, const float* std3, int to_rgb, void* stream) {
  YV4_REQUIRE(imgs && out_nchw && mean3 && std3, "v3_augment: null argument");
  YV4_REQUIRE(N > 0 && N <= 65535 && Hmax > 0 && Wmax > 0, "v3_augment: bad batch or output size (N=%d, %d x %d)", N, Hmax, Wmax);
  YV4_REQUIRE((Hmax + 3) / 4 <= 65535, "v3_augment: output too tall (%d)", Hmax);
  V3AugArgs a;
  a.imgs = imgs; a.out = out_nchw; a.N = N; a.Hmax = Hmax; a.Wmax = Wmax; a.to_rgb = to_rgb ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    YV4_REQUIRE(std3[c] != 0.f, "v3_augment: std[%d] is zero", c);
    a.mean[c] = mean3[c];
    a.stdinv[c] = (float)(1.0 / (double)std3[c]);
  }
  hipLaunchKernelGGL(v3_augment_kernel, dim3((unsigned)((Wmax + 63) / 64), (unsigned)((Hmax + 3) / 4), (unsigned)N), dim3(256),
                     0, reinterpret_cast<hipStream_t>(stream), a);
  YV4_CHECK_LAUNCH("v3_augment");
  return YV4_OK;
}
