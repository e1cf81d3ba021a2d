// Test-time input pipeline of the YOLOv4 configs in one kernel per image:
//   Resize(keep_ratio=True) -> Pad(size_divisor) -> Normalize(mean, std, to_rgb) -> ImageToTensor
// (configs/yolov4/yolov4l_coco_mosaic.py:70-84; mmdet/datasets/pipelines/transforms.py Resize / Pad / Normalize;
// the arithmetic itself lives in mmcv / OpenCV, which are third party and absent from the build image:
// PARITY UNPINNED -- oracle/preprocess_oracle.py restates OpenCV's documented 8-bit INTER_LINEAR (fixed point,
// modules/imgproc/src/resize.cpp) and mmcv.imnormalize's float32 subtract / multiply, and this kernel is tested
// bit for bit against that restatement only).
//
// One thread per output pixel of the padded (Hp x Wp) image: inside the resized extent it interpolates the 8-bit
// source with OpenCV's integer arithmetic (coefficients scaled by 2^11, two-stage rounding), outside it takes the
// pad value; then (v - mean) * (1 / std) per channel in fp32, channel order swapped if to_rgb; written planar
// (3, Hp, Wp) fp32 into the image's slot of the batch tensor (NCHW, what SingleStageDetector.simple_test takes).
//
// yv4_letterbox_u8_batch does the same for a whole test batch in ONE launch: a table of slots, one per (augmentation,
// image), each with its own source, extents, flip and canvas; the batch's zero padding (collate) is written too.
#include "yv4_common.h"

namespace yv4 {

struct PreArgs {
  const uint8_t* src; int sh, sw, s_pitch;      // source image, HWC, 3 channels, row pitch in bytes
  float* dst; int Hp, Wp; long long plane;      // destination planes (channel stride `plane` elements)
  int nh, nw;                                   // resized extent
  double inv_sx, inv_sy;                        // source / destination size ratios (OpenCV: scale_x = 1. / inv_scale_x)
  float mean[3], stdinv[3];
  int to_rgb, pad_val, pad_first;               // pad_first: Pad precedes Normalize (the pad value is normalised too)
  int flip;                                     // YV4_FLIP_*: bit 0 mirrors x, bit 1 mirrors y of the resized image
};

// OpenCV resize, INTER_LINEAR, 8-bit: sample position and 11-bit coefficients of one axis
__device__ __forceinline__ void lin_coef(int d, double inv_scale, int ssize, int& s0, int& s1, int& a0, int& a1) {
  float f = (float)((d + 0.5) * inv_scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }          // (OpenCV clamps the second tap to the last pixel)
  s0 = s;
  s1 = s + 1 < ssize ? s + 1 : s;
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
}

// OpenCV's two-stage fixed-point pass over the four taps, for the three channels of one pixel
__device__ __forceinline__ void bilinear_u8(const uint8_t* r0, const uint8_t* r1, int x0, int x1, int ax0, int ax1, int ay0,
                                            int ay1, int v[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[x0 * 3 + c] * ax0 + r0[x1 * 3 + c] * ax1;       // horizontal pass, 11 fractional bits
    const int h1 = r1[x0 * 3 + c] * ax0 + r1[x1 * 3 + c] * ax1;
    // vertical pass: ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16), rounded: (+ 2) >> 2
    const int r = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
  }
}

// mmcv.imnormalize of one 8-bit value: float32 subtract, then multiply by the reciprocal
__device__ __forceinline__ float normalize_u8(int v, float mean, float stdinv) { return ((float)v - mean) * stdinv; }

__global__ __launch_bounds__(256) void letterbox_u8_kernel(PreArgs p) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= p.Wp || y >= p.Hp) return;
  int v[3] = {p.pad_val, p.pad_val, p.pad_val};
  const bool inside = x < p.nw && y < p.nh;
  if (inside) {
    // RandomFlip after Resize (configs/yolo/yolov3_d53_mstrain-608_273e_coco.py test pipeline): the flip permutes the
    // resized image, so the pixel at (y, x) is the resized pixel at the mirrored position -- a gather index only
    const int xs = (p.flip & 1) ? p.nw - 1 - x : x;
    const int ys = (p.flip & 2) ? p.nh - 1 - y : y;
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    lin_coef(xs, p.inv_sx, p.sw, x0, x1, ax0, ax1);
    lin_coef(ys, p.inv_sy, p.sh, y0, y1, ay0, ay1);
    bilinear_u8(p.src + (size_t)y0 * p.s_pitch, p.src + (size_t)y1 * p.s_pitch, x0, x1, ax0, ax1, ay0, ay1, v);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = p.to_rgb ? 2 - c : c;                     // output channel c reads source channel sc
    float o;
    if (inside || p.pad_first) o = normalize_u8(v[sc], p.mean[c], p.stdinv[c]);
    else o = (float)p.pad_val;
    p.dst[(size_t)c * p.plane + (size_t)y * p.Wp + x] = o;
  }
}

// ---- the whole test batch in one launch: grid z is the slot, one (augmentation, image) pair -------------------------
struct BatchArgs {
  const yv4_letterbox_slot* slots;              // DEVICE copy of the validated table
  float* dst;
  float mean[3], stdinv[3];
  int to_rgb, pad_val, pad_first;
};

// The three output channels of pixel (y, x) of slot s: interpolated inside new, the pad value inside pad, 0 to the canvas
// (collate pads after Normalize).  The row taps (y0, y1, ay0, ay1) are the caller's: one thread's pixels share a row.
__device__ __forceinline__ void batch_pixel(const BatchArgs& p, const yv4_letterbox_slot& s, int x, int y, bool row_in,
                                            const uint8_t* r0, const uint8_t* r1, int ay0, int ay1, float o[3]) {
  if (x >= s.pad_w || y >= s.pad_h) {
    o[0] = o[1] = o[2] = 0.0f;
    return;
  }
  int v[3] = {p.pad_val, p.pad_val, p.pad_val};
  const bool inside = row_in && x < s.new_w;
  if (inside) {
    const int xs = (s.flip & 1) ? s.new_w - 1 - x : x;
    int x0, x1, ax0, ax1;
    lin_coef(xs, s.inv_sx, s.src_w, x0, x1, ax0, ax1);
    bilinear_u8(r0, r1, x0, x1, ax0, ax1, ay0, ay1, v);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = p.to_rgb ? 2 - c : c;
    o[c] = (inside || p.pad_first) ? normalize_u8(v[sc], p.mean[c], p.stdinv[c]) : (float)p.pad_val;
  }
}

// 256 threads = 4 rows x 64 lanes.  A slot whose rows and planes are 16-byte aligned (W % 4 == 0, aligned base) gives each
// lane four consecutive x and one 16-byte store per channel plane: a wave writes 1 KiB of a row per plane.  Any other slot
// (size_divisor=1, no Pad) takes one x per lane.  The choice is per slot, so uniform over a workgroup; the grid is sized
// for the slot that needs the most workgroups, and the threads beyond a slot's own canvas return.
__global__ __launch_bounds__(256) void letterbox_u8_batch_kernel(BatchArgs p) {
  const yv4_letterbox_slot s = p.slots[blockIdx.z];
  float* dst = p.dst + s.dst_off;
  const bool vec = (s.W & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int lane = blockIdx.x * 64 + (threadIdx.x & 63);
  const int x = vec ? lane * 4 : lane;
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= s.W || y >= s.H) return;
  const bool row_in = y < s.new_h;
  const uint8_t *r0 = s.src, *r1 = s.src;
  int ay0 = 0, ay1 = 0;
  if (row_in) {
    const int ys = (s.flip & 2) ? s.new_h - 1 - y : y;
    int y0, y1;
    lin_coef(ys, s.inv_sy, s.src_h, y0, y1, ay0, ay1);
    r0 = s.src + (size_t)y0 * s.src_pitch;
    r1 = s.src + (size_t)y1 * s.src_pitch;
  }
  const size_t plane = (size_t)s.H * s.W, at = (size_t)y * s.W + x;
  if (vec) {                                     // x + 3 < W, as W % 4 == 0
    float o[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) batch_pixel(p, s, x + k, y, row_in, r0, r1, ay0, ay1, o[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(dst + c * plane + at) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
  } else {
    float o[3];
    batch_pixel(p, s, x, y, row_in, r0, r1, ay0, ay1, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * plane + at] = o[c];
  }
}

}  // namespace yv4

using namespace yv4;

static int letterbox_impl(const uint8_t* src, int src_h, int src_w, int src_pitch, float* dst, int Hp, int Wp,
                          int64_t plane_stride, int new_h, int new_w, const float* mean3, const float* std3,
                          int to_rgb, int pad_val, int pad_before_normalize, int flip, void* stream) {
  YV4_REQUIRE(src && dst && mean3 && std3, "letterbox: null pointer");
  YV4_REQUIRE(src_h > 0 && src_w > 0 && src_pitch >= 3 * src_w && Hp > 0 && Wp > 0 && plane_stride >= (int64_t)Hp * Wp,
              "letterbox: bad geometry");
  YV4_REQUIRE(new_h > 0 && new_w > 0 && new_h <= Hp && new_w <= Wp, "letterbox: the resized image exceeds the padded one");
  YV4_REQUIRE(flip >= YV4_FLIP_NONE && flip <= YV4_FLIP_DIAGONAL, "letterbox: bad flip direction %d", flip);
  YV4_REQUIRE(pad_val >= 0 && pad_val <= 255, "letterbox: pad value must be an 8-bit value");
  PreArgs a;
  a.src = src; a.sh = src_h; a.sw = src_w; a.s_pitch = src_pitch;
  a.dst = dst; a.Hp = Hp; a.Wp = Wp; a.plane = plane_stride;
  a.nh = new_h; a.nw = new_w;
  a.inv_sx = 1.0 / ((double)new_w / (double)src_w);     // OpenCV: scale_x = 1. / ((double)dsize.width / ssize.width)
  a.inv_sy = 1.0 / ((double)new_h / (double)src_h);
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3[c];
    a.stdinv[c] = (float)(1.0 / (double)std3[c]);
  }
  a.to_rgb = to_rgb ? 1 : 0; a.pad_val = pad_val; a.pad_first = pad_before_normalize ? 1 : 0;
  a.flip = flip;
  hipLaunchKernelGGL(letterbox_u8_kernel, dim3((unsigned)((Wp + 63) / 64), (unsigned)((Hp + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  YV4_CHECK_LAUNCH("letterbox_u8");
  return YV4_OK;
}

extern "C" int yv4_letterbox_u8(const uint8_t* src, int src_h, int src_w, int src_pitch, float* dst, int Hp, int Wp,
                                int64_t plane_stride, int new_h, int new_w, const float* mean3, const float* std3,
                                int to_rgb, int pad_val, int pad_before_normalize, void* stream) {
  return letterbox_impl(src, src_h, src_w, src_pitch, dst, Hp, Wp, plane_stride, new_h, new_w, mean3, std3, to_rgb,
                        pad_val, pad_before_normalize, YV4_FLIP_NONE, stream);
}

extern "C" int yv4_letterbox_u8_flip(const uint8_t* src, int src_h, int src_w, int src_pitch, float* dst, int Hp,
                                     int Wp, int64_t plane_stride, int new_h, int new_w, const float* mean3,
                                     const float* std3, int to_rgb, int pad_val, int pad_before_normalize, int flip,
                                     void* stream) {
  return letterbox_impl(src, src_h, src_w, src_pitch, dst, Hp, Wp, plane_stride, new_h, new_w, mean3, std3, to_rgb,
                        pad_val, pad_before_normalize, flip, stream);
}

extern "C" int yv4_letterbox_u8_batch(const yv4_letterbox_slot* table, const yv4_letterbox_slot* table_dev, int N,
                                      float* dst, int64_t dst_elems, const float* mean3, const float* std3, int to_rgb,
                                      int pad_val, int pad_before_normalize, void* stream) {
  YV4_REQUIRE(table && table_dev && dst && mean3 && std3, "letterbox_batch: null pointer");
  YV4_REQUIRE(N > 0 && N <= 65535 && dst_elems > 0, "letterbox_batch: %d slots (1 .. 65535) or an empty destination", N);
  YV4_REQUIRE((reinterpret_cast<uintptr_t>(table_dev) & 7) == 0, "letterbox_batch: table_dev must be 8-byte aligned");
  YV4_REQUIRE(pad_val >= 0 && pad_val <= 255, "letterbox_batch: pad value must be an 8-bit value");
  // the kernel trusts the table: everything it indexes with is checked here, on the host copy
  int gx = 0, gy = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_letterbox_slot& s = table[n];
    YV4_REQUIRE(s.src, "letterbox_batch: slot %d: null source", n);
    YV4_REQUIRE(s.src_h > 0 && s.src_w > 0 && s.src_pitch >= 3 * (int64_t)s.src_w && s.H > 0 && s.W > 0,
                "letterbox_batch: slot %d: bad geometry", n);
    YV4_REQUIRE(s.new_h > 0 && s.new_w > 0 && s.new_h <= s.pad_h && s.new_w <= s.pad_w,
                "letterbox_batch: slot %d: the resized image exceeds the padded one", n);
    YV4_REQUIRE(s.pad_h <= s.H && s.pad_w <= s.W, "letterbox_batch: slot %d: the padded image (%d x %d) exceeds its canvas "
                "(%d x %d)", n, s.pad_h, s.pad_w, s.H, s.W);
    YV4_REQUIRE(s.flip >= YV4_FLIP_NONE && s.flip <= YV4_FLIP_DIAGONAL, "letterbox_batch: slot %d: bad flip direction %d", n,
                s.flip);
    YV4_REQUIRE(s.inv_sx == 1.0 / ((double)s.new_w / (double)s.src_w) && s.inv_sy == 1.0 / ((double)s.new_h / (double)s.src_h),
                "letterbox_batch: slot %d: the resize ratios do not follow from its sizes", n);
    const int64_t elems = 3 * (int64_t)s.H * s.W;
    YV4_REQUIRE(s.dst_off >= 0 && elems <= dst_elems && s.dst_off <= dst_elems - elems,
                "letterbox_batch: slot %d: its canvas leaves the destination buffer", n);
    const bool vec = (s.W & 3) == 0 && (reinterpret_cast<uintptr_t>(dst + s.dst_off) & 15) == 0;     // the kernel's rule
    const int lanes = vec ? s.W / 4 : s.W;
    gx = std::max(gx, (lanes + 63) / 64);
    gy = std::max(gy, (s.H + 3) / 4);
  }
  YV4_REQUIRE(gy <= 65535, "letterbox_batch: a canvas of more than 262140 rows");
  BatchArgs a;
  a.slots = table_dev; a.dst = dst;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3[c];
    a.stdinv[c] = (float)(1.0 / (double)std3[c]);
  }
  a.to_rgb = to_rgb ? 1 : 0; a.pad_val = pad_val; a.pad_first = pad_before_normalize ? 1 : 0;
  hipLaunchKernelGGL(letterbox_u8_batch_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  YV4_CHECK_LAUNCH("letterbox_u8_batch");
  return YV4_OK;
}
