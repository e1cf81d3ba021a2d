// Shared pieces of the fp32 fused convolution kernels (conv_mfma_f32.hip: the implicit-GEMM tiles on 32x32x2 MFMAs and
// the dispatcher; conv1x1_ws_f32.hip, conv_stem_f32.hip, conv3x3_wide_f32.hip, conv_wide_f32.hip: one kernel family
// each): argument block and its fill from a descriptor, scattered-row map, the 32-bit-descriptor rule, the row
// activation and the families' host functions.
#pragma once
#include "yv4_common.h"
#include "lds_dma.h"

namespace yv4 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBK = 32;   // K slice staged per step (floats)
constexpr int kLDK = 36;  // LDS row pitch in floats: 32 + 4 pad (144 B, 16B aligned)
constexpr int kThreads = 256;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* s1;
  const float* t1;
  const float* s2;
  const float* t2;
  const float* res;
  float* y;
  int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
  int x_cs, x_co, y_cs, y_co, r_cs, r_co;
  int act1, act2;
  float slope1, slope2;
  int M, K, Kw;  // Kw: row pitch of w (== K)
  int tiles_n;
  // scattered output (sub-pixel / parity convolutions of the stride-2 data gradient): output pixel
  // (n, ho, wo) is stored at row ((n*ys_H + ho*ys_sh + ys_oh)*ys_W + wo*ys_sw + ys_ow) of y
  int ys_on, ys_H, ys_W, ys_sh, ys_sw, ys_oh, ys_ow;
  double* stats;   // training: [YV4_STATS_REPLICAS][sum (Cout) | sum of squares (Cout)] of the outputs, or null
  FastDiv fd_hw, fd_wo;   // m / (Ho*Wo), r / Wo (LDS-DMA kernels; set by launch_conv_dma)
  // split-K (LDS-DMA kernels, single-image plans): workgroup (tile, split) reduces K slices
  // [split * ks_slices, ...) and stores its RAW partial tile into slab `split` of ws ([ksplit][M][ws_cs]);
  // splitk_finish_kernel adds the slabs in slab order and applies the epilogue.  ksplit <= 1: off.
  int ksplit = 0, ks_slices = 0, ws_cs = 0;
  float* ws = nullptr;
  FastDiv fd_taps, fd_kw;   // slice -> (chunk, tap), tap -> (kh, kw) at a split's first slice
};

__device__ __forceinline__ int64_t out_row(const ConvArgs& p, int m) {
  if (!p.ys_on) return m;
  const int hw = p.Ho * p.Wo;
  const int n = m / hw;
  const int r = m - n * hw;
  const int ho = r / p.Wo;
  const int wo = r - ho * p.Wo;
  return ((int64_t)n * p.ys_H + ho * p.ys_sh + p.ys_oh) * p.ys_W + wo * p.ys_sw + p.ys_ow;
}

// The argument block of a descriptor and its tensors.  An entry sets what is particular to it afterwards (scattered
// output, split-K, statistics); the tile choice alone needs no tensors.
static inline ConvArgs conv_args(const yv4_conv_desc* d, const float* x = nullptr, const float* w = nullptr,
                          const float* s1 = nullptr, const float* t1 = nullptr, const float* s2 = nullptr,
                          const float* t2 = nullptr, const float* res = nullptr, float* y = nullptr) {
  ConvArgs a{};
  a.x = x; a.w = w; a.s1 = s1; a.t1 = t1; a.s2 = s2; a.t2 = t2; a.res = res; a.y = y;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
  a.x_cs = d->x_cstride; a.x_co = d->x_coff; a.y_cs = d->y_cstride; a.y_co = d->y_coff;
  a.r_cs = d->r_cstride; a.r_co = d->r_coff;
  a.act1 = d->act1; a.act2 = d->act2; a.slope1 = d->slope1; a.slope2 = d->slope2;
  a.M = (int)((long long)d->N * d->Ho * d->Wo); a.K = d->KH * d->KW * d->Cin; a.Kw = a.K;
  return a;
}

// the LDS-DMA kernels address x and w through 32-bit buffer descriptors
static inline long long x_bytes(const ConvArgs& a) { return (long long)a.N * a.H * a.W * a.x_cs * 4; }
static inline long long w_bytes(const ConvArgs& a) { return (long long)a.Cout * a.Kw * 4; }
static inline bool dma_addressable(const ConvArgs& a) { return desc_addressable(x_bytes(a)) && desc_addressable(w_bytes(a)); }

// the activation of a lane's 16 values behind ONE uniform branch on the activation id (see act_row4, conv_mfma_f32.hip)
__device__ __forceinline__ void act_row16(float (&v)[16], int act, float slope) {
  switch (act) {
    case YV4_ACT_MISH:
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = apply_act(v[e], YV4_ACT_MISH, 0.f);
      break;
    case YV4_ACT_LEAKY:
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = v[e] >= 0.f ? v[e] : v[e] * slope;
      break;
    case YV4_ACT_SWISH:
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = apply_act(v[e], YV4_ACT_SWISH, 0.f);
      break;
    default:
      break;
  }
}

// ---- the kernel families as the dispatcher (conv_mfma_f32.hip) sees them: the domain test and one launch function
// each, for the wide families also the shape choice (hidden: these cross translation units, not the library's boundary)
#pragma GCC visibility push(hidden)
// conv3x3_wide_f32.hip
bool conv3x3_wide_f32_applies(const ConvArgs& a);
int conv3x3_wide_f32_pick(const ConvArgs& a, double* rounds_eff);
int conv3x3_wide_f32_launch(const ConvArgs& a, int shape, hipStream_t s);
// conv_wide_f32.hip
bool conv_wide_f32_applies(const ConvArgs& a);
int conv_wide_f32_pick(const ConvArgs& a, double* rounds_eff);
int conv_wide_f32_launch(const ConvArgs& a, int shape, hipStream_t s);
// conv1x1_ws_f32.hip
int wsf_slab_cols(const ConvArgs& a);
bool conv1x1_ws_f32_applies(const ConvArgs& a);
int conv1x1_ws_f32_launch(const ConvArgs& a, hipStream_t s);
// conv_stem_f32.hip (out_dtype: YV4_F32, or YV4_F16 / YV4_BF16 for the stem of the 16-bit path)
bool stem_ok(const ConvArgs& a);
int conv_stem_f32_launch(const ConvArgs& a, int out_dtype, hipStream_t s);
#pragma GCC visibility pop

}  // namespace yv4
