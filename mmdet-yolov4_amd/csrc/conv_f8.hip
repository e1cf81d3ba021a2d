// FP8 (OCP e4m3fn) inference kernels for gfx950: the fused implicit-GEMM convolution with e4m3 operands and fp32
// accumulation, the quantize op at the 16-bit -> fp8 boundary of a plan, and the SPP max-pools on e4m3 codes.
//
// Numerics.  A code is  e4m3(clamp(v * inv_s, -448, 448))  rounded to nearest even; inv_s = 1/s
// is computed on the host.  Activations carry one fp32 scale per plan buffer, weights one per output channel; both are
// folded into the stage-1 affine on the host (s1' = s1 * sw[co] * sx), so the matrix core runs with unit block scales
// (E8M0 127) and the epilogue is the chain of the 16-bit kernels:  acc*s1'+t1 -> act1 -> + r_scale*residual ->
// act2(v*s2+t2) -> e4m3 via the output buffer's inv_s, or fp32 (pred maps).
//
// Conversion is done in integer arithmetic (f32_to_e4m3 / e4m3_to_f32 below) rather than by the packed conversion
// instructions, so that the bits are those of torch.float8_e4m3fn by construction, including subnormals and ties.
//
// GEMM view as conv_mfma_h16.hip: M = N*Ho*Wo pixels, Ncol = Cout, K = KH*KW*Cin ordered (kh, kw, ci).  A K slice is
// 128 codes = one 128-byte LDS row per pixel / output channel, eight 16-byte chunks XOR-swizzled with (row & 7).  The
// workgroup (4 waves, 2 x 2) stages slice k+1 through registers while the MFMAs run on slice k (two LDS buffers, one
// barrier per slice).  Out-of-range chunks -- padding taps, the M tail, the Cout tail, the K tail -- are zeros.
//
// MFMA: v_mfma_scale_f32_32x32x64_f8f6f4, format 0 (e4m3) on both operands.  Lane (r, h) supplies row r of its
// operand and 32 consecutive K codes of the 64 of a step (bytes 32h .. 32h+31 of the step's 64-byte half row).  Only
// the ROW map matters for correctness: A and B take their K codes from the same (lane, byte) positions, and a dot
// product is invariant under a common permutation of K.  The accumulator layout is that of every 32x32 MFMA (lane
// (r, h) holds column r, rows 8*(e>>2) + 4h + (e&3)); tests/test_gpu_fp8.py checks both maps with integer data, bit
// for bit.
#include "yv4_common.h"
#include "conv_desc.h"

namespace yv4 {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// ---- e4m3fn <-> fp32 --------------------------------------------------------------------------------------------------
// v must already be clamped to [-448, 448] (448 = 0x7E, the largest finite code; 0x7F / 0xFF are NaN, never produced).
__device__ __forceinline__ unsigned f32_to_e4m3(float v) {
  const unsigned bits = __float_as_uint(v);
  const unsigned sign = (bits >> 24) & 0x80u;
  const float a = fabsf(v);
  unsigned code;
  if (a < 0.015625f) {                       // below 2^-6: subnormal codes, units of 2^-9 (exact scaling, RNE by rintf)
    code = (unsigned)rintf(a * 512.f);       // 8 = 0x08 is the smallest normal: same bits
  } else {                                   // keep 3 of the 23 mantissa bits, round to nearest even
    const unsigned b = __float_as_uint(a);
    const unsigned r = (b + 0x7FFFFu + ((b >> 20) & 1u)) >> 20;
    code = r - (120u << 3);                  // rebias 127 -> 7
  }
  return sign | code;
}

__device__ __forceinline__ float e4m3_to_f32(unsigned c) {
  const unsigned e = (c >> 3) & 15u, m = c & 7u;
  const float a = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
  return (c & 0x80u) ? -a : a;
}

__device__ __forceinline__ unsigned quant_e4m3(float v, float inv_s) {
  const float q = fminf(fmaxf(v * inv_s, -448.f), 448.f);
  return f32_to_e4m3(q);
}

// ---- the convolution ----------------------------------------------------------------------------------------------
constexpr int kF8BK = 128;       // K slice (codes = bytes)
constexpr int kF8Threads = 256;

struct ConvArgsF8 {
  const unsigned char* x;
  const unsigned char* w;
  const float* s1;
  const float* t1;
  const float* s2;
  const float* t2;
  const unsigned char* res;
  void* y;
  int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
  int x_cs, x_co, y_cs, y_co, r_cs, r_co;
  int act1, act2;
  float slope1, slope2;
  float r_scale, y_inv;
  int out_f32;
  int M, K;
  int tiles_n;
};

// The argument block of a descriptor and its tensors (the shape of conv_args, conv_f32_common.h); the launch sets tiles_n.
static inline ConvArgsF8 conv_args_f8(const yv4_conv_desc* d, int out_f32, const void* x, const void* w, const float* s1,
                                      const float* t1, const float* s2, const float* t2, const void* res, float r_scale,
                                      float y_inv, void* y) {
  ConvArgsF8 a{};
  a.x = (const unsigned char*)x; a.w = (const unsigned char*)w; a.s1 = s1; a.t1 = t1; a.s2 = s2; a.t2 = t2;
  a.res = (const unsigned char*)res; a.y = y;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
  a.x_cs = d->x_cstride; a.x_co = d->x_coff; a.y_cs = d->y_cstride; a.y_co = d->y_coff;
  a.r_cs = d->r_cstride; a.r_co = d->r_coff;
  a.act1 = d->act1; a.act2 = d->act2; a.slope1 = d->slope1; a.slope2 = d->slope2;
  a.r_scale = r_scale; a.y_inv = y_inv; a.out_f32 = out_f32;
  a.M = (int)((long long)d->N * d->Ho * d->Wo); a.K = d->KH * d->KW * d->Cin;
  return a;
}

// GENERAL_K = false: Cin % 128 == 0, a slice lies inside one (kh, kw) tap (scalar walk).  GENERAL_K = true: Cin % 16
// == 0, each 16-byte chunk derives its own (tap, channel).
template <int BM, int BN, bool GENERAL_K>
__global__ __launch_bounds__(kF8Threads, 2) void conv_f8_kernel(ConvArgsF8 p) {
  constexpr int TM = BM / 64;            // 32x32 tiles per wave, 2 x 2 waves
  constexpr int TN = BN / 64;
  constexpr int PA = BM * 8 / kF8Threads;  // 16-byte chunks staged per thread and slice
  constexpr int PB = BN * 8 / kF8Threads;
  constexpr int kRowB = 128;
  extern __shared__ __attribute__((aligned(16))) char smem_f8[];
  char* As = smem_f8;                       // [2][BM][128 B]
  char* Bs = smem_f8 + 2 * BM * kRowB;      // [2][BN][128 B]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int tile_n = blockIdx.x % p.tiles_n;
  const int tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // staging: chunk id = tid + 256 q -> row id >> 3, logical chunk id & 7 (the same for every q)
  const int lc = tid & 7;
  int a_hi0[PA], a_wi0[PA];
  long long a_base[PA];
#pragma unroll
  for (int q = 0; q < PA; ++q) {
    const int m = m0 + ((tid + kF8Threads * q) >> 3);
    if (m < p.M) {
      const int hw = p.Ho * p.Wo;
      const int n = m / hw;
      const int rm = m - n * hw;
      const int ho = rm / p.Wo;
      const int wo = rm - ho * p.Wo;
      a_hi0[q] = ho * p.stride - p.pad;
      a_wi0[q] = wo * p.stride - p.pad;
      a_base[q] = (long long)n * p.H * p.W;
    } else {
      a_hi0[q] = -(1 << 29);               // every tap out of range
      a_wi0[q] = 0;
      a_base[q] = 0;
    }
  }

  uint4 ra[PA], rb[PB];
  auto load_slice = [&](int kt) {
    const int kb = kt * kF8BK;
    int tap, c;
    if (GENERAL_K) {
      const int k = kb + lc * 16;
      tap = k / p.Cin;
      c = k - tap * p.Cin;
    } else {
      tap = kb / p.Cin;
      c = kb - tap * p.Cin + lc * 16;
    }
    const bool kin = kb + lc * 16 < p.K;
    const int kh = tap / p.KW, kw = tap - (tap / p.KW) * p.KW;
#pragma unroll
    for (int q = 0; q < PA; ++q) {
      const int hi = a_hi0[q] + kh, wi = a_wi0[q] + kw;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (kin && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
        v = *reinterpret_cast<const uint4*>(p.x + ((a_base[q] + (long long)hi * p.W + wi) * p.x_cs + p.x_co + c));
      ra[q] = v;
    }
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      const int co = n0 + ((tid + kF8Threads * q) >> 3);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (kin && co < p.Cout) v = *reinterpret_cast<const uint4*>(p.w + ((long long)co * p.K + kb + lc * 16));
      rb[q] = v;
    }
  };
  auto store_slice = [&](int buf) {
#pragma unroll
    for (int q = 0; q < PA; ++q) {
      const int row = (tid + kF8Threads * q) >> 3;
      *reinterpret_cast<uint4*>(As + (buf * BM + row) * kRowB + ((lc ^ (row & 7)) << 4)) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      const int row = (tid + kF8Threads * q) >> 3;
      *reinterpret_cast<uint4*>(Bs + (buf * BN + row) * kRowB + ((lc ^ (row & 7)) << 4)) = rb[q];
    }
  };

  f32x16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = (p.K + kF8BK - 1) / kF8BK;
  load_slice(0);
  store_slice(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_slice(kt + 1);
    const char* as_ = As + buf * BM * kRowB;
    const char* bs_ = Bs + buf * BN * kRowB;
#pragma unroll
    for (int j = 0; j < 2; ++j) {          // two 64-code MFMA steps per slice
      i32x8_t fa[TM], fb[TN];
      const int c0 = 4 * j + 2 * h;        // this lane's two logical chunks: c0, c0 + 1
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * TM * 32 + i * 32 + r;
        const uint4 lo = *reinterpret_cast<const uint4*>(as_ + row * kRowB + ((c0 ^ (row & 7)) << 4));
        const uint4 hi = *reinterpret_cast<const uint4*>(as_ + row * kRowB + (((c0 + 1) ^ (row & 7)) << 4));
        fa[i] = i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int row = wn * TN * 32 + i * 32 + r;
        const uint4 lo = *reinterpret_cast<const uint4*>(bs_ + row * kRowB + ((c0 ^ (row & 7)) << 4));
        const uint4 hi = *reinterpret_cast<const uint4*>(bs_ + row * kRowB + (((c0 + 1) ^ (row & 7)) << 4));
        fb[i] = i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[jn], acc[i][jn], 0, 0, 0, 127, 0, 127);
    }
    if (kt + 1 < nk) store_slice(buf ^ 1);  // buffer buf^1 was last read before the previous barrier
    __syncthreads();
  }

  // epilogue: lane (r, h) owns column r of each 32x32 tile, rows 8*(e>>2) + 4h + (e&3); 32 lanes store 32 consecutive
  // channels of one pixel (32 bytes of codes / 128 bytes of fp32)
  const bool has2 = p.s2 != nullptr;
#pragma unroll
  for (int jn = 0; jn < TN; ++jn) {
    const int col = n0 + wn * TN * 32 + jn * 32 + r;
    if (col >= p.Cout) continue;
    const float sc1 = p.s1[col], sh1 = p.t1[col];
    const float sc2 = has2 ? p.s2[col] : 1.f, sh2 = has2 ? p.t2[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mb = m0 + wm * TM * 32 + i * 32 + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = mb + (e & 3) + 8 * (e >> 2);
        if (m >= p.M) continue;
        float v = apply_act(__builtin_fmaf(acc[i][jn][e], sc1, sh1), p.act1, p.slope1);
        if (p.res) v += e4m3_to_f32(p.res[(long long)m * p.r_cs + p.r_co + col]) * p.r_scale;
        if (has2) v = apply_act(__builtin_fmaf(v, sc2, sh2), p.act2, p.slope2);
        const long long o = (long long)m * p.y_cs + p.y_co + col;
        if (p.out_f32) reinterpret_cast<float*>(p.y)[o] = v;
        else reinterpret_cast<unsigned char*>(p.y)[o] = (unsigned char)quant_e4m3(v, p.y_inv);
      }
    }
  }
}

template <int BM, int BN, bool GENERAL_K>
static int launch_f8(ConvArgsF8 p, hipStream_t stream) {
  constexpr size_t lds = (size_t)2 * (BM + BN) * 128;
  const long long tiles_m = ((long long)p.M + BM - 1) / BM;
  p.tiles_n = (p.Cout + BN - 1) / BN;
  const long long tiles = tiles_m * p.tiles_n;
  if (tiles <= 0 || tiles > 0x7fffffffLL) {
    set_error("conv f8: grid of %lld tiles out of range", tiles);
    return YV4_E_INVALID;
  }
  auto kern = conv_f8_kernel<BM, BN, GENERAL_K>;
  static LdsAttrOnce once;
  if (int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(kern), lds, "conv_f8")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(kF8Threads), lds, stream, p);
  YV4_CHECK_LAUNCH("conv_f8");
  return YV4_OK;
}

static int pick_tile_f8(long long M, int Cout) {
  auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn); };
  if (Cout >= 128 && tiles(128, 128) >= 512) return YV4_F8TILE_128x128;
  if (tiles(128, 64) >= 256) return YV4_F8TILE_128x64;
  return YV4_F8TILE_64x64;
}

// ---- quantize: a 16-bit or fp32 NHWC view -> an e4m3 view, 4 channels per thread ----------------------------------
template <typename T>
__global__ __launch_bounds__(256) void quantize_f8_kernel(const T* __restrict__ x, int x_cs, int x_co,
                                                          unsigned char* __restrict__ y, int y_cs, int y_co, long long P,
                                                          int C4, float inv_s) {
  const long long total = P * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long pix = i / C4;
    const int c = (int)(i - pix * C4) * 4;
    const T* src = x + pix * x_cs + x_co + c;
    unsigned word = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) word |= quant_e4m3((float)src[u], inv_s) << (8 * u);
    *reinterpret_cast<unsigned*>(y + pix * y_cs + y_co + c) = word;
  }
}

// ---- SPP on codes: mp5 / mp9 / mp13 (stride 1, windows clipped at the border) of channels [coff, coff + C) into the
// next three C-channel slots.  Codes compare in sign-magnitude order, so the max is exact (no rounding).  One thread
// per (pixel, 4 channels) walks the 13 x 13 window once.
__device__ __forceinline__ unsigned f8_key(unsigned c) { return (c & 0x80u) ? 0x7Fu - (c & 0x7Fu) : 0x80u + c; }
__device__ __forceinline__ unsigned f8_unkey(unsigned k) { return k >= 0x80u ? k - 0x80u : 0x80u | (0x7Fu - k); }

__global__ __launch_bounds__(256) void spp_f8_kernel(unsigned char* __restrict__ buf, int N, int H, int W, int C4, int cs,
                                                     int co) {
  const long long total = (long long)N * H * W * C4;
  const int C = C4 * 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long pix = i / C4;
    const int c = (int)(i - pix * C4) * 4;
    const int n = (int)(pix / ((long long)H * W));
    const int rm = (int)(pix - (long long)n * H * W);
    const int y = rm / W, x = rm - (rm / W) * W;
    unsigned m5[4] = {0u, 0u, 0u, 0u}, m9[4] = {0u, 0u, 0u, 0u}, m13[4] = {0u, 0u, 0u, 0u};
    for (int dy = -6; dy <= 6; ++dy) {
      const int yy = y + dy;
      if ((unsigned)yy >= (unsigned)H) continue;
      for (int dx = -6; dx <= 6; ++dx) {
        const int xx = x + dx;
        if ((unsigned)xx >= (unsigned)W) continue;
        const unsigned word = *reinterpret_cast<const unsigned*>(buf + (((long long)n * H + yy) * W + xx) * cs + co + c);
        const bool in9 = dy >= -4 && dy <= 4 && dx >= -4 && dx <= 4;
        const bool in5 = dy >= -2 && dy <= 2 && dx >= -2 && dx <= 2;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned k = f8_key((word >> (8 * u)) & 0xFFu);
          m13[u] = max(m13[u], k);
          if (in9) m9[u] = max(m9[u], k);
          if (in5) m5[u] = max(m5[u], k);
        }
      }
    }
    unsigned w5 = 0u, w9 = 0u, w13 = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w5 |= f8_unkey(m5[u]) << (8 * u);
      w9 |= f8_unkey(m9[u]) << (8 * u);
      w13 |= f8_unkey(m13[u]) << (8 * u);
    }
    unsigned char* o = buf + pix * cs + co + c;
    *reinterpret_cast<unsigned*>(o + C) = w5;
    *reinterpret_cast<unsigned*>(o + 2 * C) = w9;
    *reinterpret_cast<unsigned*>(o + 3 * C) = w13;
  }
}

static unsigned grid_for(long long total) {
  long long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace yv4

using namespace yv4;

#define YV4_UNSUPPORTED_IF(cond, ...) \
  do {                                \
    if (cond) {                       \
      set_error(__VA_ARGS__);         \
      return YV4_E_UNSUPPORTED;       \
    }                                 \
  } while (0)

extern "C" int yv4_conv_f8_pick_tile(const yv4_conv_desc* d) {
  if (!d) return YV4_F8TILE_64x64;
  return pick_tile_f8((long long)d->N * d->Ho * d->Wo, d->Cout);
}

extern "C" int yv4_conv_bn_act_fwd_f8(const yv4_conv_desc* d, int out_dtype, const void* x, const void* w,
                                      const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                      const void* residual, float r_scale, float y_inv_scale, void* y, void* stream) {
  YV4_REQUIRE(d && x && w && scale1 && shift1 && y, "conv f8: null argument");
  YV4_REQUIRE(out_dtype == YV4_F8E4M3 || out_dtype == YV4_F32, "conv f8: out_dtype must be YV4_F8E4M3 or YV4_F32");
  YV4_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), "conv f8: scale2/shift2 must come together");
  ConvDescRules rules{16, residual != nullptr};      // (16 channels = one 16-byte chunk of codes)
  rules.any_taps = rules.misaligned_is_unsupported = true;
  if (int rc = check_conv_desc(d, "conv f8", rules)) return rc;
  YV4_UNSUPPORTED_IF(((uintptr_t)x & 15) || ((uintptr_t)w & 15) || (out_dtype == YV4_F32 && ((uintptr_t)y & 3)),
                     "conv f8: x / w must be 16-byte aligned, an fp32 output 4-byte aligned");
  YV4_REQUIRE((long long)d->KH * d->KW * d->Cin < (1LL << 30), "conv f8: K too large");
  ConvArgsF8 a = conv_args_f8(d, out_dtype == YV4_F32 ? 1 : 0, x, w, scale1, shift1, scale2, shift2, residual, r_scale,
                              y_inv_scale, y);
  const bool general = d->Cin % kF8BK != 0;
  const int tile = d->tile ? d->tile : pick_tile_f8(a.M, d->Cout);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (tile) {
    case YV4_F8TILE_128x128: return general ? launch_f8<128, 128, true>(a, s) : launch_f8<128, 128, false>(a, s);
    case YV4_F8TILE_128x64: return general ? launch_f8<128, 64, true>(a, s) : launch_f8<128, 64, false>(a, s);
    case YV4_F8TILE_64x64: return general ? launch_f8<64, 64, true>(a, s) : launch_f8<64, 64, false>(a, s);
    default: break;
  }
  set_error("conv f8: unknown tile id %d", tile);
  return YV4_E_INVALID;
}

extern "C" int yv4_quantize_f8(const void* x, int dtype, int N, int H, int W, int C, int x_cstride, int x_coff, void* y,
                               int y_cstride, int y_coff, float inv_scale, void* stream) {
  YV4_REQUIRE(x && y, "quantize f8: null pointer");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "quantize f8: dtype must be YV4_F32/F16/BF16");
  YV4_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "quantize f8: bad shape");
  YV4_UNSUPPORTED_IF(C % 4 || x_cstride % 4 || x_coff % 4 || y_cstride % 4 || y_coff % 4 || ((uintptr_t)y & 3),
                     "quantize f8: channel counts / offsets must be multiples of 4");
  YV4_REQUIRE(x_coff >= 0 && x_coff + C <= x_cstride && y_coff >= 0 && y_coff + C <= y_cstride,
              "quantize f8: view exceeds its pixel stride");
  const long long P = (long long)N * H * W;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned g = grid_for(P * (C / 4));
  unsigned char* yb = (unsigned char*)y;
  if (dtype == YV4_F32)
    hipLaunchKernelGGL(quantize_f8_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x, x_cstride, x_coff, yb, y_cstride,
                       y_coff, P, C / 4, inv_scale);
  else if (dtype == YV4_BF16)
    hipLaunchKernelGGL(quantize_f8_kernel<__bf16>, dim3(g), dim3(256), 0, s, (const __bf16*)x, x_cstride, x_coff, yb,
                       y_cstride, y_coff, P, C / 4, inv_scale);
  else
    hipLaunchKernelGGL(quantize_f8_kernel<_Float16>, dim3(g), dim3(256), 0, s, (const _Float16*)x, x_cstride, x_coff, yb,
                       y_cstride, y_coff, P, C / 4, inv_scale);
  YV4_CHECK_LAUNCH("quantize_f8");
  return YV4_OK;
}

extern "C" int yv4_spp_pool_fwd_f8(void* buf, int N, int H, int W, int C, int cstride, int coff, void* stream) {
  YV4_REQUIRE(buf, "spp f8: null pointer");
  YV4_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "spp f8: bad shape");
  YV4_UNSUPPORTED_IF(C % 4 || cstride % 4 || coff % 4 || ((uintptr_t)buf & 3),
                     "spp f8: C, cstride and coff must be multiples of 4");
  YV4_REQUIRE(coff >= 0 && coff + 4 * C <= cstride, "spp f8: the 4C-channel concat view exceeds the pixel stride");
  const long long total = (long long)N * H * W * (C / 4);
  hipLaunchKernelGGL(spp_f8_kernel, dim3(grid_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (unsigned char*)buf, N, H, W, C / 4, cstride, coff);
  YV4_CHECK_LAUNCH("spp_f8");
  return YV4_OK;
}
