// Fused implicit-GEMM convolution for gfx950 (MI355X), fp32 in / fp32 accumulate on
// v_mfma_f32_32x32x2_f32 (exact fp32 -- there is no xf32 on CDNA4).
//
// Replaces, for inference, the reference's  Conv2d -> BatchNorm2d(eval) -> Mish
// (mmcv ConvModule as instantiated by mmdet/models/backbones/darknetcsp.py:15-35),
// the Bottleneck residual add (darknetcsp.py:60-64), the CSP-level
// cat -> BN -> act (darknetcsp.py:106-109,149-153,220-229) and the biased head
// conv (mmdet/models/dense_heads/yolocsp_head.py:180-185, 216-220).
//
// GEMM view:  M = N*Ho*Wo output pixels, Ncol = Cout, K = KH*KW*Cin.
//   A[m][k]  = x[n, ho*s-p+kh, wo*s-p+kw, ci]    (NHWC gather, zero outside)
//   B[k][co] = w[co][k]                          (weights stored K-contiguous)
// A workgroup (256 threads = 4 waves) owns a BM x BN output tile; the K loop
// stages BK=32 deep slices of A and B through double-buffered LDS (rows padded to
// 36 floats so the ds_read_b128 fragment reads are bank-conflict free), global
// loads for slice t+1 are in flight while slice t feeds the MFMAs.
// Per MFMA the lane map is  A[i=lane&31][k=lane>>5], B[k=lane>>5][j=lane&31],
// D[row=(reg&3)+8*(reg>>2)+4*(lane>>5)][col=lane&31]; rows are pixels and columns
// are output channels, so every accumulator register stores 2 x 128 contiguous
// bytes of NHWC output.
#include "conv_f32_common.h"
#include "conv_desc.h"
#include "conv_route.h"

namespace yv4 {

// (ConvArgs, out_row, lds_dma16, make_rsrc: conv_f32_common.h -- shared with conv3x3_wide_f32.hip)

template <int BM, int BN, int WAVES_M, int WAVES_N, bool UNIFORM_TAP>
__global__ __launch_bounds__(kThreads, 2) void conv_mfma_f32_kernel(ConvArgs p) {
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  constexpr int TM = BM / WAVES_M / 32;  // 32x32 MFMA tiles per wave along M
  constexpr int TN = BN / WAVES_N / 32;
  constexpr int PA = BM / 32;            // staging passes (32 rows per pass)
  constexpr int PB = BN / 32;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                   // [2][BM][kLDK]
  float* Bs = smem + 2 * BM * kLDK;   // [2][BN][kLDK]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int r = lane & 31;
  const int h = lane >> 5;

  const int tile_n = blockIdx.x % p.tiles_n;
  const int tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;

  // ---- staging coordinates: thread -> (row = tid/8 + 32*pass, 16-byte chunk cc) ----
  const int cc = tid & 7;
  const int srow = tid >> 3;

  const float* a_ptr[PA];  // &x[n, ho*s-p, wo*s-p, x_co + cc*4]  (may be out of range)
  int a_hi0[PA], a_wi0[PA];
#pragma unroll
  for (int q = 0; q < PA; ++q) {
    const int m = m0 + srow + 32 * q;
    if (m < p.M) {
      const int hw = p.Ho * p.Wo;
      const int n = m / hw;
      const int rem = m - n * hw;
      const int ho = rem / p.Wo;
      const int wo = rem - ho * p.Wo;
      const int hi0 = ho * p.stride - p.pad;
      const int wi0 = wo * p.stride - p.pad;
      a_hi0[q] = hi0;
      a_wi0[q] = wi0;
      a_ptr[q] = p.x + ((int64_t)(n * p.H + hi0) * p.W + wi0) * p.x_cs + p.x_co + cc * 4;
    } else {
      a_hi0[q] = -(1 << 28);  // never in range
      a_wi0[q] = -(1 << 28);
      a_ptr[q] = p.x;
    }
  }
  const float* b_ptr[PB];
  bool b_ok[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    const int co = n0 + srow + 32 * q;
    b_ok[q] = co < p.Cout;
    b_ptr[q] = p.w + (int64_t)(b_ok[q] ? co : 0) * p.Kw + cc * 4;
  }

  float4 ra[PA], rb[PB];

  auto load_slice = [&](int kt) {
    const int kbase = kt * kBK;
    if (UNIFORM_TAP) {
      // Cin % 32 == 0: the whole slice lies in one (kh,kw) tap.
      const int tap = kbase / p.Cin;
      const int c0 = kbase - tap * p.Cin;
      const int kh = tap / p.KW;
      const int kw = tap - kh * p.KW;
      const int64_t step = ((int64_t)kh * p.W + kw) * p.x_cs + c0;
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int hi = a_hi0[q] + kh;
        const int wi = a_wi0[q] + kw;
        const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        ra[q] = ok ? *reinterpret_cast<const float4*>(a_ptr[q] + step)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        rb[q] = b_ok[q] ? *reinterpret_cast<const float4*>(b_ptr[q] + kbase)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      // generic: Cin % 4 == 0, so a 4-float chunk never straddles a tap.
      const int k0 = kbase + cc * 4;
      const bool kok = k0 < p.K;
      const int tap = k0 / p.Cin;
      const int c0 = k0 - tap * p.Cin;
      const int kh = tap / p.KW;
      const int kw = tap - kh * p.KW;
      const int64_t step = ((int64_t)kh * p.W + kw) * p.x_cs + c0 - cc * 4;
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int hi = a_hi0[q] + kh;
        const int wi = a_wi0[q] + kw;
        const bool ok = kok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        ra[q] = ok ? *reinterpret_cast<const float4*>(a_ptr[q] + step)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        rb[q] = (b_ok[q] && kok) ? *reinterpret_cast<const float4*>(b_ptr[q] + kbase)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };

  auto store_slice = [&](int buf) {
    float* as = As + buf * BM * kLDK;
    float* bs = Bs + buf * BN * kLDK;
#pragma unroll
    for (int q = 0; q < PA; ++q)
      *reinterpret_cast<float4*>(as + (srow + 32 * q) * kLDK + cc * 4) = ra[q];
#pragma unroll
    for (int q = 0; q < PB; ++q)
      *reinterpret_cast<float4*>(bs + (srow + 32 * q) * kLDK + cc * 4) = rb[q];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = (p.K + kBK - 1) / kBK;

  load_slice(0);
  store_slice(0);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_slice(kt + 1);

    const float* as = As + buf * BM * kLDK + (wm * TM * 32 + r) * kLDK + 4 * h;
    const float* bs = Bs + buf * BN * kLDK + (wn * TN * 32 + r) * kLDK + 4 * h;
#pragma unroll
    for (int j = 0; j < kBK / 8; ++j) {
      float4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i] = *reinterpret_cast<const float4*>(as + i * 32 * kLDK + 8 * j);
#pragma unroll
      for (int i = 0; i < TN; ++i)
        fb[i] = *reinterpret_cast<const float4*>(bs + i * 32 * kLDK + 8 * j);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
          acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[jn].x, acc[i][jn], 0, 0, 0);
          acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[jn].y, acc[i][jn], 0, 0, 0);
          acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[jn].z, acc[i][jn], 0, 0, 0);
          acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[jn].w, acc[i][jn], 0, 0, 0);
        }
    }

    if (kt + 1 < nk) store_slice(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: affine1 -> act1 -> (+residual) -> [affine2 -> act2] -> NHWC store ----
  const bool has2 = p.s2 != nullptr;
#pragma unroll
  for (int jn = 0; jn < TN; ++jn) {
    const int co = n0 + wn * TN * 32 + jn * 32 + r;
    const bool cok = co < p.Cout;
    const float s1 = cok ? p.s1[co] : 0.f;
    const float t1 = cok ? p.t1[co] : 0.f;
    const float s2 = (cok && has2) ? p.s2[co] : 1.f;
    const float t2 = (cok && has2) ? p.t2[co] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (cok && m < p.M) {
          float v = acc[i][jn][e] * s1 + t1;
          v = apply_act(v, p.act1, p.slope1);
          if (p.res) v += p.res[(int64_t)m * p.r_cs + p.r_co + co];
          if (has2) v = apply_act(v * s2 + t2, p.act2, p.slope2);
          p.y[(int64_t)m * p.y_cs + p.y_co + co] = v;
        }
      }
    }
  }
}


// Epilogue of one 32x32 accumulator tile through a wave-private LDS patch: the MFMA result has
// the output channel on the lane and 16 pixels in registers, which stores as 16 dword
// instructions touching 2 x 128 B each; transposed through LDS every lane owns 4 consecutive
// channels of one pixel, so the tile leaves (and the residual arrives) in 4 dwordx4
// instructions per lane and the per-channel scale/shift become vector loads.
// `vec_ok` (uniform): all views are 16-byte aligned per pixel (false for the 255-channel heads).
// the activation of a lane's 4 values behind ONE uniform branch on the activation id (apply_act() per element left
// a scalar compare-and-branch chain per element: the compiler does not unswitch the unrolled loop)
__device__ __forceinline__ void act_row4(float4& v, int act, float slope) {
  switch (act) {
    case YV4_ACT_MISH:
      v.x = apply_act(v.x, YV4_ACT_MISH, 0.f); v.y = apply_act(v.y, YV4_ACT_MISH, 0.f);
      v.z = apply_act(v.z, YV4_ACT_MISH, 0.f); v.w = apply_act(v.w, YV4_ACT_MISH, 0.f);
      break;
    case YV4_ACT_LEAKY:
      v.x = v.x >= 0.f ? v.x : v.x * slope; v.y = v.y >= 0.f ? v.y : v.y * slope;
      v.z = v.z >= 0.f ? v.z : v.z * slope; v.w = v.w >= 0.f ? v.w : v.w * slope;
      break;
    case YV4_ACT_SWISH:
      v.x = apply_act(v.x, YV4_ACT_SWISH, 0.f); v.y = apply_act(v.y, YV4_ACT_SWISH, 0.f);
      v.z = apply_act(v.z, YV4_ACT_SWISH, 0.f); v.w = apply_act(v.w, YV4_ACT_SWISH, 0.f);
      break;
    default:
      break;
  }
}

__device__ __forceinline__ void epilogue_tile(const ConvArgs& p, const f32x16& acc, float* ep, int lane, int m_base,
                                              int co_base, bool vec_ok, bool has2) {
  const int r = lane & 31, h = lane >> 5;
  constexpr int kPitch = 36;
#pragma unroll
  for (int e = 0; e < 16; ++e) ep[((e & 3) + 8 * (e >> 2) + 4 * h) * kPitch + r] = acc[e];
  const int c4 = (lane & 7) * 4;
  const int co = co_base + c4;
  if (p.ksplit > 1) {                       // split-K partial: raw accumulators, dense [M][ws_cs] slab (ws_cs % 4 == 0)
    if (co < p.ws_cs) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = (lane >> 3) + 8 * k;
        const int m = m_base + row;
        if (m < p.M)
          *reinterpret_cast<float4*>(p.y + (int64_t)m * p.ws_cs + co) = *reinterpret_cast<const float4*>(ep + row * kPitch + c4);
      }
    }
    return;
  }
  if (vec_ok && co + 3 < p.Cout) {
    const float4 s1 = *reinterpret_cast<const float4*>(p.s1 + co);
    const float4 t1 = *reinterpret_cast<const float4*>(p.t1 + co);
    float4 s2 = make_float4(1.f, 1.f, 1.f, 1.f), t2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has2) {
      s2 = *reinterpret_cast<const float4*>(p.s2 + co);
      t2 = *reinterpret_cast<const float4*>(p.t2 + co);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = (lane >> 3) + 8 * k;
      const int m = m_base + row;
      const float4 a = *reinterpret_cast<const float4*>(ep + row * kPitch + c4);
      if (m < p.M) {
        float4 v = make_float4(a.x * s1.x + t1.x, a.y * s1.y + t1.y, a.z * s1.z + t1.z, a.w * s1.w + t1.w);
        act_row4(v, p.act1, p.slope1);
        if (p.res) {
          const float4 rr = *reinterpret_cast<const float4*>(p.res + (int64_t)m * p.r_cs + p.r_co + co);
          v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
        }
        if (has2) {
          v = make_float4(v.x * s2.x + t2.x, v.y * s2.y + t2.y, v.z * s2.z + t2.z, v.w * s2.w + t2.w);
          act_row4(v, p.act2, p.slope2);
        }
        *reinterpret_cast<float4*>(p.y + out_row(p, m) * p.y_cs + p.y_co + co) = v;
      }
    }
  } else {
    // rows that are not 16-byte aligned (the 255-channel pred maps) or a ragged column tile: lane (r, h) takes channel
    // co_base + r of the rows 2k + h, so a store instruction writes two runs of 32 consecutive floats (coalesced
    // whatever the row's alignment).  Same arithmetic, element for element, as the vector path.
    const int c = co_base + r;
    if (c < p.Cout) {
      const float sc1 = p.s1[c], sh1 = p.t1[c];
      const float sc2 = has2 ? p.s2[c] : 1.f, sh2 = has2 ? p.t2[c] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int row = 2 * k + h;
        const int m = m_base + row;
        if (m >= p.M) continue;
        float v = ep[row * kPitch + r] * sc1 + sh1;
        v = apply_act(v, p.act1, p.slope1);
        if (p.res) v += p.res[(int64_t)m * p.r_cs + p.r_co + c];
        if (has2) v = apply_act(v * sc2 + sh2, p.act2, p.slope2);
        p.y[out_row(p, m) * p.y_cs + p.y_co + c] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// Fast path (Cin % 32 == 0): LDS-DMA staging.  The next K slice goes global -> LDS directly
// (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction, no VGPR round trip and no
// ds_write: in the register-staged kernel above the VGPR->LDS store path is the largest
// non-MFMA cost, ~12 % in an ablation).
// An LDS-DMA instruction writes lane l at base + 16*l, so the LDS image is unpadded
// [row][32 floats] with 128-byte rows; ds_read_b128 conflicts are avoided by an XOR
// swizzle of the 16-byte chunk index with (row>>1)&7, applied on the SOURCE side (which
// global chunk a lane fetches) and on the read side.  Out-of-range buffer offsets deliver
// zeros, which implements conv padding, the M tail and the Cout tail.
// ---------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, int NBUF>
__global__ __launch_bounds__(kThreads, 2) void conv_mfma_f32_dma_kernel(ConvArgs p, unsigned x_bytes, unsigned w_bytes) {
  static_assert(NBUF >= 2 && NBUF <= 4, "ring of 2..4 slices");
  constexpr int D = NBUF - 1;           // prefetch distance in K slices
  constexpr int kDmaPerSlice = BM / 32 + BN / 32;   // LDS-DMA instructions per wave per slice
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  constexpr int TM = BM / WAVES_M / 32;
  constexpr int TN = BN / WAVES_N / 32;
  constexpr int PA = BM / 32;   // DMA passes over A: 32 rows per pass (8 rows per wave-instruction)
  constexpr int PB = BN / 32;
  constexpr int kRow = kBK;     // floats per LDS row (128 B, unpadded)
  typedef __attribute__((address_space(3))) void* lds_ptr_t;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                      // [NBUF][BM][32]
  float* Bs = smem + NBUF * BM * kRow;   // [NBUF][BN][32]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int r = lane & 31;
  const int h = lane >> 5;

  const unsigned nwg = gridDim.x;
  const unsigned bid = blockIdx.x;
  const unsigned xcd = bid & 7u, q8 = nwg >> 3, rem8 = nwg & 7u;
  const unsigned tile_s = (xcd < rem8 ? xcd * (q8 + 1) : rem8 * (q8 + 1) + (xcd - rem8) * q8) + (bid >> 3);
  const int ksplit = p.ksplit > 1 ? p.ksplit : 1;
  const unsigned tile = tile_s / (unsigned)ksplit;          // the splits of one tile are neighbours (same L2)
  const int split = (int)(tile_s - tile * (unsigned)ksplit);
  const int tile_n = tile % p.tiles_n;
  const int tile_m = tile / p.tiles_n;
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  if (ksplit > 1) p.y = p.ws + (size_t)split * p.M * p.ws_cs;

  const u32x4_t rsA = make_rsrc(p.x, x_bytes);
  const u32x4_t rsB = make_rsrc(p.w, w_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem;   // LDS byte address of the carve

  // staging: this lane fills LDS row (32*q + 8*wave + lane/8), physical chunk lane%8
  const int srow = 8 * wave + (lane >> 3);
  const int pc = lane & 7;
  unsigned a_off[PA];
  unsigned long long a_mask[PA];
#pragma unroll
  for (int q = 0; q < PA; ++q) {
    const int row = srow + 32 * q;
    const int lc = pc ^ ((row >> 1) & 7);    // logical chunk this lane must fetch
    const int m = m0 + row;
    unsigned long long mk = 0ull;
    unsigned off = 0u;
    if (m < p.M) {
      const int hw = p.Ho * p.Wo;
      const int n = fd_div(m, p.fd_hw);
      const int rm = m - n * hw;
      const int ho = fd_div(rm, p.fd_wo);
      const int wo = rm - ho * p.Wo;
      const int hi0 = ho * p.stride - p.pad;
      const int wi0 = wo * p.stride - p.pad;
      off = (unsigned)((((int64_t)(n * p.H + hi0) * p.W + wi0) * p.x_cs + p.x_co + lc * 4) * 4);
      mk = tap_mask(hi0, wi0, p.KH, p.KW, p.H, p.W);
    }
    a_off[q] = off;
    a_mask[q] = mk;
  }
  unsigned b_off[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    const int row = srow + 32 * q;
    const int lc = pc ^ ((row >> 1) & 7);
    const int co = n0 + row;
    b_off[q] = co < p.Cout ? (unsigned)(((int64_t)co * p.Kw + lc * 4) * 4) : kOOB;
  }

  // K is walked channel-chunk-major: the KH*KW taps of one 32-channel chunk in consecutive slices, then the next
  // chunk.  A tap re-reads the 128-B lines its neighbours read one (kw) or KW (kh) slices ago, which are still in the
  // XCD's L2; with the taps outermost each line came back Cin/32 slices later, after every concurrent tile had streamed
  // its whole window through the 4 MB L2 (profiles/r01_layer_traffic.md).  The weights stay [Cout][kh][kw][cin].
  const int ntaps = p.KH * p.KW;
  int s_tap = 0, s_c0 = 0, s_kh = 0, s_kw = 0;
  unsigned s_kb = 0;
  const int slice0 = ksplit > 1 ? split * p.ks_slices : 0;      // first K slice of this workgroup
  if (slice0) {
    const int chunk = fd_div(slice0, p.fd_taps);
    s_tap = slice0 - chunk * ntaps;
    s_c0 = chunk * kBK;
    s_kh = fd_div(s_tap, p.fd_kw);
    s_kw = s_tap - s_kh * p.KW;
    s_kb = (unsigned)((s_tap * p.Cin + s_c0) * 4);
  }

  // The kDmaPerSlice LDS-DMA pieces of a slice: the prologue issues them in one block (YV4_V3_DMA); in the K loop they
  // go out between the MFMAs of the slice being computed, a quarter per 8-deep K step (YV4_V3_DMA_PIECES inside
  // YV4_V3_COMPUTE) -- a piece costs 60-180 cycles of issue (MI355X_MICROARCH.md) during which the wave cannot feed the
  // matrix pipe unless its own MFMAs are already in flight (the weight-stationary kernel's stamps).
  unsigned d_step = 0u, d_la = 0u, d_lb = 0u;
#define YV4_V3_DMA_SETUP(BUF)                                                       \
  {                                                                                 \
    d_step = (unsigned)((((int64_t)s_kh * p.W + s_kw) * p.x_cs + s_c0) * 4);        \
    d_la = lds_base + (unsigned)(((BUF) * BM + 8 * wave) * kRow * 4);               \
    d_lb = lds_base + (unsigned)((NBUF * BM + (BUF) * BN + 8 * wave) * kRow * 4);   \
  }
#define YV4_V3_DMA_PIECE(Q)                                                         \
  {                                                                                 \
    if ((Q) < PA) {                                                                 \
      const int qa_ = (Q) < PA ? (Q) : 0;                                           \
      const bool ok = (a_mask[qa_] >> s_tap) & 1ull;                                \
      lds_dma16(rsA, d_la + 32 * qa_ * kRow * 4, ok ? a_off[qa_] + d_step : kOOB, 0u); \
    } else {                                                                        \
      const int qb_ = (Q) >= PA ? (Q) - PA : 0;                                     \
      lds_dma16(rsB, d_lb + 32 * qb_ * kRow * 4, b_off[qb_], s_kb);                  \
    }                                                                               \
  }
#define YV4_V3_DMA_ADVANCE()                                                        \
  {                                                                                 \
    s_tap += 1;                                                                     \
    s_kw += 1;                                                                      \
    const int wrap_w = s_kw == p.KW ? 1 : 0;                                        \
    s_kw = wrap_w ? 0 : s_kw;                                                       \
    s_kh += wrap_w;                                                                 \
    const int wrap_t = s_tap == ntaps ? 1 : 0;                                      \
    s_tap = wrap_t ? 0 : s_tap;                                                     \
    s_kh = wrap_t ? 0 : s_kh;                                                       \
    s_c0 += wrap_t ? kBK : 0;                                                       \
    s_kb = (unsigned)((s_tap * p.Cin + s_c0) * 4);                                  \
  }
#define YV4_V3_DMA(BUF)                                                             \
  {                                                                                 \
    YV4_V3_DMA_SETUP(BUF);                                                          \
    _Pragma("unroll") for (int q = 0; q < kDmaPerSlice; ++q) YV4_V3_DMA_PIECE(q);   \
    YV4_V3_DMA_ADVANCE();                                                           \
  }
  constexpr bool kPiecewise = TM * TN >= 2;   // (the 64 x 64 tile has ONE MFMA quad per K step to issue under: no gain, -2 %)
#define YV4_V3_DMA_PIECES(J)                                                        \
  if (kPiecewise && dma_on) {                                                       \
    __builtin_amdgcn_sched_barrier(0);                                              \
    _Pragma("unroll") for (int q = (J) * kDmaPerSlice / 4; q < ((J) + 1) * kDmaPerSlice / 4; ++q) YV4_V3_DMA_PIECE(q); \
    __builtin_amdgcn_sched_barrier(0);                                              \
  }

  // fragment read addresses: row*128 B + ((chunk ^ swz) << 4); chunk = 2j + h
  unsigned a_rd[TM], b_rd[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = wm * TM * 32 + i * 32 + r;
    a_rd[i] = (unsigned)(row * kRow * 4 + ((((row >> 1) & 7) ^ h) << 4));
  }
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int row = wn * TN * 32 + i * 32 + r;
    b_rd[i] = (unsigned)(row * kRow * 4 + ((((row >> 1) & 7) ^ h) << 4));
  }

#define YV4_V3_COMPUTE(BUF)                                                         \
  {                                                                                 \
    const char* as_ = reinterpret_cast<const char*>(As + (BUF) * BM * kRow);        \
    const char* bs_ = reinterpret_cast<const char*>(Bs + (BUF) * BN * kRow);        \
    _Pragma("unroll") for (int j = 0; j < kBK / 8; ++j) {                           \
      float4 fa[TM], fb[TN];                                                        \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                \
          fa[i] = *reinterpret_cast<const float4*>(as_ + (a_rd[i] ^ (unsigned)(j << 5))); \
      _Pragma("unroll") for (int i = 0; i < TN; ++i)                                \
          fb[i] = *reinterpret_cast<const float4*>(bs_ + (b_rd[i] ^ (unsigned)(j << 5))); \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                \
        _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                         \
          f32x16& ac_ = (j & 1) ? acc2[i][jn] : acc[i][jn];                         \
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[jn].x, ac_, 0, 0, 0); \
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[jn].y, ac_, 0, 0, 0); \
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[jn].z, ac_, 0, 0, 0); \
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[jn].w, ac_, 0, 0, 0); \
          if (i == 0 && jn == 0) YV4_V3_DMA_PIECES(j)                               \
        }                                                                           \
    }                                                                               \
  }

  // Two accumulator sets, alternating every 8 K values: each fp32 chain is half as long (the
  // sequential K = 4608 chain of a single set measured 1.7x the CPU reference's rounding error
  // against float64 at full depth, tests/test_gpu_fullsize.py); summed once before the epilogue.
  f32x16 acc[TM][TN], acc2[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; acc2[i][j][e] = 0.f; }

  // wait until at most `newer` later slices of this wave's DMAs are still in flight
#define YV4_V3_WAIT(NEWER)                                                          \
  {                                                                                 \
    if ((NEWER) >= 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * kDmaPerSlice) : "memory"); \
    else if ((NEWER) == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * kDmaPerSlice) : "memory"); \
    else if ((NEWER) == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(1 * kDmaPerSlice) : "memory"); \
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                 \
  }

  const int nk_all = p.K / kBK;
  const int nk = ksplit > 1 ? (nk_all - slice0 < p.ks_slices ? nk_all - slice0 : p.ks_slices) : nk_all;
  int issued = 0;        // slices whose DMA has been issued
  int wbuf = 0;          // ring slot the next DMA goes to
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (d < nk) {
      YV4_V3_DMA(wbuf);
      ++issued;
      wbuf = wbuf + 1 == NBUF ? 0 : wbuf + 1;
    }
  }
  YV4_V3_WAIT(issued - 1);             // slice 0 landed (this wave's part) ...
  __builtin_amdgcn_s_barrier();        // ... and everybody else's

  int rbuf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    const bool dma_on = issued < nk;   // slot wbuf was last read before the previous barrier
    if (dma_on) {
      YV4_V3_DMA_SETUP(wbuf);
      if (!kPiecewise) {
#pragma unroll
        for (int q = 0; q < kDmaPerSlice; ++q) YV4_V3_DMA_PIECE(q);
      }
    }
    __builtin_amdgcn_s_setprio(1);   // keep the MFMA cluster ahead of the other resident waves' setup code
    YV4_V3_COMPUTE(rbuf);
    __builtin_amdgcn_s_setprio(0);
    if (dma_on) {
      YV4_V3_DMA_ADVANCE();
      ++issued;
      wbuf = wbuf + 1 == NBUF ? 0 : wbuf + 1;
    }
    rbuf = rbuf + 1 == NBUF ? 0 : rbuf + 1;
    if (kt + 1 < nk) {
      // fragment reads of this slot returned (lgkmcnt(0)), slice kt+1 landed (counted
      // vmcnt: slices kt+2.. may stay in flight), then the workgroup moves on.
      YV4_V3_WAIT(issued - (kt + 2));
      __builtin_amdgcn_s_barrier();
    }
  }
#undef YV4_V3_WAIT
#undef YV4_V3_DMA
#undef YV4_V3_DMA_SETUP
#undef YV4_V3_DMA_PIECE
#undef YV4_V3_DMA_PIECES
#undef YV4_V3_DMA_ADVANCE
#undef YV4_V3_COMPUTE

  // ---- epilogue: transposed through a wave-private LDS patch (the K-loop buffers are free
  // once every wave has issued its last fragment reads: one more barrier) ----
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] += acc2[i][j][e];
  // BatchNorm statistics of the tile while it is in registers (identity-epilogue training convs; see the same
  // block in conv_mfma_h16.hip)
  if (p.stats) {
    const StatRep rep = stat_rep(p.stats, (unsigned)(tile_m), p.Cout);
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      float su = 0.f, sq = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int mb = m0 + wm * TM * 32 + i * 32 + 4 * h;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float v = acc[i][jn][e];
          if (mb + (e & 3) + 8 * (e >> 2) < p.M) { su += v; sq += v * v; }
        }
      }
      su += __shfl_xor(su, 32);
      sq += __shfl_xor(sq, 32);
      const int col = n0 + wn * TN * 32 + jn * 32 + r;
      if (h == 0 && col < p.Cout) {
        stat_add(rep, col, su);
        stat_add(rep, p.Cout + col, sq);
      }
    }
  }
  const bool has2 = p.s2 != nullptr;
  const bool vec_ok = ((p.y_cs | p.y_co) & 3) == 0 && (p.res == nullptr || ((p.r_cs | p.r_co) & 3) == 0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  float* ep = smem + wave * (32 * 36);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jn = 0; jn < TN; ++jn)
      epilogue_tile(p, acc[i][jn], ep, lane, m0 + wm * TM * 32 + i * 32, n0 + wn * TN * 32 + jn * 32, vec_ok, has2);
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int NBUF>
static int launch_conv_dma(const ConvArgs& a, hipStream_t stream) {
  constexpr size_t lds = (size_t)NBUF * (BM + BN) * kBK * sizeof(float);
  ConvArgs p = a;
  const int tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.Cout + BN - 1) / BN;
  p.fd_hw = make_fastdiv((unsigned)(p.Ho * p.Wo));
  p.fd_wo = make_fastdiv((unsigned)p.Wo);
  p.fd_taps = make_fastdiv((unsigned)(p.KH * p.KW));
  p.fd_kw = make_fastdiv((unsigned)p.KW);
  const long long tiles = (long long)tiles_m * p.tiles_n * (p.ksplit > 1 ? p.ksplit : 1);
  if (tiles <= 0 || tiles > 0x7fffffffLL) {
    set_error("conv: grid of %lld tiles out of range", tiles);
    return YV4_E_INVALID;
  }
  const long long xb = x_bytes(p), wb = w_bytes(p);
  if (!dma_addressable(p)) {
    set_error("conv dma: tensors of 4 GiB or more are not addressable through a buffer descriptor");
    return YV4_E_UNSUPPORTED;
  }
  auto kern = conv_mfma_f32_dma_kernel<BM, BN, WAVES_M, WAVES_N, NBUF>;
  static LdsAttrOnce once;
  if (int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(kern), lds, "conv_mfma_f32_dma")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(kThreads), lds, stream, p, (unsigned)xb, (unsigned)wb);
  YV4_CHECK_LAUNCH("conv_mfma_f32_dma");
  return YV4_OK;
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_conv(const ConvArgs& a, bool uniform_tap, hipStream_t stream) {
  constexpr size_t lds = (size_t)2 * (BM + BN) * kLDK * sizeof(float);
  ConvArgs p = a;
  const int tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.Cout + BN - 1) / BN;
  p.fd_hw = make_fastdiv((unsigned)(p.Ho * p.Wo));
  p.fd_wo = make_fastdiv((unsigned)p.Wo);
  const long long tiles = (long long)tiles_m * p.tiles_n;
  if (tiles <= 0 || tiles > 0x7fffffffLL) {
    set_error("conv: grid of %lld tiles out of range", tiles);
    return YV4_E_INVALID;
  }
  auto kern_u = conv_mfma_f32_kernel<BM, BN, WAVES_M, WAVES_N, true>;
  auto kern_g = conv_mfma_f32_kernel<BM, BN, WAVES_M, WAVES_N, false>;
  static LdsAttrOnce once_u, once_g;
  if (int rc = ensure_dyn_lds(once_u, reinterpret_cast<const void*>(kern_u), lds, "conv_mfma_f32")) return rc;
  if (int rc = ensure_dyn_lds(once_g, reinterpret_cast<const void*>(kern_g), lds, "conv_mfma_f32")) return rc;
  if (uniform_tap)
    hipLaunchKernelGGL(kern_u, dim3((unsigned)tiles), dim3(kThreads), lds, stream, p);
  else
    hipLaunchKernelGGL(kern_g, dim3((unsigned)tiles), dim3(kThreads), lds, stream, p);
  YV4_CHECK_LAUNCH("conv_mfma_f32");
  return YV4_OK;
}

static int pick_tile(long long M, int Cout, bool fast_ok, long long K = 0) {
  // Static choice for callers that do not autotune (training; Plan.autotune re-decides per layer on the box it runs
  // on).  From profiles/r01_conv_shapes.txt (batch 32 YOLOv4-L shapes): deep reductions with several rounds of
  // 128x128 tiles gain 5-9 % on the big tile, the remaining K >= 576 layers and the wide 1x1 layers 3-7 % on
  // 128x64; everything else stays on 64x64 (5 workgroups per CU).
  if (fast_ok) {
    auto ntiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn); };
    if (K >= 576 && Cout >= 128 && ntiles(128, 128) >= 700) return YV4_TILE_DMA_128x128;
    if (Cout >= 64 && (K >= 288 || Cout >= 256) && ntiles(128, 64) >= 512) return YV4_TILE_DMA_128x64;
    return YV4_TILE_DMA_64x64;
  }
  // 256 CUs x 2 resident workgroups.  Prefer the biggest tile that still gives the
  // chip >= 2 full rounds of workgroups; small maps (19x19) fall to smaller tiles.
  auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn); };
  if (Cout > 64) {
    if (tiles(128, 128) >= 1024) return YV4_TILE_128x128;
    if (tiles(128, 64) >= 1024 || Cout <= 64) return YV4_TILE_128x64;
    if (tiles(64, 128) >= 768) return YV4_TILE_64x128;
    return YV4_TILE_64x64;
  }
  if (Cout > 32) return tiles(128, 64) >= 1024 ? YV4_TILE_128x64 : YV4_TILE_64x64;
  return YV4_TILE_64x64;  // Cout <= 32: half of the columns idle; stem / tiny models only
}

// the pointwise layers in the kernel's domain that give each persistent wave at least YV4_WS_MINSTRIPS strips
static bool prefer_ws_f32(const ConvArgs& a) {
  static const int mode = YV4_ENV_INT("YV4_WS", 1);
  static const int min_strips = YV4_ENV_INT("YV4_WS_MINSTRIPS", 2);
  if (!mode || !conv1x1_ws_f32_applies(a)) return false;
  // strips per persistent wave: the 256 workgroups are dealt over the column slabs, 8 waves each (with the DMA pieces
  // issued under the MFMAs the kernel beats the 128x64 tile on 256 -> 256 @38 too: 62 against 67 us, tools/ab_wsf.sh)
  const int bn = wsf_slab_cols(a);
  const long long ncol = (a.Cout + bn - 1) / bn;
  return (((long long)a.M + 31) / 32) * ncol >= (long long)min_strips * 2048;
}

// The wide-tile fp32 3x3 kernel takes the layers in its domain with >= 64 input channels and at least YV4_W3F_MINOUT
// outputs per CU when one of its tile shapes fills the rounds to within YV4_W3F_MAXWASTE percent (YV4_W3F=0: off).
static int prefer_w3_f32(const ConvArgs& a) {      // the shape index, or -1
  static const int mode = YV4_ENV_INT("YV4_W3F", 1);
  static const int waste = YV4_ENV_INT("YV4_W3F_MAXWASTE", 25);
  static const int min_out = YV4_ENV_INT("YV4_W3F_MINOUT", 32768);
  if (!mode || !conv3x3_wide_f32_applies(a) || a.Cin < 64) return -1;
  double eff = 0.0;
  const int shape = conv3x3_wide_f32_pick(a, &eff);
  return shape >= 0 && fills_rounds(a.M, a.Cout, min_out, waste, eff) ? shape : -1;
}

// The general wide-tile fp32 kernel takes the stride-2 3x3 layers with >= YV4_WGF_S2CIN input channels and the 1x1
// layers with >= YV4_WGF_P1CIN, under the same fill rule (YV4_WGF=0: off).  Measured per layer at batch 32 x 608 (round 4,
// profiles/r04_layers_wide_f32.md): stride-2 3x3 with Cin >= 128 gain 4 - 32 %, 64->128@304 and the 256-channel 1x1
// layers lose 2 - 4 % against the DMA tiles, the 512 / 1024-channel 1x1 layers gain 1 - 3 %.
static int prefer_wide_f32(const ConvArgs& a) {    // the shape index, or -1
  static const int mode = YV4_ENV_INT("YV4_WGF", 1);
  static const int waste = YV4_ENV_INT("YV4_WGF_MAXWASTE", 25);
  static const int min_out = YV4_ENV_INT("YV4_WGF_MINOUT", 32768);
  static const int s2cin = YV4_ENV_INT("YV4_WGF_S2CIN", 128);
  static const int p1cin = YV4_ENV_INT("YV4_WGF_P1CIN", 512);
  if (!mode || !conv_wide_f32_applies(a)) return -1;
  const bool s2 = a.KH == 3 && a.KW == 3 && a.stride == 2 && a.Cin >= s2cin;
  const bool p1 = a.KH == 1 && a.KW == 1 && a.stride == 1 && a.Cin >= p1cin;
  if (!s2 && !p1) return -1;
  double eff = 0.0;
  const int shape = conv_wide_f32_pick(a, &eff);
  return shape >= 0 && fills_rounds(a.M, a.Cout, min_out, waste, eff) ? shape : -1;
}

static bool fast_ok(const ConvArgs& a) { return a.Cin % kBK == 0 && dma_addressable(a); }

// What the AUTO path launches: the family as its tile id and, for the two wide families, the shape index (else -1).
// conv_f32_impl launches it and yv4_conv_pick_tile reports it: a plan, the benchmark's output check and the tests
// read the latter to learn the former.
static TileId auto_route(const ConvArgs& a) {
  const bool fast = fast_ok(a);
  if (fast) {
    const int w3 = prefer_w3_f32(a);
    if (w3 >= 0) return {YV4_TILE_W3x3, w3};
    if (prefer_ws_f32(a)) return {YV4_TILE_WS_1x1, -1};
    const int wg = prefer_wide_f32(a);
    if (wg >= 0) return {YV4_TILE_WIDE, wg};
  }
  if (stem_ok(a)) return {YV4_TILE_STEM, -1};
  return {pick_tile(a.M, a.Cout, fast, a.K), -1};
}

}  // namespace yv4

using namespace yv4;

extern "C" double yv4_conv_flops(const yv4_conv_desc* d) {
  if (!d) return 0.0;
  return 2.0 * (double)d->N * d->Ho * d->Wo * d->Cout * (double)d->KH * d->KW * d->Cin;
}

// (a residual or a second affine, unknown here, keeps the tile kernels)
extern "C" int yv4_conv_pick_tile(const yv4_conv_desc* d) {
  if (!d) return YV4_TILE_AUTO;
  const TileId r = auto_route(conv_args(d));
  if (r.tile == YV4_TILE_W3x3) return YV4_TILE_W3x3_SHAPE(r.shape);   // the pinned form: a plan can copy it (see include/yv4.h)
  if (r.tile == YV4_TILE_WIDE) return YV4_TILE_WIDE_SHAPE(r.shape);
  return r.tile;
}

// stats != null: identity-epilogue conv that also accumulates the BatchNorm sums of its output; *stats_done tells
// the caller whether the selected kernel did (the LDS-DMA kernels do; the generic and stem kernels do not)
static int conv_f32_impl(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1, const float* shift1,
                         const float* scale2, const float* shift2, const float* residual, float* y, double* stats,
                         bool* stats_done, void* stream) {
  YV4_REQUIRE(d && x && w && scale1 && shift1 && y, "conv: null argument");
  YV4_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), "conv: scale2/shift2 must come together");
  if (int rc = check_conv_desc(d, "conv", {4, residual != nullptr})) return rc;
  YV4_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "conv: x / w must be 16-byte aligned");

  ConvArgs a = conv_args(d, x, w, scale1, shift1, scale2, shift2, residual, y);
  const bool uniform = (d->Cin % kBK) == 0;
  const bool fast = fast_ok(a);
  const bool forced = d->tile != YV4_TILE_AUTO;
  const TileId route = forced ? decode_tile_f32(d->tile) : auto_route(a);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tile = route.tile;
  // the kernels with the statistics epilogue: the wide and weight-stationary families, the LDS-DMA tiles
  const bool family = tile == YV4_TILE_W3x3 || tile == YV4_TILE_WIDE || tile == YV4_TILE_WS_1x1;
  const bool dma_tile = tile == YV4_TILE_DMA_64x64 || tile == YV4_TILE_DMA_128x64 || tile == YV4_TILE_DMA_128x128;
  if (stats_done) *stats_done = stats && (family || (fast && dma_tile));
  if (stats_done && *stats_done) a.stats = stats;
  // (a forced id's shape wins; the measurement build's YV4_*_SHAPE overrides the automatic one; -1: the launch picks)
  auto shape_of = [&](int env_shape) { return route.shape >= 0 && (forced || env_shape < 0) ? route.shape : env_shape; };
  if (tile == YV4_TILE_W3x3) {
    YV4_REQUIRE(!forced || (fast && conv3x3_wide_f32_applies(a)), "conv: the wide 3x3 tile needs a 3x3 / stride 1 / pad 1 conv "
                "with Cin %% 32 == 0, Cout %% 16 == 0 (64 .. 1024) and 4-aligned channel strides / offsets");
    static const int env_shape = YV4_ENV_INT("YV4_W3F_SHAPE", -1);
    return conv3x3_wide_f32_launch(a, shape_of(env_shape), s);
  }
  if (tile == YV4_TILE_WIDE) {
    YV4_REQUIRE(!forced || (fast && conv_wide_f32_applies(a)), "conv: the wide tile needs Cin %% 32 == 0, Cout %% 16 == 0 "
                "(64 .. 2048) and 4-aligned channel strides / offsets");
    static const int env_shape = YV4_ENV_INT("YV4_WGF_SHAPE", -1);
    return conv_wide_f32_launch(a, shape_of(env_shape), s);
  }
  if (tile == YV4_TILE_WS_1x1) {
    YV4_REQUIRE(!forced || (fast && conv1x1_ws_f32_applies(a)), "conv: the weight-stationary tile needs a 1x1 / stride 1 conv "
                "with Cin 64, 128 or 256, Cout >= 32 and no residual");
    return conv1x1_ws_f32_launch(a, s);
  }
  switch (tile) {
    case YV4_TILE_128x128: return launch_conv<128, 128, 2, 2>(a, uniform, s);
    case YV4_TILE_128x64: return launch_conv<128, 64, 2, 2>(a, uniform, s);
    case YV4_TILE_64x128: return launch_conv<64, 128, 2, 2>(a, uniform, s);
    case YV4_TILE_64x64: return launch_conv<64, 64, 2, 2>(a, uniform, s);
    case YV4_TILE_STEM: if (stem_ok(a)) return conv_stem_f32_launch(a, YV4_F32, s); break;
    case YV4_TILE_DMA_64x64: if (fast) return launch_conv_dma<64, 64, 2, 2, 2>(a, s); break;
    case YV4_TILE_DMA_128x64: if (fast) return launch_conv_dma<128, 64, 2, 2, 2>(a, s); break;
    case YV4_TILE_DMA_128x128: if (fast) return launch_conv_dma<128, 128, 2, 2, 2>(a, s); break;
    default: break;
  }
  set_error("conv: unknown or inapplicable tile id %d", tile);
  return YV4_E_INVALID;
}

extern "C" int yv4_conv_bn_act_fwd(const yv4_conv_desc* d, const float* x, const float* w,
                                   const float* scale1, const float* shift1,
                                   const float* scale2, const float* shift2,
                                   const float* residual, float* y, void* stream) {
  return conv_f32_impl(d, x, w, scale1, shift1, scale2, shift2, residual, y, nullptr, nullptr, stream);
}

// ---- split-K: the single-image (latency) form of the LDS-DMA kernels ----------------------------------------------
// At batch 1 the deep layers have a handful of tiles (512 -> 512 3x3 at 19x19: 6 x 8 tiles of 64 x 64 on 256 CUs) and
// 144 K slices each: the chip idles while 48 workgroups walk K serially.  Splitting K over `ksplit` workgroups per tile
// fills the CUs; partials go to per-split slabs (plain stores, no atomics) that one small kernel adds IN SLAB ORDER
// before the usual epilogue, so the result is deterministic (but not bit-identical to the unsplit kernel's summation
// order: plans use it for N == 1 only, where no cross-batch bit-exactness is claimed).
namespace yv4 {
__global__ __launch_bounds__(256) void splitk_finish_kernel(ConvArgs p) {
  const int c4n = p.ws_cs >> 2;
  const long long total = (long long)p.M * c4n;
  const bool has2 = p.s2 != nullptr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / c4n);
    const int co = (int)(i - (long long)m * c4n) * 4;
    const float* src = p.ws + (int64_t)m * p.ws_cs + co;
    const size_t slab = (size_t)p.M * p.ws_cs;
    float4 a = *reinterpret_cast<const float4*>(src);
    for (int s = 1; s < p.ksplit; ++s) {
      const float4 b = *reinterpret_cast<const float4*>(src + s * slab);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = co + u;
      if (c >= p.Cout) continue;
      float t = v[u] * p.s1[c] + p.t1[c];
      t = apply_act(t, p.act1, p.slope1);
      if (p.res) t += p.res[(int64_t)m * p.r_cs + p.r_co + c];
      if (has2) t = apply_act(t * p.s2[c] + p.t2[c], p.act2, p.slope2);
      p.y[(int64_t)m * p.y_cs + p.y_co + c] = t;
    }
  }
}

// how many ways to split K for this layer's 64 x 64 LDS-DMA tiles (splitk_ways, conv_route.h): ~2 workgroups per CU, at
// least 8 slices of 32 per split; 1 = do not split (enough tiles already, or a layer outside the LDS-DMA kernels)
static int splitk_choice(const yv4_conv_desc* d) {
  const long long M = (long long)d->N * d->Ho * d->Wo;
  const ConvArgs a = conv_args(d);
  if (!fast_ok(a)) return 1;
  const long long tiles = ((M + 63) / 64) * ((d->Cout + 63) / 64);
  static const long long target = (long long)YV4_ENV_INT("YV4_SPLITK_TARGET", (int)(512LL));
  static const int min_slices = YV4_ENV_INT("YV4_SPLITK_MINSL", 8);
  return splitk_ways(tiles, a.K / kBK, target, min_slices);
}
}  // namespace yv4

extern "C" size_t yv4_conv_splitk_workspace(const yv4_conv_desc* d, int* ksplit) {
  if (!d) return 0;
  const int ks = splitk_choice(d);
  if (ksplit) *ksplit = ks;
  return splitk_workspace_bytes(d, ks, 4);
}

extern "C" int yv4_conv_bn_act_fwd_splitk(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1,
                                          const float* shift1, const float* scale2, const float* shift2,
                                          const float* residual, float* y, float* workspace, size_t workspace_bytes,
                                          void* stream) {
  YV4_REQUIRE(d, "conv splitk: null descriptor");
  const int ks = splitk_choice(d);
  if (ks <= 1) return yv4_conv_bn_act_fwd(d, x, w, scale1, shift1, scale2, shift2, residual, y, stream);
  YV4_REQUIRE(x && w && scale1 && shift1 && y && workspace, "conv splitk: null argument");
  YV4_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), "conv splitk: scale2/shift2 must come together");
  if (int rc = check_conv_desc(d, "conv splitk", {4, residual != nullptr})) return rc;
  YV4_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
              "conv splitk: x / w / workspace must be 16-byte aligned");
  YV4_REQUIRE(workspace_bytes >= splitk_workspace_bytes(d, ks, 4), "conv splitk: workspace too small");
  ConvArgs a = conv_args(d, x, w, scale1, shift1, scale2, shift2, residual, y);
  splitk_set(a, ks, kBK, 4, workspace);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = launch_conv_dma<64, 64, 2, 2, 2>(a, s)) return rc;
  hipLaunchKernelGGL(splitk_finish_kernel, dim3(splitk_finish_grid(a, 4)), dim3(256), 0, s, a);
  YV4_CHECK_LAUNCH("conv splitk finish");
  return YV4_OK;
}

// Training-mode convolution feeding a BatchNorm: y = conv(x, w) (identity epilogue, `ones` / `zeros` = Cout unit
// scales / zero shifts) and the per-channel sums of y for the batch statistics, accumulated by the conv kernel's
// epilogue where the selected kernel supports it, else by the BN reduction kernel afterwards -- either way
// `stats` holds YV4_STATS_REPLICAS x [sum (Cout) | sum of squares (Cout)] whose column sums are the totals.
extern "C" int yv4_conv_fwd_stats(const yv4_conv_desc* d, int dtype, const void* x, const void* w, const float* ones,
                                  const float* zeros, void* y, double* stats, int stats_is_zero, void* stream) {
  YV4_REQUIRE(d && stats, "conv_fwd_stats: null argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "conv_fwd_stats: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(d->y_coff >= 0 && d->y_coff + d->Cout <= d->y_cstride && d->act1 == YV4_ACT_NONE,
              "conv_fwd_stats: the output view exceeds its pixel stride, or the epilogue is not the identity");
  if (!stats_is_zero &&
      hipMemsetAsync(stats, 0, sizeof(double) * YV4_STATS_REPLICAS * 2 * d->Cout, reinterpret_cast<hipStream_t>(stream)) !=
          hipSuccess) {
    set_error("conv_fwd_stats: memset failed");
    return YV4_E_LAUNCH;
  }
  // deterministic mode: the kernels receive the pointer with bit 0 set (stat_rep) and fill fixed-point replica pairs
  double* const kstats = tag_stats(stats);
  if (dtype != YV4_F32) return conv_stats_h16(d, dtype, x, w, ones, zeros, y, kstats, stream);
  bool done = false;
  const int rc = conv_f32_impl(d, reinterpret_cast<const float*>(x), reinterpret_cast<const float*>(w), ones, zeros, nullptr,
                               nullptr, nullptr, reinterpret_cast<float*>(y), kstats, &done, stream);
  if (rc != YV4_OK || done) return rc;
  // (a tile without the statistics epilogue: one pass over y into replica 0 -- replica pair 0 in deterministic mode)
  return bn_partial_sums_replica0(y, YV4_F32, (int64_t)d->N * d->Ho * d->Wo, d->Cout, d->y_cstride, d->y_coff, stats, stream);
}

// Convolution with a scattered store: output pixel (n, ho, wo) goes to y[n, ho*sh + oh, wo*sw + ow, :]
// of an (N, Hy, Wy, y_cstride) tensor, and d->Ho / d->Wo are taken as given (input rows past the
// bottom / right edge read zeros).  This is one parity class of the data gradient of a stride-2
// convolution: dX[2i+a, 2j+b] is a stride-1 correlation of dY with the taps of matching parity, so the
// four classes together cost exactly the forward FLOPs (a zero-dilated dY costs 4x).
extern "C" int yv4_conv_scatter_fwd(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1,
                                    const float* shift1, float* y, int Hy, int Wy, int sh, int sw, int oh, int ow,
                                    void* stream) {
  YV4_REQUIRE(d && x && w && scale1 && shift1 && y, "conv scatter: null argument");
  ConvDescRules rules{4};
  rules.scatter = true; rules.acts = 0;      // (identity epilogue, whatever the descriptor's activation fields hold)
  if (int rc = check_conv_desc(d, "conv scatter", rules)) return rc;
  YV4_REQUIRE(d->Cin % kBK == 0, "conv scatter: Cin must be a multiple of 32 (the LDS-DMA tiles)");
  YV4_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "conv scatter: x / w must be 16-byte aligned");
  YV4_REQUIRE(sh > 0 && sw > 0 && oh >= 0 && ow >= 0 && (d->Ho - 1) * sh + oh < Hy && (d->Wo - 1) * sw + ow < Wy,
              "conv scatter: the scattered grid does not fit the output tensor");
  ConvArgs a = conv_args(d, x, w, scale1, shift1, nullptr, nullptr, nullptr, y);
  YV4_REQUIRE(dma_addressable(a), "conv scatter: tensors of 4 GiB or more are not supported");
  a.act1 = 0; a.act2 = 0;      // identity epilogue, whatever the descriptor's activation fields hold
  a.ys_on = 1; a.ys_H = Hy; a.ys_W = Wy; a.ys_sh = sh; a.ys_sw = sw; a.ys_oh = oh; a.ys_ow = ow;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tile = d->tile == YV4_TILE_AUTO ? YV4_TILE_DMA_64x64 : d->tile;
  switch (tile) {
    case YV4_TILE_DMA_64x64: return launch_conv_dma<64, 64, 2, 2, 2>(a, s);
    case YV4_TILE_DMA_128x64: return launch_conv_dma<128, 64, 2, 2, 2>(a, s);
    case YV4_TILE_DMA_128x128: return launch_conv_dma<128, 128, 2, 2, 2>(a, s);
    default: break;
  }
  set_error("conv scatter: tile id %d is not an LDS-DMA tile", tile);
  return YV4_E_INVALID;
}
