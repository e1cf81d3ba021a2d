// Train-mode BatchNorm (+ activation, + residual) forward / backward on gfx950: statistics, finalize, fold, the
// general row passes and the pipelined 16-bit Mish passes (bn16_*), with their launch code and C entries.
//
// What they replace in the reference's training step:
//   ATen batch_norm forward/backward in training mode + MishCudaFunction.backward (mish.py:27-36)
#include "train_common.h"

namespace yv4 {

// ---------------------------------------------------------------------------------
// Train-mode BatchNorm.  x is an NHWC view (M rows, C channels).
//   stats:   per-channel sum and sum of squares, fp64 partials per workgroup -> atomics (double)
//   fwd:     z = (x - mean) * invstd * gamma + beta;  y = act(z) (+ residual)
//   bwd:     g = dy * act'(z);  dbeta = sum g;  dgamma = sum g * xhat;
//            dx = gamma * invstd * (g - dbeta/M - xhat * dgamma/M)
// act in {none, Mish, LeakyReLU, Swish}; Mish' as mmdet/ops/mish_cuda/src/mish.h:21-29.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float act_grad(float z, int act, float slope) {
  switch (act) {
    case YV4_ACT_MISH: {
      // mish.h:21-29 with sp = log1p(e^z), a = 1 + e^z, w = a^2 + 1:  tanh(sp) = (a^2 - 1) / (a^2 + 1) = 1 - 2 / w  and
      // (1 - tanh^2(sp)) * (1 - exp(-sp)) = (4 a^2 / w^2) * (e / a), so
      //     mish'(z) = 1 - 2 / w + 4 z a e / w^2
      // -- ONE reciprocal and one exp2 (hardware, 1 ulp each; quarter-rate instructions): |error| < 1e-6 against the libm
      // form, well inside the 1e-4 gradient budget.  The two BN-backward kernels are bound by exactly this arithmetic
      // (~35 issue slots per element at 16 lanes per SIMD and clock = their 0.6 ms on the 757 M-element layer); the
      // earlier form spent two reciprocals and ~6 more slots here.
      const float e = __builtin_amdgcn_exp2f(fminf(z, 20.f) * 1.44269504088896340736f);
      const float a = e + 1.f;
      const float iw = __builtin_amdgcn_rcpf(__builtin_fmaf(a, a, 1.f));
      const float g = __builtin_fmaf(4.f * (z * (a * e)), iw * iw, __builtin_fmaf(-2.f, iw, 1.f));
      return z >= 20.f ? 1.f : g;
    }
    case YV4_ACT_LEAKY: return z > 0.f ? 1.f : slope;   // (torch's leaky_relu_backward: slope AT zero, either sign of it)
    case YV4_ACT_SWISH: {
      const float s = 1.f / (1.f + expf(-z));
      return s + z * s * (1.f - s);
    }
    default: return 1.f;
  }
}
// Two channels at a time for the Mish passes of the BatchNorm kernels: the compiler does not pair the per-channel fp32
// arithmetic by itself (no v_pk_* in the scalar loops), and these kernels are bound by their VALU issue slots (a wave
// instruction takes four cycles on a 16-lane SIMD: ~30 slots per element = 0.6 ms on the 757 M-element layer, which is
// also its HBM time).  Every operation below is the scalar path's, done on a pair -- v_pk_mul / v_pk_add / v_pk_fma --
// so the results are bit for bit the scalar ones; the transcendentals stay one per element.
__device__ __forceinline__ f32x2_t splat2(float v) { f32x2_t r; r.x = v; r.y = v; return r; }
__device__ __forceinline__ f32x2_t mish_grad2(f32x2_t z) {
  f32x2_t zc;
  zc.x = fminf(z.x, 20.f); zc.y = fminf(z.y, 20.f);
  const f32x2_t t = zc * 1.44269504088896340736f;
  f32x2_t e;
  e.x = __builtin_amdgcn_exp2f(t.x); e.y = __builtin_amdgcn_exp2f(t.y);
  const f32x2_t a = e + 1.f;
  const f32x2_t w = __builtin_elementwise_fma(a, a, splat2(1.f));
  f32x2_t iw;
  iw.x = __builtin_amdgcn_rcpf(w.x); iw.y = __builtin_amdgcn_rcpf(w.y);
  f32x2_t g = __builtin_elementwise_fma(4.f * (z * (a * e)), iw * iw, __builtin_elementwise_fma(splat2(-2.f), iw, splat2(1.f)));
  g.x = z.x >= 20.f ? 1.f : g.x;
  g.y = z.y >= 20.f ? 1.f : g.y;
  return g;
}
// mish_fast_f32 on a pair, expression for expression: e = exp2(x log2 e), n = e (e + 2), (x n) / (n + 2), x itself from 20 on
__device__ __forceinline__ f32x2_t mish_fwd2(f32x2_t x) {
  const f32x2_t t = x * 1.44269504088896340736f;
  f32x2_t e;
  e.x = __builtin_amdgcn_exp2f(t.x); e.y = __builtin_amdgcn_exp2f(t.y);
  const f32x2_t n = e * (e + 2.f);
  const f32x2_t d = n + 2.f;
  f32x2_t r;
  r.x = __builtin_amdgcn_rcpf(d.x); r.y = __builtin_amdgcn_rcpf(d.y);
  f32x2_t y = (x * n) * r;
  y.x = x.x >= 20.f ? x.x : y.x;
  y.y = x.y >= 20.f ? x.y : y.y;
  return y;
}
// (the forward of the fused BN + activation uses apply_act -- hardware exp2 / rcp Mish, < 2e-6 absolute from the
// libm form: with the libm form the kernel was VALU-bound, ~45 instructions per element at 2 bytes in, 2 out)
__device__ __forceinline__ float act_fwd_exact(float z, int act, float slope) {
  switch (act) {
    case YV4_ACT_MISH: return mish_f32(z);
    case YV4_ACT_LEAKY: return z >= 0.f ? z : z * slope;
    case YV4_ACT_SWISH: return z * sigmoid_f32(z);
    default: return z;
  }
}

#ifndef YV4_BN_RED_WAVES
#define YV4_BN_RED_WAVES 1
#endif
#ifndef YV4_BN_APPLY_WAVES
#define YV4_BN_APPLY_WAVES 1
#endif
constexpr int kBnRows = 8192;  // rows per workgroup at most (512 measured 1.2-1.5x slower on the >= 1 M-row maps:
                               // the per-workgroup LDS / global atomics then outweigh 32 KB of streaming)

// Thread map of the per-channel reductions: a row of the NHWC view is C4 = C/4 float4s; the
// workgroup's 256 threads cover rows_per_pass = 256 / C4 rows at a time (all threads busy and
// perfectly coalesced for every C4 <= 256; wider rows are walked in passes of 256 float4s).
struct RedMap {
  int cq0, cq_step, rsub, rstep;
  bool active;
};
__device__ __forceinline__ RedMap red_map(int C4) {
  RedMap m;
  if (C4 <= 256) {
    const int rpp = 256 / C4;
    m.active = (int)threadIdx.x < rpp * C4;
    m.cq0 = threadIdx.x % C4;
    m.cq_step = C4;          // one quad per thread
    m.rsub = threadIdx.x / C4;
    m.rstep = rpp;
  } else {
    m.active = true;
    m.cq0 = threadIdx.x;
    m.cq_step = 256;
    m.rsub = 0;
    m.rstep = 1;
  }
  return m;
}

// Block-level combine of per-thread partials (a: first C values, b: second C values) and one
// double atomic per channel per workgroup.  part[] lives in LDS: [2][C] doubles.
// det (yv4_set_deterministic): part[] is [2][2*C] 64-bit words -- hi words of (a | b), then their lo words (fx_add)
template <int SHIFT, int FR = 0>
__device__ __forceinline__ void red_flush(double* part, int C, int c, const double (&a)[4], const double (&b)[4],
                                          bool active, int det) {
  if (active) {
    u64_t* w = reinterpret_cast<u64_t*>(part);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (det) {
        fx_add<SHIFT, FR>(w + c + k, w + 2 * C + c + k, a[k]);
        fx_add<SHIFT, FR>(w + C + c + k, w + 3 * C + c + k, b[k]);
      } else {
        atomicAdd(&part[c + k], a[k]);
        atomicAdd(&part[C + c + k], b[k]);
      }
    }
  }
}
// a workgroup's fixed-point words -> the global accumulator's (the sticky non-finite bit travels as an OR)
__device__ __forceinline__ void fx_merge(u64_t* ghi, u64_t* glo, u64_t h, u64_t l) {
  if (h) atomicAdd(ghi, h);
  if (l >> 63) atomicOr(glo, 1ull << 63);
  l &= ~(1ull << 63);
  if (l) atomicAdd(glo, l);
}
constexpr int kBnFloatRun = 16;  // unrolled iterations (x4 rows) a thread sums in fp32 before folding into its doubles

#ifndef YV4_BN_UNROLL
#define YV4_BN_UNROLL 4
#endif
constexpr int kBnUnroll = YV4_BN_UNROLL;    // independent row loads in flight per thread (the loops are latency-bound otherwise)
#ifndef YV4_BN_RED_UNROLL
#define YV4_BN_RED_UNROLL 2
#endif
constexpr int kBnRedUnroll = YV4_BN_RED_UNROLL;   // (4 and 8 measured 0.8 % / 3 % slower on the whole step: registers -> occupancy)

// rows per workgroup: enough workgroups to fill the chip (>= ~1024) but at most kBnRows rows each
static const int g_bn_rows_cap = YV4_ENV_INT("YV4_BN_ROWS", kBnRows);
static const int g_bn_min_wg = YV4_ENV_INT("YV4_BN_MINWG", 1024);
static inline int bn_rows_per_block(int64_t M) {
  int64_t r = (M + g_bn_min_wg - 1) / g_bn_min_wg;
  if (r < 32) r = 32;
  if (r > g_bn_rows_cap) r = g_bn_rows_cap;
  return (int)r;
}

// sums[c] += sum x, sums[C + c] += sum x^2   (double)
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ x, int64_t M, int C, int cs, int co,
                                                       double* __restrict__ sums, int rows_per_block, int det) {
  extern __shared__ double part[];   // [2][C]; det: [4][C] words
  const int C4 = C >> 2;
  for (int i = threadIdx.x; i < (det ? 4 : 2) * C; i += 256) part[i] = 0.0;
  __syncthreads();
  const RedMap mp = red_map(C4);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  if (mp.active) {
    for (int cq = mp.cq0; cq < C4; cq += mp.cq_step) {
      float fs[4] = {0, 0, 0, 0}, fq[4] = {0, 0, 0, 0};
      double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
      int it = 0;
      const T* col = x + co + cq * 4;
      for (int64_t rr = r0 + mp.rsub; rr < r1; rr += (int64_t)mp.rstep * kBnRedUnroll) {
        if (++it == kBnFloatRun) {       // bound the length of an fp32 running sum (64 rows)
          it = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) { ds[k] += fs[k]; dq[k] += fq[k]; fs[k] = 0.f; fq[k] = 0.f; }
        }
        float4 v[kBnRedUnroll];
#pragma unroll
        for (int u = 0; u < kBnRedUnroll; ++u) {
          const int64_t row = rr + (int64_t)u * mp.rstep;
          v[u] = row < r1 ? El<T>::ld4(col + row * cs) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kBnRedUnroll; ++u) {
          fs[0] += v[u].x; fs[1] += v[u].y; fs[2] += v[u].z; fs[3] += v[u].w;
          fq[0] += v[u].x * v[u].x; fq[1] += v[u].y * v[u].y; fq[2] += v[u].z * v[u].z; fq[3] += v[u].w * v[u].w;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) { ds[k] += fs[k]; dq[k] += fq[k]; }
      red_flush<kFxStat, kFxStatFr>(part, C, cq * 4, ds, dq, true, det);
    }
  }
  __syncthreads();
  if (det) {      // sums: [hi words (2*C) | lo words (2*C)]
    const u64_t* w = reinterpret_cast<const u64_t*>(part);
    u64_t* g = reinterpret_cast<u64_t*>(sums);
    for (int i = threadIdx.x; i < 2 * C; i += 256) fx_merge(g + i, g + 2 * C + i, w[i], w[2 * C + i]);
    return;
  }
  for (int i = threadIdx.x; i < 2 * C; i += 256) atomicAdd(&sums[i], part[i]);
}
// det: the words of [hi (n) | lo (n)] -> n doubles in place (consumers outside the library: SyncBN's all-reduce)
template <int SHIFT, int FR = 0>
__global__ void fx_decode_kernel(double* __restrict__ buf, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64_t* w = reinterpret_cast<const u64_t*>(buf);
  buf[i] = fx_value<SHIFT, FR>(w[i], w[n + i]);
}

// mean / biased var / invstd from the sums; running stats update (unbiased var, momentum)
// `rows`: optional device-resident row count (SyncBN: the all-reduced count travels with the sums)
// clear_work: the replicas are zeroed as they are read (a persistent statistics buffer is clean again for the next
// forward); zero_after: 4*C doubles cleared for the backward reduction of the same layer -- both replace memsets.
__global__ void bn_finalize_kernel(double* __restrict__ sums, int64_t M_host, int C, float eps, float momentum,
                                   float* mean, float* invstd, float* running_mean, float* running_var,
                                   const double* __restrict__ rows, int replicas, int clear_work,
                                   double* __restrict__ zero_after, int det) {
  // 256 threads = 32 channels x 8 replica lanes: a lane adds every 8th replica (independent loads in flight), the 8
  // lanes of a channel combine by shuffle.  (One thread per channel walking 64 replicas was a chain of 128 dependent
  // loads: 18 us per call, 2 ms of the bf16 train step over its 108 BatchNorms.)
  const int c = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int rl = threadIdx.x & 7;
  double s1 = 0.0, s2 = 0.0;
  // Every load of a lane is issued before the first is used (the first YV4_STATS_REPLICAS = 64 replicas: eight per lane;
  // a larger count adds a loop over the rest): as a loop over a run-time count the loads went out one iteration at a time behind the zeroing stores of the
  // iteration before -- a chain of eight memory round trips, 7.5 us per call and 0.85 ms of the bf16 train step.
  if (det) {
    // replica PAIRS of fixed-point words (stat_rep / bn_stats_kernel): integer sums over the pairs, any order
    u64_t h1 = 0, l1 = 0, h2 = 0, l2 = 0;
    if (c < C) {
      u64_t* w = reinterpret_cast<u64_t*>(sums);
      u64_t v[4][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = rl + 8 * k;
        const bool in = r < replicas / 2;
        u64_t* hp = w + (size_t)(2 * (in ? r : 0)) * 2 * C;
        u64_t* lp = hp + 2 * C;
        v[k][0] = in ? hp[c] : 0; v[k][1] = in ? lp[c] : 0; v[k][2] = in ? hp[C + c] : 0; v[k][3] = in ? lp[C + c] : 0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        fx_fold(h1, l1, v[k][0], v[k][1]);
        fx_fold(h2, l2, v[k][2], v[k][3]);
      }
      if (clear_work) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int r = rl + 8 * k;
          if (r < replicas / 2) {
            u64_t* hp = w + (size_t)(2 * r) * 2 * C;
            u64_t* lp = hp + 2 * C;
            hp[c] = 0; hp[C + c] = 0; lp[c] = 0; lp[C + c] = 0;
          }
        }
      }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      fx_fold(h1, l1, __shfl_xor(h1, o), __shfl_xor(l1, o));
      fx_fold(h2, l2, __shfl_xor(h2, o), __shfl_xor(l2, o));
    }
    s1 = fx_value<kFxStat, kFxStatFr>(h1, l1);
    s2 = fx_value<kFxStat, kFxStatFr>(h2, l2);
  } else {
    if (c < C) {
      double a1[8], a2[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int r = rl + 8 * k;
        const bool in = r < replicas;
        a1[k] = in ? sums[(size_t)r * 2 * C + c] : 0.0;
        a2[k] = in ? sums[(size_t)r * 2 * C + C + c] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) { s1 += a1[k]; s2 += a2[k]; }      // (replica order rl, rl + 8, ...: as before)
      if (clear_work) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int r = rl + 8 * k;
          if (r < replicas) {
            sums[(size_t)r * 2 * C + c] = 0.0;
            sums[(size_t)r * 2 * C + C + c] = 0.0;
          }
        }
      }
      // replicas beyond the unrolled 64 (a caller's own block count, yv4_bn_finalize): the same lane stride, summed and
      // cleared one at a time.  The conv epilogue's 64 and SyncBN's 1 never enter this loop.
      for (int r = 64 + rl; r < replicas; r += 8) {
        s1 += sums[(size_t)r * 2 * C + c];
        s2 += sums[(size_t)r * 2 * C + C + c];
        if (clear_work) {
          sums[(size_t)r * 2 * C + c] = 0.0;
          sums[(size_t)r * 2 * C + C + c] = 0.0;
        }
      }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
  }
  if (c < C && zero_after && rl == 0) {      // 4*C words: [dbeta | dgamma] and, in deterministic mode, their lo words
#pragma unroll
    for (int k = 0; k < 4; ++k) zero_after[k * C + c] = 0.0;
  }
  if (c >= C || rl != 0) return;
  const double M = rows ? *rows : (double)M_host;
  const double m = s1 / M;
  double var = s2 / M - m * m;
  if (var < 0) var = 0;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = M > 1 ? var * M / (M - 1) : var;
    running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
}

// totals of a conv epilogue's replicas as 2*C doubles (SyncBN: they are all-reduced before the finalize)
__global__ void stats_fold_kernel(double* __restrict__ sums, int C, int replicas, int clear_work, double* __restrict__ out,
                                  int det) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * C) return;
  if (det) {
    u64_t* w = reinterpret_cast<u64_t*>(sums);
    u64_t h = 0, l = 0;
    for (int r = 0; r < replicas / 2; ++r) {
      u64_t* hp = w + (size_t)(2 * r) * 2 * C + i;
      fx_fold(h, l, hp[0], hp[2 * C]);
      if (clear_work) { hp[0] = 0; hp[2 * C] = 0; }
    }
    out[i] = fx_value<kFxStat, kFxStatFr>(h, l);
  } else {
    double a = 0.0;
    for (int r = 0; r < replicas; ++r) {
      a += sums[(size_t)r * 2 * C + i];
      if (clear_work) sums[(size_t)r * 2 * C + i] = 0.0;
    }
    out[i] = a;
  }
}

struct BnArgs {
  const void* x; int x_cs, x_co;
  const float* mean; const float* invstd; const float* gamma; const float* beta;
  const void* res; int r_cs, r_co;
  void* y; int y_cs, y_co;
  const void* dy; int dy_cs, dy_co;
  void* dx; int dx_cs, dx_co;
  double* sums;      // bwd: [dbeta (C) | dgamma (C)]
  float* dgamma; float* dbeta;   // written by workgroup 0 of the apply pass
  int64_t M; int C; int act; float slope;
  int rows_per_block;
  int eval_mode;     // backward of an eval-mode BN (running statistics are constants): no mean/variance terms
  int64_t M_total;   // rows behind the statistics (= M, or the sum over ranks for SyncBN)
  const double* rows; // optional device-resident M_total
  int publish;       // the apply pass writes dgamma / dbeta from `sums` (not when `sums` were all-reduced)
  int red_cg;        // bn_act_bwd_reduce_kernel: channels per workgroup (grid.y groups)
  int det;           // `sums` holds fixed-point words: [hi (2*C) | lo (2*C)] (yv4_set_deterministic)
};

// entry i of the backward sums [dbeta (C) | dgamma (C)]
__device__ __forceinline__ double bn_sum(const BnArgs& p, int i) {
  if (!p.det) return p.sums[i];
  const u64_t* w = reinterpret_cast<const u64_t*>(p.sums);
  return fx_value<kFxGrad>(w[i], w[2 * p.C + i]);
}

// Elementwise passes use the reductions' thread map too: a thread keeps ONE channel group of V channels (its
// mean / invstd / gamma / beta live in registers) and walks rows -- no per-element index division,
// kBnUnroll independent row loads in flight.  V = 4 channels per thread (V = 8 for 16-bit rows: YV4_BN_VEC8=1).
// YV4_BN_NT (build-time, tools/ab_bn_nt.sh): 1 = the BatchNorm passes' row loads non-temporal, 2 = their stores.  Measured at
// YOLOv4-L 608 batch 64 bf16 on one box (profiles/r05_bn_nt_ab.txt): non-temporal STORES take the forward pass from 4.04 to
// 3.78 ms per step and the backward apply pass from 6.21 to 6.11, the train step from 1 194 to 1 199-1 204 images/s;
// non-temporal loads cost 4 % on both.  Default: stores only.
#ifndef YV4_BN_NT
#define YV4_BN_NT 2
#endif

template <typename T, int V> struct RowVec {
  typedef T raw __attribute__((ext_vector_type(V)));
  static __device__ __forceinline__ raw ld(const T* p) {
    if (YV4_BN_NT & 1) return __builtin_nontemporal_load(reinterpret_cast<const raw*>(p));
    return *reinterpret_cast<const raw*>(p);
  }
  static __device__ __forceinline__ void st(T* p, const float (&v)[V]) {
    raw o;
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = (T)v[k];
    if (YV4_BN_NT & 2) __builtin_nontemporal_store(o, reinterpret_cast<raw*>(p));
    else *reinterpret_cast<raw*>(p) = o;
  }
  static __device__ __forceinline__ raw zero() {
    raw o;
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = (T)0.f;
    return o;
  }
};

template <typename T, int V>
__global__ __launch_bounds__(256, YV4_BN_APPLY_WAVES) void bn_act_fwd_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  const T* px = reinterpret_cast<const T*>(p.x);
  const T* pres = reinterpret_cast<const T*>(p.res);
  T* py = reinterpret_cast<T*>(p.y);
  const int CV = p.C / V;
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  if (!mp.active) return;
  for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
    const int c = cq * V;
    float mu[V], sa[V], be[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {       // z = (x - mu) * sa + be
      mu[k] = p.mean[c + k]; sa[k] = p.invstd[c + k] * p.gamma[c + k]; be[k] = p.beta[c + k];
    }
    for (int64_t rr = r0 + mp.rsub; rr < r1; rr += (int64_t)mp.rstep * kBnUnroll) {
      typename RV::raw v[kBnUnroll], rs[kBnUnroll];
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        const bool ok = row < r1;
        v[u] = ok ? RV::ld(px + row * p.x_cs + p.x_co + c) : RV::zero();
        rs[u] = (ok && pres) ? RV::ld(pres + row * p.r_cs + p.r_co + c) : RV::zero();
      }
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        if (row >= r1) continue;
        float o[V];
        if (p.act == YV4_ACT_MISH) {      // (uniform) pairs of channels: see mish_grad2
#pragma unroll
          for (int k = 0; k < V; k += 2) {
            f32x2_t x2, m2, s2, b2, r2;
            x2.x = (float)v[u][k]; x2.y = (float)v[u][k + 1];
            m2.x = mu[k]; m2.y = mu[k + 1]; s2.x = sa[k]; s2.y = sa[k + 1]; b2.x = be[k]; b2.y = be[k + 1];
            r2.x = (float)rs[u][k]; r2.y = (float)rs[u][k + 1];
            const f32x2_t y2 = mish_fwd2((x2 - m2) * s2 + b2) + r2;
            o[k] = y2.x; o[k + 1] = y2.y;
          }
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = apply_act(((float)v[u][k] - mu[k]) * sa[k] + be[k], p.act, p.slope) + (float)rs[u][k];
        }
        RV::st(py + row * p.y_cs + p.y_co + c, o);
      }
    }
  }
}

// Grid: (row blocks, channel groups of p.red_cg channels).  Every workgroup ends with one double atomic per channel it
// covers; with ~1000 row blocks over ALL channels a small map (38 x 38 x 256 at batch 64: 47 MB) spent 12-14 us of its
// 43 us queueing ~1000 adds on each of its 512 addresses.  Splitting the channels over grid.y keeps the workgroup count
// (and the bytes in flight) and divides the adds per address by the number of groups; a group is >= 64 channels, so a
// workgroup still reads whole 128-byte lines of every row.
template <typename T, int V>
__global__ __launch_bounds__(256, YV4_BN_RED_WAVES) void bn_act_bwd_reduce_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  extern __shared__ double part[];   // [2][Cl]: dbeta | dgamma of this workgroup's channels
  const int cb = (int)blockIdx.y * p.red_cg;
  const int Cl = min(p.red_cg, p.C - cb);
  const T* px = reinterpret_cast<const T*>(p.x) + p.x_co + cb;
  const T* pdy = reinterpret_cast<const T*>(p.dy) + p.dy_co + cb;
  const int CV = Cl / V;
  for (int i = threadIdx.x; i < (p.det ? 4 : 2) * Cl; i += 256) part[i] = 0.0;
  __syncthreads();
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  if (mp.active) {
    for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
      const int c = cq * V;
      float mu[V], is[V], ga[V], be[V];
      // fp32 running sums over this thread's rows (at most rows_per_block / rows-per-pass, a few hundred terms):
      // double registers here cost a wave of occupancy (135 -> 119 VGPRs) and 35 % of the kernel's speed
      float db[V], dg[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        mu[k] = p.mean[cb + c + k]; is[k] = p.invstd[cb + c + k]; ga[k] = p.gamma[cb + c + k]; be[k] = p.beta[cb + c + k];
        db[k] = 0.f; dg[k] = 0.f;
      }
      for (int64_t rr = r0 + mp.rsub; rr < r1; rr += (int64_t)mp.rstep * kBnRedUnroll) {
        typename RV::raw xv[kBnRedUnroll], gv[kBnRedUnroll];
#pragma unroll
        for (int u = 0; u < kBnRedUnroll; ++u) {
          const int64_t row = rr + (int64_t)u * mp.rstep;
          const bool ok = row < r1;
          xv[u] = ok ? RV::ld(px + row * p.x_cs + c) : RV::zero();
          gv[u] = ok ? RV::ld(pdy + row * p.dy_cs + c) : RV::zero();   // zero beyond r1 -> contributes nothing
        }
        if (p.act == YV4_ACT_MISH) {      // (uniform) pairs of channels: see mish_grad2
#pragma unroll
          for (int u = 0; u < kBnRedUnroll; ++u) {
#pragma unroll
            for (int k = 0; k < V; k += 2) {
              f32x2_t x2, g2, m2, i2, a2, b2, db2, dg2;
              x2.x = (float)xv[u][k]; x2.y = (float)xv[u][k + 1];
              g2.x = (float)gv[u][k]; g2.y = (float)gv[u][k + 1];
              m2.x = mu[k]; m2.y = mu[k + 1]; i2.x = is[k]; i2.y = is[k + 1];
              a2.x = ga[k]; a2.y = ga[k + 1]; b2.x = be[k]; b2.y = be[k + 1];
              db2.x = db[k]; db2.y = db[k + 1]; dg2.x = dg[k]; dg2.y = dg[k + 1];
              const f32x2_t xh2 = (x2 - m2) * i2;
              const f32x2_t gg = g2 * mish_grad2(xh2 * a2 + b2);
              db2 = db2 + gg;
              dg2 = dg2 + gg * xh2;
              db[k] = db2.x; db[k + 1] = db2.y; dg[k] = dg2.x; dg[k + 1] = dg2.y;
            }
          }
        } else {
#pragma unroll
          for (int u = 0; u < kBnRedUnroll; ++u) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
              const float xhat = ((float)xv[u][k] - mu[k]) * is[k];
              const float g = (float)gv[u][k] * act_grad(xhat * ga[k] + be[k], p.act, p.slope);
              db[k] += g;
              dg[k] += g * xhat;
            }
          }
        }
      }
#pragma unroll
      for (int h = 0; h < V; h += 4) {
        const double ddb[4] = {db[h], db[h + 1], db[h + 2], db[h + 3]}, ddg[4] = {dg[h], dg[h + 1], dg[h + 2], dg[h + 3]};
        red_flush<kFxGrad>(part, Cl, c + h, ddb, ddg, true, p.det);
      }
    }
  }
  __syncthreads();
  if (p.det) {
    const u64_t* w = reinterpret_cast<const u64_t*>(part);
    u64_t* g = reinterpret_cast<u64_t*>(p.sums);
    for (int i = threadIdx.x; i < Cl; i += 256) {
      fx_merge(g + cb + i, g + 2 * p.C + cb + i, w[i], w[2 * Cl + i]);
      fx_merge(g + p.C + cb + i, g + 3 * p.C + cb + i, w[Cl + i], w[3 * Cl + i]);
    }
    return;
  }
  for (int i = threadIdx.x; i < Cl; i += 256) {
    atomicAdd(&p.sums[cb + i], part[i]);
    atomicAdd(&p.sums[p.C + cb + i], part[Cl + i]);
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256, YV4_BN_APPLY_WAVES) void bn_act_bwd_apply_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  const T* px = reinterpret_cast<const T*>(p.x);
  const T* pdy = reinterpret_cast<const T*>(p.dy);
  T* pdx = reinterpret_cast<T*>(p.dx);
  const int CV = p.C / V;
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  if (blockIdx.x == 0 && p.publish) {   // the reduction kernel has completed (stream order): publish dbeta / dgamma as fp32
    for (int i = threadIdx.x; i < p.C; i += 256) {
      const double sb = bn_sum(p, i), sg = bn_sum(p, p.C + i);
      if (p.publish == 2) {             // accumulate into existing gradients (the parameter's .grad itself)
        p.dbeta[i] += (float)sb;
        p.dgamma[i] += (float)sg;
      } else {
        p.dbeta[i] = (float)sb;
        p.dgamma[i] = (float)sg;
      }
    }
  }
  if (!mp.active) return;
  const double invM = 1.0 / (p.rows ? *p.rows : (double)p.M_total);
  for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
    const int c = cq * V;
    // dx = k1 * (g - dbm - xhat * dgm),  xhat = (x - mu) * is,  z = xhat * ga + be
    float mu[V], is[V], ga[V], be[V], k1[V], dbm[V], dgm[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      mu[k] = p.mean[c + k]; is[k] = p.invstd[c + k]; ga[k] = p.gamma[c + k]; be[k] = p.beta[c + k];
      k1[k] = ga[k] * is[k];
      dbm[k] = p.eval_mode ? 0.f : (float)(bn_sum(p, c + k) * invM);
      dgm[k] = p.eval_mode ? 0.f : (float)(bn_sum(p, p.C + c + k) * invM);
    }
    for (int64_t rr = r0 + mp.rsub; rr < r1; rr += (int64_t)mp.rstep * kBnUnroll) {
      typename RV::raw xv[kBnUnroll], gv[kBnUnroll];
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        const bool ok = row < r1;
        xv[u] = ok ? RV::ld(px + row * p.x_cs + p.x_co + c) : RV::zero();
        gv[u] = ok ? RV::ld(pdy + row * p.dy_cs + p.dy_co + c) : RV::zero();
      }
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        if (row >= r1) continue;
        float o[V];
        // (scalar on purpose: the paired form of the other two passes costs this one 15 registers and, bound by its
        // 6 bytes per element as it is, 4 % of its speed -- tools/bn_bench.py --kernels, same box)
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xhat = ((float)xv[u][k] - mu[k]) * is[k];
          const float g = (float)gv[u][k] * act_grad(xhat * ga[k] + be[k], p.act, p.slope);
          o[k] = p.eval_mode ? k1[k] * g : k1[k] * (g - dbm[k] - xhat * dgm[k]);
        }
        RV::st(pdx + row * p.dx_cs + p.dx_co + c, o);
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// The three BatchNorm + Mish row passes for 16-bit maps, second form (round 5).  The general kernels above were measured
// at 5.3 / 5.5 / 7.1 ms per bf16 step and priced at "~35 issue slots per element"; the disassembly says otherwise: the
// Mish derivative is 15 packed fp32 operations, 4 transcendentals (8 issue cycles each on this part, not 16), 6 scalar
// compare / select / min and 4 conversions per PAIR of elements = ~150 issue cycles per pair and wave, 2.7 ms per pass on
// the whole chip -- and 4 bytes per element at 5.5 TB/s are 4.2 ms.  The passes run at neither roof but at most of their
// SUM: a wave loads its rows, waits, computes, stores, and 4-5 waves per SIMD do not cover one another's waits.  Here:
//   * the row loop is software-pipelined: the loads of rows i + U .. i + 2U are in flight while rows i .. i + U are
//     computed (two register sets, the loop unrolled by two so that no set is ever copied);
//   * per-channel constants are folded (z = A x + B with A = gamma * invstd, B = beta - mean * A; the backward's
//     dx = k1 g + (c1 x + c0)): 2-5 registers per channel instead of 3-7, one fma instead of subtract + multiply + fma;
//   * Mish and its derivative clamp the exponent's argument instead of selecting the asymptote afterwards (for z >= 20 the
//     expressions round to z and to 1 by themselves): two v_min per pair instead of two compares and two selects;
//   * no run-time activation switch inside the loops (Mish only; anything else stays on the general kernels).
// 16-bit outputs are the fp32 expression rounded once; against the general kernels they differ by the re-association of
// the affine map (<= 1 ulp of the 16-bit type, tests/test_gpu_train_ops.py::test_bn16_*).  fp32 maps never come here.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ f32x2_t exp_clamped2(f32x2_t z) {       // e^min(z, 20)
  f32x2_t zc;
  zc.x = fminf(z.x, 20.f); zc.y = fminf(z.y, 20.f);
  const f32x2_t t = zc * 1.44269504088896340736f;
  f32x2_t e;
  e.x = __builtin_amdgcn_exp2f(t.x); e.y = __builtin_amdgcn_exp2f(t.y);
  return e;
}
__device__ __forceinline__ f32x2_t mish_fwd2c(f32x2_t z) {          // z n / (n + 2), n = e (e + 2)
  const f32x2_t e = exp_clamped2(z);
  const f32x2_t n = e * (e + 2.f);
  const f32x2_t d = n + 2.f;
  f32x2_t r;
  r.x = __builtin_amdgcn_rcpf(d.x); r.y = __builtin_amdgcn_rcpf(d.y);
  return z * (n * r);
}
__device__ __forceinline__ f32x2_t mish_grad2c(f32x2_t z) {         // 1 - u + z a e u^2, a = 1 + e, u = 2 / (a^2 + 1)
  f32x2_t zc;
  zc.x = fminf(z.x, 20.f); zc.y = fminf(z.y, 20.f);
  const f32x2_t t = zc * 1.44269504088896340736f;
  f32x2_t e;
  e.x = __builtin_amdgcn_exp2f(t.x); e.y = __builtin_amdgcn_exp2f(t.y);
  const f32x2_t a = e + 1.f;
  const f32x2_t w = __builtin_elementwise_fma(a, a, splat2(1.f));
  f32x2_t iw;
  iw.x = __builtin_amdgcn_rcpf(w.x); iw.y = __builtin_amdgcn_rcpf(w.y);
  const f32x2_t u = iw + iw;
  return __builtin_elementwise_fma(zc * (a * e), u * u, splat2(1.f) - u);
}

template <typename T, int V, int U>
__global__ __launch_bounds__(256) void bn16_fwd_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  typedef typename RV::raw raw;
  const T* px = reinterpret_cast<const T*>(p.x);
  const T* pres = reinterpret_cast<const T*>(p.res);
  T* py = reinterpret_cast<T*>(p.y);
  const int CV = p.C / V;
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  if (!mp.active) return;
  const bool has_res = pres != nullptr;
  const int64_t step = (int64_t)mp.rstep * U;
  for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
    const int c = cq * V;
    f32x2_t A[V / 2], B[V / 2];
#pragma unroll
    for (int k = 0; k < V; k += 2) {
      A[k / 2].x = p.invstd[c + k] * p.gamma[c + k];
      A[k / 2].y = p.invstd[c + k + 1] * p.gamma[c + k + 1];
      B[k / 2].x = p.beta[c + k] - p.mean[c + k] * A[k / 2].x;
      B[k / 2].y = p.beta[c + k + 1] - p.mean[c + k + 1] * A[k / 2].y;
    }
    // (no range checks in here: a select between a loaded value and zero makes the wave wait for the load where it is
    // ISSUED, which is exactly what the pipeline is there to avoid -- the main loop only runs on whole stages)
    auto load = [&](int64_t rr, raw (&xv)[U], raw (&rv)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        xv[u] = RV::ld(px + row * p.x_cs + p.x_co + c);
        rv[u] = has_res ? RV::ld(pres + row * p.r_cs + p.r_co + c) : RV::zero();
      }
    };
    auto work = [&](int64_t rr, const raw (&xv)[U], const raw (&rv)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        float o[V];
#pragma unroll
        for (int k = 0; k < V; k += 2) {
          f32x2_t x2, r2;
          x2.x = (float)xv[u][k]; x2.y = (float)xv[u][k + 1];
          r2.x = (float)rv[u][k]; r2.y = (float)rv[u][k + 1];
          const f32x2_t y2 = mish_fwd2c(__builtin_elementwise_fma(x2, A[k / 2], B[k / 2])) + r2;
          o[k] = y2.x; o[k + 1] = y2.y;
        }
        RV::st(py + row * p.y_cs + p.y_co + c, o);
      }
    };
    raw xa[U], ra[U], xb[U], rb[U];
    int64_t rr = r0 + mp.rsub;
    const int64_t span = (int64_t)(2 * U - 1) * mp.rstep;      // a double stage starting at rr touches rows rr .. rr + span
    if (rr + span < r1) {
      load(rr, xa, ra);
      for (;;) {
        load(rr + step, xb, rb);
        work(rr, xa, ra);
        const int64_t nx = rr + 2 * step;
        const bool more = nx + span < r1;
        load(more ? nx : rr, xa, ra);      // (always issued -- past the end it re-reads this stage: a branch here makes the
                                             // compiler wait for EVERY load at the join, the next stage's included)
        work(rr + step, xb, rb);
        rr = nx;
        if (!more) break;
      }
    }
    for (; rr < r1; rr += mp.rstep) {                           // the rows that do not fill a double stage
      const raw xv = RV::ld(px + rr * p.x_cs + p.x_co + c);
      const raw rv = has_res ? RV::ld(pres + rr * p.r_cs + p.r_co + c) : RV::zero();
      float o[V];
#pragma unroll
      for (int k = 0; k < V; k += 2) {
        f32x2_t x2, r2;
        x2.x = (float)xv[k]; x2.y = (float)xv[k + 1];
        r2.x = (float)rv[k]; r2.y = (float)rv[k + 1];
        const f32x2_t y2 = mish_fwd2c(__builtin_elementwise_fma(x2, A[k / 2], B[k / 2])) + r2;
        o[k] = y2.x; o[k + 1] = y2.y;
      }
      RV::st(py + rr * p.y_cs + p.y_co + c, o);
    }
  }
}

template <typename T, int V, int U>
__global__ __launch_bounds__(256) void bn16_bwd_reduce_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  typedef typename RV::raw raw;
  extern __shared__ double part[];   // [2][Cl]: dbeta | dgamma of this workgroup's channels (det: [4][Cl] words)
  const int cb = (int)blockIdx.y * p.red_cg;
  const int Cl = min(p.red_cg, p.C - cb);
  const T* px = reinterpret_cast<const T*>(p.x) + p.x_co + cb;
  const T* pdy = reinterpret_cast<const T*>(p.dy) + p.dy_co + cb;
  const int CV = Cl / V;
  for (int i = threadIdx.x; i < (p.det ? 4 : 2) * Cl; i += 256) part[i] = 0.0;
  __syncthreads();
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  const int64_t step = (int64_t)mp.rstep * U;
  if (mp.active) {
    for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
      const int c = cq * V;
      // z = A x + B, xhat = I x + J
      f32x2_t A[V / 2], B[V / 2], I[V / 2], J[V / 2], db[V / 2], dg[V / 2];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float is = p.invstd[cb + c + k], mu = p.mean[cb + c + k], ga = p.gamma[cb + c + k], be = p.beta[cb + c + k];
        const float a_ = is * ga;
        if (k & 1) { A[k / 2].y = a_; B[k / 2].y = be - mu * a_; I[k / 2].y = is; J[k / 2].y = -mu * is; }
        else { A[k / 2].x = a_; B[k / 2].x = be - mu * a_; I[k / 2].x = is; J[k / 2].x = -mu * is; }
      }
#pragma unroll
      for (int k = 0; k < V / 2; ++k) { db[k] = splat2(0.f); dg[k] = splat2(0.f); }
      auto load = [&](int64_t rr, raw (&xv)[U], raw (&gv)[U]) {       // (whole stages only: see bn16_fwd_kernel)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t row = rr + (int64_t)u * mp.rstep;
          xv[u] = RV::ld(px + row * p.x_cs + c);
          gv[u] = RV::ld(pdy + row * p.dy_cs + c);
        }
      };
      auto row_terms = [&](const raw& xv, const raw& gv) {
#pragma unroll
        for (int k = 0; k < V; k += 2) {
          f32x2_t x2, g2;
          x2.x = (float)xv[k]; x2.y = (float)xv[k + 1];
          g2.x = (float)gv[k]; g2.y = (float)gv[k + 1];
          const f32x2_t gg = g2 * mish_grad2c(__builtin_elementwise_fma(x2, A[k / 2], B[k / 2]));
          db[k / 2] = db[k / 2] + gg;
          dg[k / 2] = __builtin_elementwise_fma(gg, __builtin_elementwise_fma(x2, I[k / 2], J[k / 2]), dg[k / 2]);
        }
      };
      auto work = [&](const raw (&xv)[U], const raw (&gv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) row_terms(xv[u], gv[u]);
      };
      raw xa[U], ga[U], xb[U], gb[U];
      int64_t rr = r0 + mp.rsub;
      const int64_t span = (int64_t)(2 * U - 1) * mp.rstep;
      if (rr + span < r1) {
        load(rr, xa, ga);
        for (;;) {
          load(rr + step, xb, gb);
          work(xa, ga);
          const int64_t nx = rr + 2 * step;
          const bool more = nx + span < r1;
          load(more ? nx : rr, xa, ga);      // (always issued -- past the end it re-reads this stage: a branch here makes the
                                             // compiler wait for EVERY load at the join, the next stage's included)
          work(xb, gb);
          rr = nx;
          if (!more) break;
        }
      }
      for (; rr < r1; rr += mp.rstep) row_terms(RV::ld(px + rr * p.x_cs + c), RV::ld(pdy + rr * p.dy_cs + c));
#pragma unroll
      for (int h = 0; h < V; h += 4) {
        const double ddb[4] = {db[h / 2].x, db[h / 2].y, db[h / 2 + 1].x, db[h / 2 + 1].y};
        const double ddg[4] = {dg[h / 2].x, dg[h / 2].y, dg[h / 2 + 1].x, dg[h / 2 + 1].y};
        red_flush<kFxGrad>(part, Cl, c + h, ddb, ddg, true, p.det);
      }
    }
  }
  __syncthreads();
  if (p.det) {
    const u64_t* w = reinterpret_cast<const u64_t*>(part);
    u64_t* g = reinterpret_cast<u64_t*>(p.sums);
    for (int i = threadIdx.x; i < Cl; i += 256) {
      fx_merge(g + cb + i, g + 2 * p.C + cb + i, w[i], w[2 * Cl + i]);
      fx_merge(g + p.C + cb + i, g + 3 * p.C + cb + i, w[Cl + i], w[3 * Cl + i]);
    }
    return;
  }
  for (int i = threadIdx.x; i < Cl; i += 256) {
    atomicAdd(&p.sums[cb + i], part[i]);
    atomicAdd(&p.sums[p.C + cb + i], part[Cl + i]);
  }
}

template <typename T, int V, int U>
__global__ __launch_bounds__(256) void bn16_bwd_apply_kernel(BnArgs p) {
  typedef RowVec<T, V> RV;
  typedef typename RV::raw raw;
  const T* px = reinterpret_cast<const T*>(p.x);
  const T* pdy = reinterpret_cast<const T*>(p.dy);
  T* pdx = reinterpret_cast<T*>(p.dx);
  const int CV = p.C / V;
  const RedMap mp = red_map(CV);
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  if (blockIdx.x == 0 && p.publish) {   // the reduction kernel has completed (stream order): publish dbeta / dgamma as fp32
    for (int i = threadIdx.x; i < p.C; i += 256) {
      const double sb = bn_sum(p, i), sg = bn_sum(p, p.C + i);
      if (p.publish == 2) {
        p.dbeta[i] += (float)sb;
        p.dgamma[i] += (float)sg;
      } else {
        p.dbeta[i] = (float)sb;
        p.dgamma[i] = (float)sg;
      }
    }
  }
  if (!mp.active) return;
  const double invM = 1.0 / (p.rows ? *p.rows : (double)p.M_total);
  const int64_t step = (int64_t)mp.rstep * U;
  for (int cq = mp.cq0; cq < CV; cq += mp.cq_step) {
    const int c = cq * V;
    // dx = k1 (g - dbm - xhat dgm) = k1 g + (c1 x + c0),  c1 = -k1 dgm invstd,  c0 = -k1 dbm + k1 dgm mean invstd
    f32x2_t A[V / 2], B[V / 2], K1[V / 2], C0[V / 2], C1[V / 2];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float is = p.invstd[c + k], mu = p.mean[c + k], ga = p.gamma[c + k], be = p.beta[c + k];
      const float a_ = is * ga;
      const float dbm = p.eval_mode ? 0.f : (float)(bn_sum(p, c + k) * invM);
      const float dgm = p.eval_mode ? 0.f : (float)(bn_sum(p, p.C + c + k) * invM);
      const float k1 = a_, c1 = -(k1 * dgm) * is, c0 = -(k1 * dbm) - c1 * mu;
      if (k & 1) { A[k / 2].y = a_; B[k / 2].y = be - mu * a_; K1[k / 2].y = k1; C0[k / 2].y = c0; C1[k / 2].y = c1; }
      else { A[k / 2].x = a_; B[k / 2].x = be - mu * a_; K1[k / 2].x = k1; C0[k / 2].x = c0; C1[k / 2].x = c1; }
    }
    auto load = [&](int64_t rr, raw (&xv)[U], raw (&gv)[U]) {         // (whole stages only: see bn16_fwd_kernel)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = rr + (int64_t)u * mp.rstep;
        xv[u] = RV::ld(px + row * p.x_cs + p.x_co + c);
        gv[u] = RV::ld(pdy + row * p.dy_cs + p.dy_co + c);
      }
    };
    auto one_row = [&](int64_t row, const raw& xv, const raw& gv) {
      float o[V];
#pragma unroll
      for (int k = 0; k < V; k += 2) {
        f32x2_t x2, g2;
        x2.x = (float)xv[k]; x2.y = (float)xv[k + 1];
        g2.x = (float)gv[k]; g2.y = (float)gv[k + 1];
        const f32x2_t gg = g2 * mish_grad2c(__builtin_elementwise_fma(x2, A[k / 2], B[k / 2]));
        const f32x2_t d2 = __builtin_elementwise_fma(K1[k / 2], gg, __builtin_elementwise_fma(C1[k / 2], x2, C0[k / 2]));
        o[k] = d2.x; o[k + 1] = d2.y;
      }
      RV::st(pdx + row * p.dx_cs + p.dx_co + c, o);
    };
    auto work = [&](int64_t rr, const raw (&xv)[U], const raw (&gv)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) one_row(rr + (int64_t)u * mp.rstep, xv[u], gv[u]);
    };
    raw xa[U], ga[U], xb[U], gb[U];
    int64_t rr = r0 + mp.rsub;
    const int64_t span = (int64_t)(2 * U - 1) * mp.rstep;
    if (rr + span < r1) {
      load(rr, xa, ga);
      for (;;) {
        load(rr + step, xb, gb);
        work(rr, xa, ga);
        const int64_t nx = rr + 2 * step;
        const bool more = nx + span < r1;
        load(more ? nx : rr, xa, ga);      // (always issued -- past the end it re-reads this stage: a branch here makes the
                                             // compiler wait for EVERY load at the join, the next stage's included)
        work(rr + step, xb, gb);
        rr = nx;
        if (!more) break;
      }
    }
    for (; rr < r1; rr += mp.rstep)
      one_row(rr, RV::ld(px + rr * p.x_cs + p.x_co + c), RV::ld(pdy + rr * p.dy_cs + p.dy_co + c));
  }
}

__global__ void sums_to_float_kernel(const double* __restrict__ sums, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)sums[i];
}

}  // namespace yv4

using namespace yv4;

// ... and the vector width of the BN row passes: 4 channels for fp32, 8 for 16-bit operands whose strides allow it
#define YV4_DISPATCH_TV(dtype, v8, CALL)                                          \
  switch (dtype) {                                                                \
    case YV4_F32: { typedef float T; constexpr int V = 4; CALL; } break;          \
    case YV4_F16: { typedef _Float16 T; if (v8) { constexpr int V = 8; CALL; } else { constexpr int V = 4; CALL; } } break; \
    default: { typedef __bf16 T; if (v8) { constexpr int V = 8; CALL; } else { constexpr int V = 4; CALL; } } break;        \
  }
// (ablation switch, off by default: 8 channels per thread -- 16-byte accesses on 16-bit rows -- measured no faster on the
// forward pass and 20 % SLOWER on the backward apply pass over YOLOv4-L's shapes, tools/bn_bench.py --kernels: the
// passes are bound by bytes in flight per CU, which the extra registers reduce)
static const bool g_bn_vec8 = YV4_ENV_INT("YV4_BN_VEC8", 0) == 1;
// the pipelined 16-bit Mish passes (bn16_*): on / off, channels per thread (4 or 8) and rows per pipeline stage
static const int g_bn16 = YV4_ENV_INT("YV4_BN16", 1);
static const int g_bn16_v = YV4_ENV_INT("YV4_BN16_V", 4);
#ifndef YV4_BN16_U
#define YV4_BN16_U 2
#endif
#define YV4_DISPATCH_H16V(dtype, v8, CALL)                                                                      \
  if ((dtype) == YV4_F16) { typedef _Float16 T; if (v8) { constexpr int V = 8; CALL; } else { constexpr int V = 4; CALL; } } \
  else { typedef __bf16 T; if (v8) { constexpr int V = 8; CALL; } else { constexpr int V = 4; CALL; } }

// phase: 0 = sums + finalize (one rank), 1 = sums only (SyncBN: the caller all-reduces `work`), 2 = sums only, in the
// layout of a conv epilogue's replica 0 (fixed-point words stay words)
static int bn_stats_impl(int dtype, const void* x, int64_t M, int C, int x_cstride, int x_coff, float eps, float momentum,
                         double* work, float* mean, float* invstd, float* running_mean, float* running_var,
                         void* stream, int phase = 0) {
  YV4_REQUIRE(x && work && (phase != 0 || (mean && invstd)) && M > 0 && C > 0, "bn_train_stats: bad argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "bn_train_stats: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(C % 4 == 0 && x_cstride % 4 == 0 && x_coff % 4 == 0, "bn_train_stats: channels must be multiples of 4");
  YV4_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_train_stats: running stats come together");
  YV4_REQUIRE(C <= 4096, "bn_train_stats: more than 4096 channels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int det = deterministic() ? 1 : 0;      // work: [hi (2*C) | lo (2*C)] fixed-point words
  if (det && C > 2048) {                        // 4 C doubles of LDS per workgroup: 64 KB at 2 048 channels
    set_error("bn_train_stats: deterministic mode takes at most 2048 channels (%d given)", C);
    return YV4_E_UNSUPPORTED;
  }
  if (hipMemsetAsync(work, 0, sizeof(double) * (det ? 4 : 2) * C, s) != hipSuccess) { set_error("bn_train_stats: memset failed"); return YV4_E_LAUNCH; }
  const int rpb = bn_rows_per_block(M);
  dim3 grid((unsigned)((M + rpb - 1) / rpb));
  YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(bn_stats_kernel<T>, grid, dim3(256), sizeof(double) * (det ? 4 : 2) * C, s,
                                           reinterpret_cast<const T*>(x), M, C, x_cstride, x_coff, work, rpb, det));
  if (phase == 0)
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 31) / 32), dim3(256), 0, s, work, M, C, eps, momentum, mean, invstd,
                       running_mean, running_var, (const double*)nullptr, det ? 2 : 1, 0, (double*)nullptr, det);
  else if (det && phase == 1)     // the caller (SyncBN) all-reduces doubles
    hipLaunchKernelGGL((fx_decode_kernel<kFxStat, kFxStatFr>), dim3((2 * C + 255) / 256), dim3(256), 0, s, work, 2 * C);
  YV4_CHECK_LAUNCH("bn_train_stats");
  return YV4_OK;
}

static int bn_fwd_impl(int dtype, const void* x, int x_cstride, int x_coff, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, const void* residual, int r_cstride, int r_coff, void* y,
                       int y_cstride, int y_coff, int64_t M, int C, int act, float slope, void* stream) {
  YV4_REQUIRE(x && mean && invstd && gamma && beta && y && M > 0 && C > 0, "bn_act_fwd: bad argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "bn_act_fwd: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(((C | x_cstride | x_coff | y_cstride | y_coff) & 3) == 0, "bn_act_fwd: channels must be multiples of 4");
  YV4_REQUIRE(!residual || ((r_cstride | r_coff) & 3) == 0, "bn_act_fwd: residual channels must be multiples of 4");
  BnArgs a = {};
  a.x = x; a.x_cs = x_cstride; a.x_co = x_coff; a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta;
  a.res = residual; a.r_cs = r_cstride; a.r_co = r_coff; a.y = y; a.y_cs = y_cstride; a.y_co = y_coff;
  a.M = M; a.C = C; a.act = act; a.slope = slope;
  YV4_REQUIRE(C <= 4096, "bn_act_fwd: more than 4096 channels");
  a.rows_per_block = bn_rows_per_block(M);
  const dim3 grid((unsigned)((M + a.rows_per_block - 1) / a.rows_per_block));
  const bool v8 = dtype != YV4_F32 && g_bn_vec8 && ((C | x_cstride | x_coff | y_cstride | y_coff) & 7) == 0 &&
                  (!residual || ((r_cstride | r_coff) & 7) == 0);
  if (dtype != YV4_F32 && act == YV4_ACT_MISH && g_bn16) {
    const bool w8 = g_bn16_v == 8 && ((C | x_cstride | x_coff | y_cstride | y_coff) & 7) == 0 &&
                    (!residual || ((r_cstride | r_coff) & 7) == 0);
    YV4_DISPATCH_H16V(dtype, w8, hipLaunchKernelGGL((bn16_fwd_kernel<T, V, YV4_BN16_U>), grid, dim3(256), 0,
                                                    reinterpret_cast<hipStream_t>(stream), a));
    YV4_CHECK_LAUNCH("bn_act_fwd");
    return YV4_OK;
  }
  YV4_DISPATCH_TV(dtype, v8, hipLaunchKernelGGL((bn_act_fwd_kernel<T, V>), grid, dim3(256), 0,
                                                reinterpret_cast<hipStream_t>(stream), a));
  YV4_CHECK_LAUNCH("bn_act_fwd");
  return YV4_OK;
}

static int bn_bwd_impl(int dtype, const void* x, int x_cstride, int x_coff, const void* dy, int dy_cstride, int dy_coff,
                       const float* mean, const float* invstd, const float* gamma, const float* beta, void* dx,
                       int dx_cstride, int dx_coff, float* dgamma, float* dbeta, double* work, int64_t M, int C, int act,
                       float slope, void* stream, int eval_mode = 0, int phase = 0, int64_t M_total = 0,
                       const double* rows_dev = nullptr, int accumulate = 0, int work_is_zero = 0) {
  // phase 0: reduce + apply; 1: reduce only, dgamma / dbeta published from the LOCAL sums (SyncBN: the caller
  // then all-reduces `work`); 2: apply only, `work` holding the sums over M_total rows
  YV4_REQUIRE(x && dy && mean && invstd && gamma && beta && work && M > 0 && C > 0, "bn_act_bwd: bad argument");
  YV4_REQUIRE(phase == 2 || (dgamma && dbeta), "bn_act_bwd: dgamma / dbeta missing");
  YV4_REQUIRE(phase == 1 || dx, "bn_act_bwd: dx missing");
  YV4_REQUIRE(phase != 2 || rows_dev || M_total >= M, "bn_act_bwd: total row count below the local one");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "bn_act_bwd: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(((C | x_cstride | x_coff | dy_cstride | dy_coff | dx_cstride | dx_coff) & 3) == 0,
              "bn_act_bwd: channels must be multiples of 4");
  YV4_REQUIRE(C <= 4096, "bn_act_bwd: more than 4096 channels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // deterministic mode: `work` is [hi (2*C) | lo (2*C)] fixed-point words between the reduction and the apply pass of
  // ONE call; what leaves the library (phase 1) or enters it (phase 2) is doubles
  const int det = deterministic() && phase != 2 ? 1 : 0;
  if (phase != 2 && !work_is_zero && hipMemsetAsync(work, 0, sizeof(double) * (det ? 4 : 2) * C, s) != hipSuccess) {
    set_error("bn_act_bwd: memset failed");
    return YV4_E_LAUNCH;
  }
  BnArgs a = {};
  a.x = x; a.x_cs = x_cstride; a.x_co = x_coff; a.dy = dy; a.dy_cs = dy_cstride; a.dy_co = dy_coff;
  a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta; a.dx = dx; a.dx_cs = dx_cstride; a.dx_co = dx_coff;
  a.sums = work; a.M = M; a.C = C; a.act = act; a.slope = slope; a.eval_mode = eval_mode;
  a.dgamma = dgamma; a.dbeta = dbeta; a.det = det;
  a.M_total = phase == 2 ? M_total : M;
  a.publish = phase == 0 ? (accumulate ? 2 : 1) : 0;
  a.rows = phase == 2 ? rows_dev : nullptr;
  a.rows_per_block = bn_rows_per_block(M);
  dim3 grid((unsigned)((M + a.rows_per_block - 1) / a.rows_per_block));
  const bool v8 = dtype != YV4_F32 && g_bn_vec8 && ((C | x_cstride | x_coff | dy_cstride | dy_coff | dx_cstride | dx_coff) & 7) == 0;
  const bool b16 = dtype != YV4_F32 && act == YV4_ACT_MISH && g_bn16;
  const bool w8 = g_bn16_v == 8 && ((C | x_cstride | x_coff | dy_cstride | dy_coff | dx_cstride | dx_coff) & 7) == 0;
  if (phase != 2) {
    // channel groups of >= 64 channels (whole 128-byte lines of 16-bit rows), the row blocks shrunk so that the
    // workgroup count stays what bn_rows_per_block aims at
    static const int cg_min = YV4_ENV_INT("YV4_BN_RED_CG", 64);
    int groups = 1;
    if (cg_min > 0 && C % cg_min == 0 && C / cg_min >= 2) groups = C / cg_min < 16 ? C / cg_min : 16;
    while (groups > 1 && (C % groups != 0 || (C / groups) % 8 != 0)) --groups;
    BnArgs r = a;
    r.red_cg = C / groups;
    if (det && r.red_cg > 2048) {                // 4 doubles of LDS per channel of a group: 64 KB at 2 048
      set_error("bn_act_bwd: deterministic mode takes at most 2048 channels per reduction group (%d)", r.red_cg);
      return YV4_E_UNSUPPORTED;
    }
    int64_t rpb = (int64_t)a.rows_per_block * groups;
    if (rpb > g_bn_rows_cap) rpb = g_bn_rows_cap;
    r.rows_per_block = (int)rpb;
    const dim3 rgrid((unsigned)((M + rpb - 1) / rpb), (unsigned)groups);
    if (b16) {
      YV4_DISPATCH_H16V(dtype, w8, hipLaunchKernelGGL((bn16_bwd_reduce_kernel<T, V, YV4_BN16_U>), rgrid, dim3(256),
                                                      sizeof(double) * (det ? 4 : 2) * r.red_cg, s, r));
    } else {
      YV4_DISPATCH_TV(dtype, v8, hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<T, V>), rgrid, dim3(256), sizeof(double) * (det ? 4 : 2) * r.red_cg, s, r));
    }
  }
  if (phase == 1) {
    if (det) hipLaunchKernelGGL(fx_decode_kernel<kFxGrad>, dim3((2 * C + 255) / 256), dim3(256), 0, s, work, 2 * C);
    hipLaunchKernelGGL(sums_to_float_kernel, dim3((C + 255) / 256), dim3(256), 0, s, work, C, dbeta);
    hipLaunchKernelGGL(sums_to_float_kernel, dim3((C + 255) / 256), dim3(256), 0, s, work + C, C, dgamma);
  } else {
    if (b16) {
      YV4_DISPATCH_H16V(dtype, w8, hipLaunchKernelGGL((bn16_bwd_apply_kernel<T, V, YV4_BN16_U>), grid, dim3(256), 0, s, a));
    } else {
      YV4_DISPATCH_TV(dtype, v8, hipLaunchKernelGGL((bn_act_bwd_apply_kernel<T, V>), grid, dim3(256), 0, s, a));
    }
  }
  YV4_CHECK_LAUNCH("bn_act_bwd");
  return YV4_OK;
}

extern "C" int yv4_bn_train_stats(const float* x, int64_t M, int C, int x_cstride, int x_coff, float eps, float momentum,
                                  double* work /* 4*C doubles */, float* mean, float* invstd, float* running_mean,
                                  float* running_var, void* stream) {
  return bn_stats_impl(YV4_F32, x, M, C, x_cstride, x_coff, eps, momentum, work, mean, invstd, running_mean, running_var,
                       stream);
}
extern "C" int yv4_bn_train_stats_h16(const void* x, int dtype, int64_t M, int C, int x_cstride, int x_coff, float eps,
                                      float momentum, double* work, float* mean, float* invstd, float* running_mean,
                                      float* running_var, void* stream) {
  return bn_stats_impl(dtype, x, M, C, x_cstride, x_coff, eps, momentum, work, mean, invstd, running_mean, running_var,
                       stream);
}

extern "C" int yv4_bn_act_fwd(const float* x, int x_cstride, int x_coff, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, const float* residual, int r_cstride, int r_coff,
                              float* y, int y_cstride, int y_coff, int64_t M, int C, int act, float slope, void* stream) {
  return bn_fwd_impl(YV4_F32, x, x_cstride, x_coff, mean, invstd, gamma, beta, residual, r_cstride, r_coff, y, y_cstride,
                     y_coff, M, C, act, slope, stream);
}
extern "C" int yv4_bn_act_fwd_h16(const void* x, int dtype, int x_cstride, int x_coff, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, const void* residual,
                                  int r_cstride, int r_coff, void* y, int y_cstride, int y_coff, int64_t M, int C, int act,
                                  float slope, void* stream) {
  return bn_fwd_impl(dtype, x, x_cstride, x_coff, mean, invstd, gamma, beta, residual, r_cstride, r_coff, y, y_cstride,
                     y_coff, M, C, act, slope, stream);
}

extern "C" int yv4_bn_act_bwd(const float* x, int x_cstride, int x_coff, const float* dy, int dy_cstride, int dy_coff,
                              const float* mean, const float* invstd, const float* gamma, const float* beta,
                              float* dx, int dx_cstride, int dx_coff, float* dgamma, float* dbeta,
                              double* work /* 4*C doubles */, int64_t M, int C, int act, float slope, void* stream) {
  return bn_bwd_impl(YV4_F32, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, dx, dx_cstride,
                     dx_coff, dgamma, dbeta, work, M, C, act, slope, stream);
}
extern "C" int yv4_bn_act_bwd_h16(const void* x, int dtype, int x_cstride, int x_coff, const void* dy, int dy_cstride,
                                  int dy_coff, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, void* dx, int dx_cstride, int dx_coff, float* dgamma, float* dbeta,
                                  double* work, int64_t M, int C, int act, float slope, void* stream) {
  return bn_bwd_impl(dtype, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, dx, dx_cstride,
                     dx_coff, dgamma, dbeta, work, M, C, act, slope, stream);
}

// yv4_conv_fwd_stats' fallback: the sums of y into the first replica (pair) of a cleared statistics buffer, left in the
// form yv4_bn_finalize(replicas = YV4_STATS_REPLICAS) reads
int bn_partial_sums_replica0(const void* x, int dtype, int64_t M, int C, int x_cstride, int x_coff, double* stats,
                             void* stream) {
  return bn_stats_impl(dtype, x, M, C, x_cstride, x_coff, 0.f, 0.f, stats, nullptr, nullptr, nullptr, nullptr, stream, 2);
}

// ---- SyncBN: the same kernels with the cross-rank exchange between their two halves -----------------
extern "C" int yv4_bn_partial_sums(const void* x, int dtype, int64_t M, int C, int x_cstride, int x_coff, double* work,
                                   void* stream) {
  return bn_stats_impl(dtype, x, M, C, x_cstride, x_coff, 0.f, 0.f, work, nullptr, nullptr, nullptr, nullptr, stream, 1);
}
extern "C" int yv4_bn_finalize(double* work, int replicas, int64_t M_total, const double* rows_dev, int C, float eps,
                               float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                               int clear_work, double* zero_after, void* stream) {
  YV4_REQUIRE(work && mean && invstd && (rows_dev || M_total > 0) && C > 0 && replicas >= 1, "bn_finalize: bad argument");
  YV4_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize: running stats come together");
  // replicas == YV4_STATS_REPLICAS: the buffer a conv epilogue filled (yv4_conv_fwd_stats) -- fixed-point replica pairs
  // in deterministic mode; any other count: plain doubles (SyncBN's all-reduced totals)
  const int det = deterministic() && replicas == YV4_STATS_REPLICAS ? 1 : 0;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 31) / 32), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), work,
                     M_total, C, eps, momentum, mean, invstd, running_mean, running_var, rows_dev, replicas, clear_work ? 1 : 0,
                     zero_after, det);
  YV4_CHECK_LAUNCH("bn_finalize");
  return YV4_OK;
}
extern "C" int yv4_conv_stats_fold(double* stats, int C, int clear_stats, double* out, void* stream) {
  YV4_REQUIRE(stats && out && C > 0, "conv_stats_fold: bad argument");
  hipLaunchKernelGGL(stats_fold_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), stats,
                     C, YV4_STATS_REPLICAS, clear_stats ? 1 : 0, out, deterministic() ? 1 : 0);
  YV4_CHECK_LAUNCH("conv_stats_fold");
  return YV4_OK;
}
extern "C" int yv4_bn_act_bwd_sums(const void* x, int dtype, int x_cstride, int x_coff, const void* dy, int dy_cstride,
                                   int dy_coff, const float* mean, const float* invstd, const float* gamma,
                                   const float* beta, float* dgamma, float* dbeta, double* work, int64_t M, int C,
                                   int act, float slope, void* stream) {
  return bn_bwd_impl(dtype, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, nullptr, 4, 0,
                     dgamma, dbeta, work, M, C, act, slope, stream, 0, 1);
}
extern "C" int yv4_bn_act_bwd_apply(const void* x, int dtype, int x_cstride, int x_coff, const void* dy, int dy_cstride,
                                    int dy_coff, const float* mean, const float* invstd, const float* gamma,
                                    const float* beta, void* dx, int dx_cstride, int dx_coff, const double* work,
                                    int64_t M, int64_t M_total, const double* rows_dev, int C, int act, float slope,
                                    void* stream) {
  return bn_bwd_impl(dtype, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, dx, dx_cstride,
                     dx_coff, nullptr, nullptr, const_cast<double*>(work), M, C, act, slope, stream, 0, 2, M_total,
                     rows_dev);
}

// As yv4_bn_act_bwd_h16 / yv4_bn_eval_act_bwd, but dgamma / dbeta are ADDED to (the parameters' own .grad: no temporary,
// no accumulation kernel afterwards)
extern "C" int yv4_bn_act_bwd_accum(const void* x, int dtype, int x_cstride, int x_coff, const void* dy, int dy_cstride,
                                    int dy_coff, const float* mean, const float* invstd, const float* gamma,
                                    const float* beta, void* dx, int dx_cstride, int dx_coff, float* dgamma, float* dbeta,
                                    double* work, int64_t M, int C, int act, float slope, int flags, void* stream) {
  // flags: bit 0 = eval-mode BN, bit 1 = `work` is already zero (yv4_bn_finalize's zero_after cleared it)
  return bn_bwd_impl(dtype, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, dx, dx_cstride,
                     dx_coff, dgamma, dbeta, work, M, C, act, slope, stream, flags & 1, 0, 0, nullptr, 1, (flags >> 1) & 1);
}

extern "C" int yv4_bn_eval_act_bwd(const void* x, int dtype, int x_cstride, int x_coff, const void* dy, int dy_cstride,
                                   int dy_coff, const float* mean, const float* invstd, const float* gamma,
                                   const float* beta, void* dx, int dx_cstride, int dx_coff, float* dgamma, float* dbeta,
                                   double* work, int64_t M, int C, int act, float slope, void* stream) {
  return bn_bwd_impl(dtype, x, x_cstride, x_coff, dy, dy_cstride, dy_coff, mean, invstd, gamma, beta, dx, dx_cstride,
                     dx_coff, dgamma, dbeta, work, M, C, act, slope, stream, 1);
}
