// Backward halves of elementwise.hip's data-movement ops on gfx950: zero-dilation (the data gradient of a stride-2
// convolution), SPP max-pool backward and nearest-resample backward.
#include "train_common.h"

namespace yv4 {

// ---------------------------------------------------------------------------------
// dst[n, 2y, 2x, c] = src[n, y, x, c], everything else 0  (dst is (N, 2H, 2W, C) dense NHWC).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dilate2_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int H,
                                                      int W, int C4, int src_cs, int src_co) {
  const size_t total = (size_t)N * 2 * H * 2 * W * C4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % C4);
    size_t t = i / C4;
    const int x = (int)(t % (2 * W));
    t /= 2 * W;
    const int y = (int)(t % (2 * H));
    const int n = (int)(t / (2 * H));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (((x | y) & 1) == 0)
      v = *reinterpret_cast<const float4*>(src + ((size_t)(n * H + (y >> 1)) * W + (x >> 1)) * src_cs + src_co + c4 * 4);
    reinterpret_cast<float4*>(dst)[i] = v;
  }
}
// ---------------------------------------------------------------------------------
// SPP backward (darknetcsp.py:176-181,203-206,222-226: cat([x, mp5(x), mp9(x), mp13(x)])):
//   dx[p] = dcat[0][p] + sum over k in {5,9,13}, over output positions q whose window argmax is p,
//   of dcat[k][q].
// One thread owns (n, y, x, 4 channels) as an OUTPUT position: it rescans the 13x13 window of the
// saved input once in row-major order, tracking the first maximum of the nested 5 / 9 / 13 windows
// (torch's max_pool2d keeps the first maximum in scan order), and scatters its three gradients with
// float atomics into the fp32 accumulator dx (N, H, W, C dense, zero on entry), plus its own
// identity-branch gradient.  Replaces three ATen max_pool2d backward passes + three adds.
// ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void spp_pool_bwd_kernel(const T* __restrict__ xcat, int x_cs, int x_co,
                                                           const T* __restrict__ dcat, int d_cs, int d_co,
                                                           float* __restrict__ dx, int N, int H, int W, int C) {
  const int C4 = C >> 2;
  const size_t total = (size_t)N * H * W * C4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float ninf = -__builtin_huge_valf();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % C4);
    size_t t = i / C4;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const int n = (int)(t / H);
    const T* base = xcat + (size_t)n * H * W * x_cs + x_co + c4 * 4;
    float m[3][4];
    int am[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int u = 0; u < 4; ++u) { m[k][u] = ninf; am[k][u] = y * W + x; }
    for (int dy = -6; dy <= 6; ++dy) {
      const int yy = y + dy;
      if ((unsigned)yy >= (unsigned)H) continue;
      const int ady = dy < 0 ? -dy : dy;
      for (int dxx = -6; dxx <= 6; ++dxx) {
        const int xx = x + dxx;
        if ((unsigned)xx >= (unsigned)W) continue;
        const int adx = dxx < 0 ? -dxx : dxx;
        const int rad = ady > adx ? ady : adx;
        const float4 v4 = El<T>::ld4(base + ((size_t)yy * W + xx) * x_cs);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        const int pos = yy * W + xx;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (v[u] > m[2][u]) { m[2][u] = v[u]; am[2][u] = pos; }
          if (rad <= 4 && v[u] > m[1][u]) { m[1][u] = v[u]; am[1][u] = pos; }
          if (rad <= 2 && v[u] > m[0][u]) { m[0][u] = v[u]; am[0][u] = pos; }
        }
      }
    }
    const T* g = dcat + ((size_t)(n * H + y) * W + x) * d_cs + d_co + c4 * 4;
    float* dxn = dx + (size_t)n * H * W * C + c4 * 4;
    const float4 g0 = El<T>::ld4(g);
    const float gi[4] = {g0.x, g0.y, g0.z, g0.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) atomicAdd(dxn + (size_t)(y * W + x) * C + u, gi[u]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 gk = El<T>::ld4(g + (k + 1) * C);
      const float gv[4] = {gk.x, gk.y, gk.z, gk.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(dxn + (size_t)am[k][u] * C + u, gv[u]);
    }
  }
}

// The same scatter for the maps an SPP block actually sees (19x19 at 608 px): everything in LDS, and the window
// argmax found by CASCADED 5x5 pools instead of a 13x13 scan per pixel.
//   * Every element becomes a KEY: (order-preserving bits of the value) : (all-ones - position).  The maximum key of a
//     window is its largest value and, among equal values, the smallest position -- the first hit of the row-major scan
//     `v > best` that torch's pooling (and the kernel above) performs.  Keys make the argmax a plain associative,
//     idempotent max, so pool9 = pool5 o pool5 and pool13 = pool5 o pool9 exactly (windows clipped at the border), and
//     each 5x5 pool separates into a row pass and a column pass: 30 LDS reads per element for the three pools instead
//     of 169 global loads and 507 compare/select pairs (the round-2 form: 0.99 ms at batch 64 x 512 channels).
//   * one workgroup = one image x CG channels (8 for 16-bit keys, 4 for 64-bit keys of fp32 values): three key planes (in, row-pass, out -- rotated through the cascade)
//     and the fp32 accumulator plane, H*W x CG each; the three pool gradients go to the accumulator by LDS atomics,
//     the identity branch by a plain add, and dx is written once.
template <typename T> struct SppKey;
template <> struct SppKey<float> {
  typedef unsigned long long K;
  static constexpr int CG = 4;
  static __device__ __forceinline__ K make(float v, int pos) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;                                     // -0 == +0 for `>`
    b ^= (b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u;
    return ((K)b << 32) | (K)(0xFFFFFFFFu - (unsigned)pos);
  }
  static __device__ __forceinline__ int pos(K k) { return (int)(0xFFFFFFFFu - (unsigned)k); }
};
template <typename T> struct SppKey {                                 // _Float16 / __bf16
  typedef unsigned K;
  static constexpr int CG = 8;
  static __device__ __forceinline__ K make(T v, int pos) {
    unsigned b = (unsigned)__builtin_bit_cast(unsigned short, v);
    if (b == 0x8000u) b = 0u;
    b ^= (b & 0x8000u) ? 0xFFFFu : 0x8000u;
    return (b << 16) | (0xFFFFu - (unsigned)pos);
  }
  static __device__ __forceinline__ int pos(K k) { return (int)(0xFFFFu - (k & 0xFFFFu)); }
};

constexpr int kSppItems = 16;      // (position, channel) items per thread: H*W*CG <= 4096 (the 64 KB LDS bound of the launch)
template <typename T>
__global__ __launch_bounds__(256) void spp_pool_bwd_lds_kernel(const T* __restrict__ xcat, int x_cs, int x_co,
                                                               const T* __restrict__ dcat, int d_cs, int d_co,
                                                               float* __restrict__ dx, int H, int W, int C, int det) {
  // det (yv4_set_deterministic): the accumulator plane holds 64-bit FIXED-POINT integers with one exponent for the
  // workgroup -- 2^40 / (the power of two above the largest |gradient| it will add, found by an integer max) -- so the
  // scatter's atomics are integer adds and the plane's value does not depend on their order.  A non-finite gradient
  // anywhere in the block makes the block's outputs NaN (the step is skipped by the loss scaler either way).
  typedef SppKey<T> SK;
  typedef typename SK::K K;
  constexpr int CG = SK::CG;
  extern __shared__ __attribute__((aligned(16))) unsigned char spp_raw[];
  const int HW = H * W;
  K* ka = reinterpret_cast<K*>(spp_raw);             // [HW][CG]
  K* kb = ka + (size_t)HW * CG;
  K* kc = kb + (size_t)HW * CG;
  float* acc = reinterpret_cast<float*>(kc + (size_t)HW * CG);
  long long* acc64 = reinterpret_cast<long long*>(acc);
  __shared__ unsigned smax;
  if (det && threadIdx.x == 0) smax = 0u;
  if (det) __syncthreads();
  unsigned gmax = 0u;
  const int n = blockIdx.y;
  const int cg0 = blockIdx.x * CG;
  const int nc = min(CG, C - cg0);
  const int items = HW * CG;
  const T* xb = xcat + (size_t)n * HW * x_cs + x_co + cg0;
  const T* gb = dcat + (size_t)n * HW * d_cs + d_co + cg0;
  const FastDiv fd_w = make_fastdiv((unsigned)W);
  // a thread keeps the same items (i = tid + 256 j) through every pass: their coordinates and their three pool gradients
  // are fetched once, all loads in flight together
  float g[3][kSppItems];
  float gid0[kSppItems];           // (deterministic mode only)
  short iy[kSppItems], ix[kSppItems];
#pragma unroll
  for (int j = 0; j < kSppItems; ++j) {
    const int i = threadIdx.x + 256 * j;
    const int pos = i / CG, c = i - pos * CG;
    const int y = fd_div(pos, fd_w);
    iy[j] = (short)y;
    ix[j] = (short)(pos - y * W);
    const bool ok = i < items && c < nc;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g[k][j] = ok ? (float)gb[(size_t)pos * d_cs + (size_t)(k + 1) * C + c] : 0.f;
      gmax = max(gmax, __float_as_uint(g[k][j]) & 0x7fffffffu);
    }
    if (i < items) {
      ka[i] = ok ? SK::make(xb[(size_t)pos * x_cs + c], pos) : (K)0;
      const float gid = ok ? (float)gb[(size_t)pos * d_cs + c] : 0.f;     // the identity branch's gradient
      if (det) { gid0[j] = gid; gmax = max(gmax, __float_as_uint(gid) & 0x7fffffffu); }
      else acc[i] = gid;
    }
  }
  double fx_scale = 1.0;
  bool fx_bad = false;
  if (det) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = max(gmax, (unsigned)__shfl_xor((int)gmax, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&smax, gmax);
    __syncthreads();
    const unsigned mb = smax;
    fx_bad = mb >= 0x7f800000u;
    fx_scale = __builtin_ldexp(1.0, 166 - (int)(mb >> 23));      // |g| < 2^(e - 126)  ->  |g * scale| < 2^40
#pragma unroll
    for (int j = 0; j < kSppItems; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < items) acc64[i] = fx_bad ? 0ll : (long long)__builtin_rint((double)gid0[j] * fx_scale);
    }
  }
  __syncthreads();
  K* src = ka; K* tmp = kb; K* out = kc;
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
    // row pass: tmp(y, x) = max src(y, x-2 .. x+2)
#pragma unroll
    for (int j = 0; j < kSppItems; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < items) {
        const int c = i & (CG - 1), y = iy[j], x = ix[j];
        const K* row = src + (size_t)y * W * CG + c;
        K m = row[x * CG];
#pragma unroll
        for (int d = -2; d <= 2; ++d) {
          if (d == 0) continue;
          const int xx = min(max(x + d, 0), W - 1);              // a clamped neighbour repeats an element of the window
          const K v = row[xx * CG];
          m = v > m ? v : m;
        }
        tmp[i] = m;
      }
    }
    __syncthreads();
    // column pass + scatter of this pool's gradient to its argmax
#pragma unroll
    for (int j = 0; j < kSppItems; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < items) {
        const int c = i & (CG - 1), y = iy[j], x = ix[j];
        const K* col = tmp + (size_t)x * CG + c;
        K m = col[(size_t)y * W * CG];
#pragma unroll
        for (int d = -2; d <= 2; ++d) {
          if (d == 0) continue;
          const int yy = min(max(y + d, 0), H - 1);
          const K v = col[(size_t)yy * W * CG];
          m = v > m ? v : m;
        }
        out[i] = m;
        const float gv = k == 0 ? g[0][j] : (k == 1 ? g[1][j] : g[2][j]);
        if (c < nc) {
          if (det) {
            if (!fx_bad) atomicAdd(reinterpret_cast<u64_t*>(&acc64[SK::pos(m) * CG + c]), (u64_t)(long long)__builtin_rint((double)gv * fx_scale));
          } else {
            atomicAdd(&acc[SK::pos(m) * CG + c], gv);
          }
        }
      }
    }
    __syncthreads();
    K* t = src; src = out; out = t;                  // the pooled keys feed the next 5x5 pool
  }
  float* o = dx + (size_t)n * HW * C + cg0;
#pragma unroll
  for (int j = 0; j < kSppItems; ++j) {
    const int i = threadIdx.x + 256 * j;
    if (i < items) {
      const int pos = i / CG, c = i - pos * CG;
      if (c < nc) o[(size_t)pos * C + c] = !det ? acc[i] : (fx_bad ? __builtin_nanf("") : (float)((double)acc64[i] / fx_scale));
    }
  }
}

// Backward of the nearest resample by an INTEGER factor (yolo_neck_csp.py:213-219: F.interpolate(scale 2) into the concat
// buffer): dx[n, sy, sx, c] = the sum of the fy x fx gradient pixels that read it, fp32 sum, one rounding.  The gradient is a
// channel slice of the concat buffer's gradient (dy_cs / dy_co).
template <typename T>
__global__ __launch_bounds__(256) void resample_nearest_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int Hs,
                                                                   int Ws, int fy, int fx, int C4, int dy_cs, int dy_co) {
  const size_t total = (size_t)N * Hs * Ws * C4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int Wd = Ws * fx, Hd = Hs * fy;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % C4);
    size_t t = i / C4;
    const int sx = (int)(t % Ws);
    t /= Ws;
    const int sy = (int)(t % Hs);
    const int n = (int)(t / Hs);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < fy; ++j)
      for (int k = 0; k < fx; ++k) {
        const float4 v = El<T>::ld4(dy + ((size_t)(n * Hd + sy * fy + j) * Wd + sx * fx + k) * dy_cs + dy_co + c4 * 4);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
    El<T>::st4(dx + i * 4, a);
  }
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_dilate2_fwd(const float* src, float* dst, int N, int H, int W, int C, int src_cstride, int src_coff,
                               void* stream) {
  YV4_REQUIRE(src && dst && N > 0 && H > 0 && W > 0 && C > 0, "dilate2: bad argument");
  YV4_REQUIRE(C % 4 == 0 && src_cstride % 4 == 0 && src_coff % 4 == 0, "dilate2: channels must be multiples of 4");
  const size_t total = (size_t)N * 2 * H * 2 * W * (C / 4);
  hipLaunchKernelGGL(dilate2_kernel, dim3(ew_grid_t(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, dst,
                     N, H, W, C / 4, src_cstride, src_coff);
  YV4_CHECK_LAUNCH("dilate2");
  return YV4_OK;
}

extern "C" int yv4_spp_pool_bwd(const void* xcat, int x_cstride, int x_coff, const void* dcat, int d_cstride, int d_coff,
                                float* dx, int N, int H, int W, int C, int dtype, void* stream) {
  YV4_REQUIRE(xcat && dcat && dx && N > 0 && H > 0 && W > 0 && C > 0, "spp_pool_bwd: bad argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "spp_pool_bwd: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(((C | x_cstride | x_coff | d_cstride | d_coff) & 3) == 0, "spp_pool_bwd: channels must be multiples of 4");
  YV4_REQUIRE(x_coff + C <= x_cstride && d_coff + 4 * C <= d_cstride, "spp_pool_bwd: view exceeds its pixel stride");
  YV4_REQUIRE((long long)H * W < (1LL << 31), "spp_pool_bwd: H*W does not fit 31 bits");
  const bool f32 = dtype == YV4_F32;
  const int cg = f32 ? SppKey<float>::CG : SppKey<__bf16>::CG;
  const int det = deterministic() ? 1 : 0;
  const size_t lds = (size_t)H * W * cg * (3 * (f32 ? 8 : 4) + (det ? 8 : 4));
  if (lds <= 64 * 1024 && N <= 65535 && (long long)H * W * cg <= 256 * kSppItems) {   // small maps: keys and accumulator LDS-resident
    dim3 grid((unsigned)((C + cg - 1) / cg), (unsigned)N);
    YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(spp_pool_bwd_lds_kernel<T>, grid, dim3(256), lds,
                                             reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(xcat),
                                             x_cstride, x_coff, reinterpret_cast<const T*>(dcat), d_cstride, d_coff, dx, H,
                                             W, C, det));
    YV4_CHECK_LAUNCH("spp_pool_bwd");
    return YV4_OK;
  }
  if (det) {
    set_error("spp_pool_bwd: deterministic mode needs the LDS-resident form (H*W*%d <= %d, got %dx%d): the large-map "
              "kernel scatters with float atomics", cg, 256 * kSppItems, H, W);
    return YV4_E_UNSUPPORTED;
  }
  const size_t total = (size_t)N * H * W * (C / 4);
  YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(spp_pool_bwd_kernel<T>, dim3(ew_grid_t(total)), dim3(256), 0,
                                           reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(xcat),
                                           x_cstride, x_coff, reinterpret_cast<const T*>(dcat), d_cstride, d_coff, dx, N,
                                           H, W, C));
  YV4_CHECK_LAUNCH("spp_pool_bwd");
  return YV4_OK;
}


extern "C" int yv4_resample_nearest_bwd(const void* dy, void* dx, int N, int Hs, int Ws, int Hd, int Wd, int C, int dy_cstride,
                                        int dy_coff, int dtype, void* stream) {
  YV4_REQUIRE(dy && dx && N > 0 && Hs > 0 && Ws > 0 && C > 0, "resample_bwd: bad argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "resample_bwd: dtype must be f32, f16 or bf16");
  YV4_REQUIRE(Hd % Hs == 0 && Wd % Ws == 0 && Hd / Hs <= 8 && Wd / Ws <= 8, "resample_bwd: integer scale factors up to 8 only");
  YV4_REQUIRE(((C | dy_cstride | dy_coff) & 3) == 0 && dy_coff >= 0 && dy_coff + C <= dy_cstride,
              "resample_bwd: channels must be multiples of 4 and the view inside its pixel stride");
  const size_t total = (size_t)N * Hs * Ws * (C / 4);
  YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(resample_nearest_bwd_kernel<T>, dim3(ew_grid_t(total)), dim3(256), 0,
                                           reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(dy),
                                           reinterpret_cast<T*>(dx), N, Hs, Ws, Hd / Hs, Wd / Ws, C / 4, dy_cstride, dy_coff));
  YV4_CHECK_LAUNCH("resample_nearest_bwd");
  return YV4_OK;
}
