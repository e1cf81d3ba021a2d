// fp32 stem: 3x3 / stride 1 / pad 1 convolution of the 3-channel image (stored NHWC with C padded to
// 4), Cout <= 64.  K = 9 taps x 4 channels = 36 is too shallow for the LDS-staged kernels (they
// spend their time in prologue/epilogue) and the layer is bound by its own OUTPUT
// (N*H*W*Cout*4 B = 1.5 GB at batch 32, 608^2, Cout 32), so this kernel keeps everything in
// registers: a wave owns 32 consecutive pixels of one image row x 32 output channels
// (one 32x32 MFMA tile), fetches its 9 x 8-byte input taps straight into the MFMA A operand
// (lane (r,h): pixel r, channels 2h,2h+1 of each tap; out-of-image taps come back as zeros from
// the buffer descriptor), holds the 18 weight values it needs for the whole kernel, issues
// 18 MFMAs per tile and streams the epilogue to HBM in 128-byte rows.
#include "conv_f32_common.h"
#include "conv_desc.h"

namespace yv4 {

// one value to y[row_base + lane_off]: row_base (elements) is wave-uniform, lane_off a 32-bit per-lane constant
template <int OUT>
__device__ __forceinline__ void stem_store(float* y, long long row_base, unsigned lane_off, float v) {
  if (OUT == 0) (y + row_base)[lane_off] = v;
  else if (OUT == 1) (reinterpret_cast<_Float16*>(y) + row_base)[lane_off] = (_Float16)v;
  else (reinterpret_cast<__bf16*>(y) + row_base)[lane_off] = (__bf16)v;
}

// OUT: 0 fp32 (p.y), 1 fp16, 2 bf16 (p.y reinterpreted; the 16-bit inference path keeps the image
// and this layer's arithmetic in fp32 and only rounds the layer's output).
template <int TN, int OUT>
__global__ __launch_bounds__(kThreads) void conv_stem3x3_kernel(ConvArgs p, unsigned x_bytes, int tiles_w, long long ntiles) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int r = lane & 31;
  const int h = lane >> 5;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, x_bytes, 0x00020000);
  constexpr unsigned kOOB = 0xFFFFFFF0u;

  // weights: B[k][cout r] with k = (tap, ci = 2h + j)
  float wv[TN][9][2];
  float s1[TN], t1[TN];
#pragma unroll
  for (int jn = 0; jn < TN; ++jn) {
    const int co = jn * 32 + r;
    const bool cok = co < p.Cout;
    s1[jn] = cok ? p.s1[co] : 0.f;
    t1[jn] = cok ? p.t1[co] : 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int j = 0; j < 2; ++j) wv[jn][tap][j] = cok ? p.w[(size_t)co * p.Kw + tap * 4 + 2 * h + j] : 0.f;
  }

  // tile walk in wave-uniform 32-bit arithmetic with magic-number divisors (the 64-bit per-lane divides of the
  // first version were a third of the instructions of a tile)
  // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2: XCD c walks the c-th eighth of the tile
  // list with all its waves side by side, so the rows a tile shares with the tiles above and below it (3 input rows
  // per output row) are fetched by one L2 once instead of by three (measured 3.4x the input before, FETCH_SIZE).
  const int nblk_all = (int)gridDim.x;
  const int nch = nblk_all < 8 ? nblk_all : 8;
  const int chunk = (int)blockIdx.x % nch, local = (int)blockIdx.x / nch;
  const int nblk = (nblk_all - chunk + nch - 1) / nch;               // workgroups walking this chunk
  const int cq = (int)ntiles / nch, crem = (int)ntiles % nch;
  const int t_lo = chunk * cq + (chunk < crem ? chunk : crem);
  const int t_hi = t_lo + cq + (chunk < crem ? 1 : 0);
  const int wave_id = __builtin_amdgcn_readfirstlane(local * 4 + (tid >> 6));
  const int nwaves = nblk * 4;
  for (int t = t_lo + wave_id; t < t_hi; t += nwaves) {
    const long long ty = fd_div(t, p.fd_wo);     // n*H + y   (fd_wo: tiles per row, fd_hw: H -- set by launch_conv_stem)
    const int tx = t - (int)ty * tiles_w;
    const int y = (int)ty - fd_div((int)ty, p.fd_hw) * p.H;
    const int x = tx * 32 + r;
    // byte offset of x[n, y, x, x_co + 2h]
    const unsigned base = (unsigned)(((ty * p.W + x) * p.x_cs + p.x_co + 2 * h) * 4);
    u32x2 a[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const bool rok = (unsigned)(y + kh - 1) < (unsigned)p.H;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const bool ok = rok && (unsigned)(x + kw - 1) < (unsigned)p.W;
        const unsigned off = base + (unsigned)((((kh - 1) * p.W + (kw - 1)) * p.x_cs) * 4);
        a[kh * 3 + kw] = __builtin_amdgcn_raw_buffer_load_b64(rsA, ok ? off : kOOB, 0, 0);
      }
    }
    f32x16 acc[TN];
#pragma unroll
    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[jn][e] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        acc[jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[tap].x), wv[jn][tap][0], acc[jn], 0, 0, 0);
        acc[jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[tap].y), wv[jn][tap][1], acc[jn], 0, 0, 0);
      }
    // epilogue: lane (r, h) holds channel jn*32 + r of the tile's pixels (e&3) + 8*(e>>2) + 4h.  The row address is
    // wave-uniform (scalar base + one per-lane offset that never changes), the activation sits behind one uniform
    // switch and the bounds test is per tile: the per-element form of all three cost 2.7x the 18 MFMAs in VALU time.
    const long long mrow = ty * p.W + tx * 32;
    const bool full = tx * 32 + 32 <= p.W;
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      if (jn * 32 + r >= p.Cout) continue;
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = acc[jn][e] * s1[jn] + t1[jn];
      act_row16(v, p.act1, p.slope1);
      const unsigned lane_off = (unsigned)(4 * h * p.y_cs + jn * 32 + r);
      if (full) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          stem_store<OUT>(p.y, (mrow + (e & 3) + 8 * (e >> 2)) * p.y_cs + p.y_co, lane_off, v[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (tx * 32 + (e & 3) + 8 * (e >> 2) + 4 * h < p.W)
            stem_store<OUT>(p.y, (mrow + (e & 3) + 8 * (e >> 2)) * p.y_cs + p.y_co, lane_off, v[e]);
      }
    }
  }
}

template <int OUT>
static int launch_conv_stem(const ConvArgs& a, hipStream_t stream) {
  const long long xb = x_bytes(a);
  if (!desc_addressable(xb)) {
    set_error("conv stem: input of 4 GiB or more is not addressable through a buffer descriptor");
    return YV4_E_UNSUPPORTED;
  }
  const int tiles_w = (a.W + 31) / 32;
  const long long ntiles = (long long)a.N * a.H * tiles_w;
  if (ntiles >= (1LL << 31)) {
    set_error("conv stem: %lld tiles do not fit 31 bits", ntiles);
    return YV4_E_UNSUPPORTED;
  }
  long long blocks = (ntiles + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;   // 8 workgroups per CU, grid-stride over the tiles
  ConvArgs p = a;
  p.fd_wo = make_fastdiv((unsigned)tiles_w);   // the stem kernel's tile walk: t / tiles_w, (n*H + y) / H
  p.fd_hw = make_fastdiv((unsigned)a.H);
  if (a.Cout <= 32)
    hipLaunchKernelGGL((conv_stem3x3_kernel<1, OUT>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, (unsigned)xb,
                       tiles_w, ntiles);
  else
    hipLaunchKernelGGL((conv_stem3x3_kernel<2, OUT>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, (unsigned)xb,
                       tiles_w, ntiles);
  YV4_CHECK_LAUNCH("conv_stem3x3");
  return YV4_OK;
}

bool stem_ok(const ConvArgs& a) {
  return a.Cin == 4 && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.Cout <= 64 && a.res == nullptr &&
         a.s2 == nullptr && a.x_co % 2 == 0 && desc_addressable(x_bytes(a));
}

int conv_stem_f32_launch(const ConvArgs& a, int out_dtype, hipStream_t s) {
  if (out_dtype == YV4_F16) return launch_conv_stem<1>(a, s);
  if (out_dtype == YV4_BF16) return launch_conv_stem<2>(a, s);
  return launch_conv_stem<0>(a, s);
}

}  // namespace yv4

using namespace yv4;

// The stem of the 16-bit path: fp32 image (NHWC, C padded to 4) and fp32 weights in, fp32 MFMA,
// output rounded to fp16 / bf16 (the layer is bound by its output bytes, which this halves).
extern "C" int yv4_conv_stem_fwd(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1,
                                 const float* shift1, void* y, int out_dtype, void* stream) {
  YV4_REQUIRE(d && x && w && scale1 && shift1 && y, "conv stem: null argument");
  YV4_REQUIRE(out_dtype == YV4_F32 || out_dtype == YV4_F16 || out_dtype == YV4_BF16, "conv stem: bad out_dtype");
  ConvDescRules rules{1};      // (alignment is part of the shape rule below, with which the geometry check says Ho/Wo == H/W)
  rules.acts = 1;
  if (int rc = check_conv_desc(d, "conv stem", rules)) return rc;
  const ConvArgs a = conv_args(d, x, w, scale1, shift1, nullptr, nullptr, nullptr, reinterpret_cast<float*>(y));
  YV4_REQUIRE(stem_ok(a), "conv stem: needs Cin 4 (3 padded), 3x3, stride 1, pad 1, Cout <= 64");
  return conv_stem_f32_launch(a, out_dtype, reinterpret_cast<hipStream_t>(stream));
}
