// Conv weight -> the convolution kernels' packed operands on gfx950: one weight per launch (yv4_pack_weight) and a
// table of weights in one launch (yv4_pack_weights_multi).
#include "train_common.h"

namespace yv4 {

// Conv weight -> the kernels' packed operand in ONE pass (cast included): rows x (KHo*KWo*ICp) with K ordered
// (kh, kw, channel), zero-padded channels; output tap (kh, kw) reads source tap (kh0 + kh*kh_step, kw0 + kw*kw_step).
// transpose = 0: rows = Cout, channel = Cin (forward operand); 1: rows = Cin, channel = Cout -- with the taps
// mirrored (kh0 = KH-1, step -1) the operand of the data gradient (ATen needs flip + transpose + contiguous + cast = 3
// launches per conv per step for it), with a tap subset the operand of one parity class of a stride-2 data gradient
// (list-indexing the taps cost two host-to-device index uploads and two gather kernels per class).  The source is addressed through its element strides,
// so contiguous and channels_last parameters both go without a copy.
template <typename T>
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, long long s_co, long long s_ci,
                                                          long long s_kh, long long s_kw, int Cout, int Cin, int KHo, int KWo,
                                                          int kh0, int kh_step, int kw0, int kw_step, int tf, int ICp,
                                                          T* __restrict__ dst, int nrows) {
  // one output row (r, kh, kw) of ICp channels per workgroup iteration: two small divides per row, none per element
  const int IC = tf ? Cout : Cin;
  const int taps = KHo * KWo;
  for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
    const int r = row / taps;
    const int tap = row - r * taps;
    const int kh = tap / KWo, kw = tap - kh * KWo;
    const float* src = w + (kh0 + kh * kh_step) * s_kh + (kw0 + kw * kw_step) * s_kw + (tf ? r * s_ci : r * s_co);
    const long long s_ic = tf ? s_co : s_ci;
    T* d = dst + (size_t)row * ICp;
    for (int ic = threadIdx.x; ic < ICp; ic += 256) d[ic] = (T)(ic < IC ? src[ic * s_ic] : 0.f);
  }
}

// The same pass over a TABLE of weights in one launch (yv4_pack_weights_multi): workgroup b serves the descriptor whose
// [first_block, first_block + nblocks) range holds b, rows_per_block output rows of it.
//
// An output row (r, kh, kw) runs over the channel ic; in the SOURCE (an fp32 (Cout, Cin, KH, KW) parameter, normally
// contiguous) the element sits at r*s_r + ic*s_ic + tap offset, and whichever of the forward operand (s_ic = KH*KW) and
// the data-gradient operand (s_ic = Cin*KH*KW) is packed, neighbouring ic are 36 bytes or kilobytes apart: reading row
// by row (round 2) moved 4 bytes per 64- or 128-byte line touched and took 0.87 ms per YOLOv4-L step (64 M parameters,
// both operands).  Here a workgroup stages a box of the source -- NR rows r x ICc channels x every tap the descriptor
// uses -- in LDS, walking the source in ITS order (taps fastest, then whichever of r / ic has the smaller stride), and
// writes the output rows from LDS with the channel across lanes.
constexpr int kPackStage = 9216;       // floats staged per pass (36 KB)

template <typename T>
__device__ __forceinline__ void pack_rows(const yv4_pack_desc& d, int row0, int row1, float* stage) {
  const int tf = d.transpose;
  const int IC = tf ? d.Cout : d.Cin;
  const int ICp = (IC + d.pad_to - 1) / d.pad_to * d.pad_to;
  const int taps = d.KHo * d.KWo;
  const long long s_ic = tf ? d.s_co : d.s_ci, s_r = tf ? d.s_ci : d.s_co;
  T* dst = reinterpret_cast<T*>(d.dst);
  // bounding box of the source taps the descriptor reads
  const int khl = d.kh0 + (d.KHo - 1) * d.kh_step, kwl = d.kw0 + (d.KWo - 1) * d.kw_step;
  const int khmin = min(d.kh0, khl), kwmin = min(d.kw0, kwl);
  const int nbh = abs(khl - d.kh0) + 1, nbw = abs(kwl - d.kw0) + 1;
  const int TB = nbh * nbw, TBs = TB | 1;                    // odd LDS pitch per (r, ic): channel-strided reads hit all banks
  const int rA = row0 / taps, rB = (row1 - 1) / taps;        // rows r touched (inclusive)
  const bool ic_inner = s_ic <= s_r;
  int NR, ICc;
  if (ic_inner) {
    if (ICp * TBs <= kPackStage) { ICc = ICp; NR = min(rB - rA + 1, kPackStage / (ICp * TBs)); }
    else { NR = 1; ICc = (kPackStage / TBs) & ~7; }
  } else {
    NR = min(rB - rA + 1, max(8, 64 / TB));                  // >= 256 contiguous source bytes per ic
    ICc = min(ICp, (kPackStage / (NR * TBs)) & ~7);
  }
  constexpr int VEC = sizeof(T) == 2 ? 2 : 1;                // 16-bit outputs are stored in pairs
  const FastDiv fd_tb = make_fastdiv((unsigned)TB), fd_bw = make_fastdiv((unsigned)nbw), fd_kwo = make_fastdiv((unsigned)d.KWo),
                fd_taps = make_fastdiv((unsigned)taps);
  const int tid = threadIdx.x;
  for (int r0 = rA; r0 <= rB; r0 += NR) {
    const int nr = min(NR, rB - r0 + 1);
    const FastDiv fd_nr = make_fastdiv((unsigned)nr);
    const int orow0 = max(row0, r0 * taps), orow1 = min(row1, (r0 + nr) * taps);
    for (int c0 = 0; c0 < ICp; c0 += ICc) {
      const int cn = min(ICc, ICp - c0);
      const FastDiv fd_cn = make_fastdiv((unsigned)cn);
      __syncthreads();                                       // the previous pass has been written out
      const int total = nr * cn * TB;
      // eight independent loads in flight per thread (the staging is latency-bound otherwise)
      for (int e0 = tid; e0 < total; e0 += 256 * 8) {
        float v[8];
        int li[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = e0 + 256 * u;
          v[u] = 0.f;
          li[u] = -1;
          if (e < total) {
            const int q = fd_div(e, fd_tb), t = e - q * TB;
            int rl, cl;
            if (ic_inner) { rl = fd_div(q, fd_cn); cl = q - rl * cn; }
            else { cl = fd_div(q, fd_nr); rl = q - cl * nr; }
            const int bh = fd_div(t, fd_bw), bw = t - bh * nbw;
            const int ic = c0 + cl;
            li[u] = (rl * cn + cl) * TBs + t;
            if (ic < IC) v[u] = d.w[(long long)(r0 + rl) * s_r + (long long)ic * s_ic + (khmin + bh) * d.s_kh + (kwmin + bw) * d.s_kw];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (li[u] >= 0) stage[li[u]] = v[u];
      }
      __syncthreads();
      const int cv = cn / VEC;
      const FastDiv fd_cv = make_fastdiv((unsigned)cv);
      const int wtotal = (orow1 - orow0) * cv;
      for (int i = tid; i < wtotal; i += 256) {
        const int ro = fd_div(i, fd_cv), pc = i - ro * cv;
        const int row = orow0 + ro;
        const int r = fd_div(row, fd_taps), tap = row - r * taps;
        const int kh = fd_div(tap, fd_kwo), kw = tap - kh * d.KWo;
        const int tb = (d.kh0 + kh * d.kh_step - khmin) * nbw + (d.kw0 + kw * d.kw_step - kwmin);
        const float* sp = stage + ((r - r0) * cn + pc * VEC) * TBs + tb;
        T* o = dst + (size_t)row * ICp + c0 + pc * VEC;
        if constexpr (VEC == 2) {
          union { T h[2]; unsigned u; } pk;
          pk.h[0] = (T)sp[0];
          pk.h[1] = (T)sp[TBs];
          *reinterpret_cast<unsigned*>(o) = pk.u;
        } else {
          o[0] = (T)sp[0];
        }
      }
    }
  }
}
__global__ __launch_bounds__(256) void pack_weights_multi_kernel(const yv4_pack_desc* __restrict__ table, int n) {
  __shared__ float stage[kPackStage];
  // binary search of the descriptor (uniform per workgroup)
  int lo = 0, hi = n - 1;
  const int b = (int)blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const yv4_pack_desc d = table[lo];
  const int R = d.transpose ? d.Cin : d.Cout;
  const int nrows = R * d.KHo * d.KWo;
  const int row0 = (b - d.first_block) * d.rows_per_block;
  const int row1 = row0 + d.rows_per_block < nrows ? row0 + d.rows_per_block : nrows;
  if (row0 >= row1) return;
  switch (d.dtype) {
    case YV4_F32: pack_rows<float>(d, row0, row1, stage); break;
    case YV4_F16: pack_rows<_Float16>(d, row0, row1, stage); break;
    default: pack_rows<__bf16>(d, row0, row1, stage); break;
  }
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_pack_weight(const float* w, int64_t s_co, int64_t s_ci, int64_t s_kh, int64_t s_kw, int Cout, int Cin,
                               int KH, int KW, int KHo, int KWo, int kh0, int kh_step, int kw0, int kw_step, int transpose,
                               int pad_to, void* dst, int dtype, void* stream) {
  YV4_REQUIRE(w && dst && Cout > 0 && Cin > 0 && KH > 0 && KW > 0 && KHo > 0 && KWo > 0 && pad_to > 0,
              "pack_weight: bad argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "pack_weight: dtype must be f32, f16 or bf16");
  const int khl = kh0 + (KHo - 1) * kh_step, kwl = kw0 + (KWo - 1) * kw_step;
  YV4_REQUIRE(kh0 >= 0 && kh0 < KH && khl >= 0 && khl < KH && kw0 >= 0 && kw0 < KW && kwl >= 0 && kwl < KW,
              "pack_weight: tap selection leaves the %dx%d kernel", KH, KW);
  const int IC = transpose ? Cout : Cin, R = transpose ? Cin : Cout;
  const int ICp = (IC + pad_to - 1) / pad_to * pad_to;
  const long long nrows = (long long)R * KHo * KWo;
  YV4_REQUIRE(nrows < (1LL << 31), "pack_weight: too many rows");
  const unsigned grid = (unsigned)(nrows < 8192 ? nrows : 8192);
  YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(pack_weight_kernel<T>, dim3(grid), dim3(256), 0,
                                           reinterpret_cast<hipStream_t>(stream), w, (long long)s_co, (long long)s_ci,
                                           (long long)s_kh, (long long)s_kw, Cout, Cin, KHo, KWo, kh0, kh_step, kw0, kw_step,
                                           transpose ? 1 : 0, ICp, reinterpret_cast<T*>(dst), (int)nrows));
  YV4_CHECK_LAUNCH("pack_weight");
  return YV4_OK;
}

extern "C" int yv4_pack_weights_multi(const yv4_pack_desc* table_dev, int n, int total_blocks, void* stream) {
  YV4_REQUIRE(table_dev && n > 0 && total_blocks > 0, "pack_weights_multi: bad argument");
  hipLaunchKernelGGL(pack_weights_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     table_dev, n);
  YV4_CHECK_LAUNCH("pack_weights_multi");
  return YV4_OK;
}
