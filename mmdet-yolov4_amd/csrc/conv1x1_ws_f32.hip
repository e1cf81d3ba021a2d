// fp32 1x1 / stride 1 convolution, weight-stationary and persistent (the fp32 form of conv1x1_ws_h16.hip).
// The pointwise layers with Cin <= 256 run at 50-57 % of the fp32 matrix peak on the tiles of conv_mfma_f32.hip (profiles/
// r02_layers.json): a tile's K loop is 2-8 slices, so a workgroup's life is mostly its first-slice latency and its
// epilogue.  Here one 8-wave workgroup per CU keeps its weight slab (BN x Cin floats, <= 64 KB) in LDS for the whole
// layer and every wave walks its own strips of 32 pixels with a private 3-stage LDS-DMA ring (stage = 32 pixels x 32
// channels) that runs on across strips; no barrier after the slab has landed.  The summation order of an output is
// EXACTLY the tile kernels' (slices of 32 channels in order; inside a slice the MFMA K pairs (8j+i, 8j+4+i), i = 0..3;
// two accumulator sets alternating with j, added once at the end), so a layer gives the same bits whichever kernel a
// batch size selects -- the plans' cross-batch bit-exactness (bench.py's output check) holds.
#include "conv_f32_common.h"

namespace yv4 {

constexpr int kWsfWaves = 8;
constexpr int kWsfThreads = kWsfWaves * 64;
constexpr int kWsfStages = 3;
constexpr int kWsfStageBytes = 4096;   // 32 pixels x 32 channels x 4 bytes
constexpr int kWsfGrid = 256;

template <int NT>
__global__ __launch_bounds__(kWsfThreads, 1) void conv1x1_ws_f32_kernel(ConvArgs p, unsigned x_bytes, unsigned w_bytes, int ncol,
                                                                        int nstrips, int cpr_shift) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  constexpr int BN = NT * 32;
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* smem_c = reinterpret_cast<char*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;
  const int h = lane >> 5;
#ifdef YV4_MEASURE
  // YV4_WSF_STAMP=1 (bit 8 of cpr_shift): cycles per wave in [1] the counted wait for a stage, [2] fragment reads + MFMAs +
  // the stage's DMA pieces, [3] epilogue up to its vmcnt(0), [4] rest of the epilogue; printed by two workgroups
  const bool stamp_on = (cpr_shift & 256) != 0;
  // YV4_WSF_ABL (wrong results on purpose): 1 a quarter of the output stores, 2 no stage DMAs, 4 no MFMAs, 8 no epilogue,
  // 16 stage DMAs issued but out of range (zero fill, nothing fetched)
  const bool few_stores = (cpr_shift & 512) != 0;
  const bool abl_nodma = (cpr_shift & 1024) != 0, abl_nomfma = (cpr_shift & 2048) != 0, abl_noepi = (cpr_shift & 4096) != 0;
  const bool abl_oob = (cpr_shift & 8192) != 0;
  cpr_shift &= 255;
  unsigned long long tsum[5] = {0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
  const unsigned long long tbegin = tlast;
#define YV4_WSF_STAMP(SLOT) if (stamp_on) { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); tsum[SLOT] += n_ - tlast; tlast = n_; }
#define YV4_WSF_OOB abl_oob
#define YV4_WSF_NODMA abl_nodma
#define YV4_WSF_NOMFMA abl_nomfma
#else
#define YV4_WSF_STAMP(SLOT)
#define YV4_WSF_OOB false
#define YV4_WSF_NODMA false
#define YV4_WSF_NOMFMA false
#endif
  const int kc_n = p.Cin >> 5;          // 32-channel stages per strip
  const int cpr = 1 << cpr_shift;       // 16-byte chunks per weight row (Cin / 4 >= 16)
  const int wpitch = p.Cin * 4;

  char* Ws = smem_c;
  char* ring = smem_c + BN * wpitch + wave * (kWsfStages * kWsfStageBytes);
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem;
  const unsigned ring_lds = lds_base + (unsigned)(BN * wpitch + wave * (kWsfStages * kWsfStageBytes));

  const unsigned b = blockIdx.x;
  const int xcd = (int)(b & 7u), local = (int)(b >> 3);
  const int col = local % ncol;
  const int walker = (local / ncol) * 8 + xcd;
  const int nwalkers = ((int)(gridDim.x >> 3) / ncol) * 8;
  const int NW = nwalkers * kWsfWaves;
  const int gw = walker * kWsfWaves + wave;
  const int n0 = col * BN;

  const u32x4_t rsA = make_rsrc(p.x, x_bytes);
  const u32x4_t rsB = make_rsrc(p.w, w_bytes);

  // the weight slab, once: rows of Cin floats, 16-byte chunks XOR-swizzled with row & 15
  {
    const int groups = (BN * cpr) >> 6;
    for (int g = wave; g < groups; g += kWsfWaves) {
      const int c = g * 64 + lane;
      const int row = c >> cpr_shift;
      const int pch = c & (cpr - 1);
      const int co = n0 + row;
      const unsigned voff = co < p.Cout ? (unsigned)(((int64_t)co * p.Kw + (pch ^ (row & 15)) * 4) * 4) : kOOB;
      lds_dma16(rsB, lds_base + (unsigned)(g * 1024), voff, 0u);
    }
  }

  float s1[NT], t1[NT], s2[NT], t2[NT];
  const bool has2 = p.s2 != nullptr;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = n0 + t * 32 + r;
    const bool ok = c < p.Cout;
    s1[t] = ok ? p.s1[c] : 0.f;
    t1[t] = ok ? p.t1[c] : 0.f;
    s2[t] = (ok && has2) ? p.s2[c] : 1.f;
    t2[t] = (ok && has2) ? p.t2[c] : 0.f;
  }

  const unsigned a_rd = (unsigned)(r * 128 + ((h ^ ((r >> 1) & 7)) << 4));
  unsigned w_rd[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = t * 32 + r;
    w_rd[t] = (unsigned)(row * wpitch + ((h ^ (row & 15)) << 4));
  }

  const int my_n = gw < nstrips ? (nstrips - gw + NW - 1) / NW : 0;
  const int lrow = lane >> 3;
  const unsigned lch_even = (unsigned)(((lane & 7) ^ ((lane >> 4) & 7)) * 4);
  const unsigned lch_odd = (unsigned)(((lane & 7) ^ (((lane >> 4) + 4) & 7)) * 4);
  // Issue side: the stage DMAs of a strip start at per-lane offsets that are computed once per strip (iss_voff: rows
  // 8 j + lrow, chunk swizzled by row); the stage adds its 128 bytes through the scalar offset.  In the loop the four
  // 1 KB pieces of stage kc + 2 are issued one per j step BETWEEN the wave's own MFMAs, where a piece's issue cost
  // (~60-180 cycles, MI355X_MICROARCH.md) runs under the MFMA in flight; issued in one block at the top of the stage
  // they were 1.0-1.4 k cycles per stage that only the partner wave's MFMAs could cover (stamps: DESIGN 12.9).
  int iss_i = 0, iss_kc = 0, iss_slot = 0;
  unsigned iss_voff[4];
#define YV4_WSF_ISSUE_STRIP()                                                                               \
  {                                                                                                         \
    const int row0_ = (gw + iss_i * NW) * 32 + lrow;                                                        \
    const bool live_ = iss_i < my_n && !YV4_WSF_OOB;                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                         \
      const int row_ = row0_ + 8 * j;                                                                       \
      const unsigned lch_ = (j & 1) ? lch_odd : lch_even;                                                   \
      iss_voff[j] = (live_ && row_ < p.M) ? (unsigned)(((int64_t)row_ * p.x_cs + p.x_co + (int)lch_) * 4) : kOOB; \
    }                                                                                                       \
  }
#define YV4_WSF_ISSUE_PIECE(J)                                                                              \
  if (!YV4_WSF_NODMA)                                                                                       \
    lds_dma16(rsA, ring_lds + (unsigned)(iss_slot * kWsfStageBytes + (J) * 1024), iss_voff[J], (unsigned)(iss_kc << 7));
#define YV4_WSF_ISSUE_ADVANCE()                                                                             \
  {                                                                                                         \
    iss_kc += 1;                                                                                            \
    if (iss_kc == kc_n) {                                                                                   \
      iss_kc = 0;                                                                                           \
      iss_i += 1;                                                                                           \
      YV4_WSF_ISSUE_STRIP();                                                                                \
    }                                                                                                       \
    iss_slot = iss_slot + 1 == kWsfStages ? 0 : iss_slot + 1;                                               \
  }
#define YV4_WSF_ISSUE()                                                                                     \
  {                                                                                                         \
    YV4_WSF_ISSUE_PIECE(0) YV4_WSF_ISSUE_PIECE(1) YV4_WSF_ISSUE_PIECE(2) YV4_WSF_ISSUE_PIECE(3)             \
    YV4_WSF_ISSUE_ADVANCE();                                                                                \
  }

  YV4_WSF_ISSUE_STRIP();
  YV4_WSF_ISSUE();
  YV4_WSF_ISSUE();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  float st_su[NT], st_sq[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { st_su[t] = 0.f; st_sq[t] = 0.f; }

  int rslot = 0;
  for (int i = 0; i < my_n; ++i) {
    f32x16 acc[NT], acc2[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[t][e] = 0.f; acc2[t][e] = 0.f; }

    for (int kc = 0; kc < kc_n; ++kc) {
      YV4_WSF_STAMP(4);
      // stages 0 and 1 of a strip were confirmed in front of the previous strip's stores; later ones by count: only the
      // four pieces of stage kc + 1 (issued during stage kc - 1) may still be in flight (see conv1x1_ws_h16.hip)
      if (kc >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      YV4_WSF_STAMP(1);
      const char* st = ring + rslot * kWsfStageBytes;
      const unsigned kx = (unsigned)(kc << 7);               // (kc * 8) << 4: chunk index inside the weight row
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (YV4_WSF_NOMFMA) { YV4_WSF_ISSUE_PIECE(j) continue; }
        const float4 fa = *reinterpret_cast<const float4*>(st + (a_rd ^ (unsigned)(j << 5)));
        float4 fb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) fb[t] = *reinterpret_cast<const float4*>(Ws + ((w_rd[t] ^ (unsigned)(j << 5)) ^ kx));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x16& ac_ = (j & 1) ? acc2[t] : acc[t];
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb[t].x, ac_, 0, 0, 0);
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb[t].y, ac_, 0, 0, 0);
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb[t].z, ac_, 0, 0, 0);
          ac_ = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb[t].w, ac_, 0, 0, 0);
          if (t == 0) {                      // piece j of stage kc + 2, under the MFMA just issued
            __builtin_amdgcn_sched_barrier(0);
            YV4_WSF_ISSUE_PIECE(j)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      YV4_WSF_ISSUE_ADVANCE();
      rslot = rslot + 1 == kWsfStages ? 0 : rslot + 1;
      YV4_WSF_STAMP(2);
    }

    // epilogue: lane (r, h) holds channel n0 + 32t + r of pixels m0 + (e&3) + 8(e>>2) + 4h; the arithmetic is
    // epilogue_tile's, operation for operation
    const int m0 = (gw + i * NW) * 32;
    const bool full = m0 + 32 <= p.M;
#ifdef YV4_MEASURE
    if (abl_noepi) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (acc[0][0] == 12345.678f) p.y[0] = acc[NT - 1][3] + acc2[0][1];
      continue;
    }
#endif
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = n0 + t * 32 + r;
      if (c >= p.Cout) continue;
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = acc[t][e] + acc2[t][e];
      if (p.stats) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const bool in = full || (m0 + (e & 3) + 8 * (e >> 2) + 4 * h < p.M);
          st_su[t] += in ? v[e] : 0.f;
          st_sq[t] += in ? v[e] * v[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = __builtin_fmaf(v[e], s1[t], t1[t]);     // epilogue_tile's a * s + t is an fma
      act_row16(v, p.act1, p.slope1);
      if (has2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = __builtin_fmaf(v[e], s2[t], t2[t]);
        act_row16(v, p.act2, p.slope2);
      }
      float* yb = p.y + ((int64_t)(m0 + 4 * h) * p.y_cs + p.y_co + c);
      if (t == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stages in flight, before the stores join the counter
      if (t == 0) { YV4_WSF_STAMP(3); }
#ifdef YV4_MEASURE
      if (few_stores) {
#pragma unroll
        for (int e = 0; e < 4; ++e) yb[(int64_t)((e & 3) + 8 * (e >> 2)) * p.y_cs] = v[e] + v[e + 4] + v[e + 8] + v[e + 12];
      } else
#endif
      if (full) {
#pragma unroll
        for (int e = 0; e < 16; ++e) yb[(int64_t)((e & 3) + 8 * (e >> 2)) * p.y_cs] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (m0 + (e & 3) + 8 * (e >> 2) + 4 * h < p.M) yb[(int64_t)((e & 3) + 8 * (e >> 2)) * p.y_cs] = v[e];
      }
    }
  }
#undef YV4_WSF_ISSUE
#undef YV4_WSF_ISSUE_PIECE
#undef YV4_WSF_ISSUE_ADVANCE
#undef YV4_WSF_ISSUE_STRIP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tail's out-of-range stage DMAs still write this wave's ring
#ifdef YV4_MEASURE
  YV4_WSF_STAMP(4);
  if (stamp_on && lane == 0 && (blockIdx.x == 0 || blockIdx.x == 101))
    printf("wsf wg %d wave %d strips %d: total %llu | issue %llu wait %llu reads+mfma %llu epi-to-vmcnt0 %llu epi-rest %llu (cycles)\n",
           (int)blockIdx.x, wave, my_n, __builtin_amdgcn_s_memtime() - tbegin, tsum[0], tsum[1], tsum[2], tsum[3], tsum[4]);
#endif
#undef YV4_WSF_STAMP
#undef YV4_WSF_OOB
#undef YV4_WSF_NODMA
#undef YV4_WSF_NOMFMA

  if (p.stats && my_n > 0) {
    const StatRep rep = stat_rep(p.stats, (unsigned)(gw), p.Cout);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float su = st_su[t], sq = st_sq[t];
      su += __shfl_xor(su, 32);
      sq += __shfl_xor(sq, 32);
      const int c = n0 + t * 32 + r;
      if (h == 0 && c < p.Cout) {
        stat_add(rep, c, su);
        stat_add(rep, p.Cout + c, sq);
      }
    }
  }
}

int wsf_slab_cols(const ConvArgs& a) {
  const int cout32 = (a.Cout + 31) / 32 * 32;
  for (int bn = 128; bn >= 32; bn >>= 1) {
    if (bn > cout32) continue;
    if ((long long)bn * a.Cin * 4 + kWsfWaves * kWsfStages * kWsfStageBytes > 160 * 1024) continue;
    const int ncol = (a.Cout + bn - 1) / bn;
    if (32 % ncol != 0) continue;
    return bn;
  }
  return 0;
}

bool conv1x1_ws_f32_applies(const ConvArgs& a) {
  return a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && !a.ys_on && a.res == nullptr && a.ksplit <= 1 &&
         (a.Cin == 64 || a.Cin == 128 || a.Cin == 256) && a.Kw == a.Cin && a.Cout >= 32 && wsf_slab_cols(a) > 0;
}

template <int NT>
static int launch_wsf(const ConvArgs& a, hipStream_t stream) {
  constexpr int BN = NT * 32;
  const int ncol = (a.Cout + BN - 1) / BN;
  const size_t lds = (size_t)BN * a.Cin * 4 + (size_t)kWsfWaves * kWsfStages * kWsfStageBytes;
  const int nstrips = (a.M + 31) / 32;
  int cpr_shift = 0;
  while ((4 << cpr_shift) < a.Cin) ++cpr_shift;
  const long long xb = x_bytes(a), wb = w_bytes(a);
  auto kern = conv1x1_ws_f32_kernel<NT>;
  static LdsAttrOnce once;
  if (int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(kern), 160 * 1024, "conv1x1_ws_f32")) return rc;
#ifdef YV4_MEASURE
  static const int stamp = YV4_ENV_INT("YV4_WSF_STAMP", 0);
  if (stamp) cpr_shift |= 256;
  static const int abl = YV4_ENV_INT("YV4_WSF_ABL", 0);
  cpr_shift |= (abl & 31) << 9;
#endif
  hipLaunchKernelGGL(kern, dim3(kWsfGrid), dim3(kWsfThreads), lds, stream, a, (unsigned)xb, (unsigned)wb, ncol, nstrips,
                     cpr_shift);
  YV4_CHECK_LAUNCH("conv1x1_ws_f32");
  return YV4_OK;
}

int conv1x1_ws_f32_launch(const ConvArgs& a, hipStream_t s) {
  switch (wsf_slab_cols(a)) {
    case 128: return launch_wsf<4>(a, s);
    case 64: return launch_wsf<2>(a, s);
    case 32: return launch_wsf<1>(a, s);
    default: break;
  }
  set_error("conv1x1 ws f32: no weight slab of this layer fits the LDS");
  return YV4_E_UNSUPPORTED;
}

}  // namespace yv4
