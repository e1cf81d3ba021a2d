// The kw-shared 3x3 weight gradient on gfx950: both forms of the kernel (the first in the measurement build only),
// its domain test (wgrad3x3_applies) and its launch function (wgrad3x3_launch).  The dispatcher, wgrad_impl, is in
// conv_wgrad.hip; what the weight gradient replaces in the reference's training step is said there.
#include "wgrad_common.h"

namespace yv4 {

// ---------------------------------------------------------------------------------
// Weight gradient of the 3x3 / stride-1 / pad-1 layers with Cin % 128 == 0 (71 % of YOLOv4-L's weight-gradient FLOPs):
// the three kw taps of one (kh, 128-channel chunk) share ONE LDS image of the slice's source pixels.
//   dW[co][kh][kw][ci] = sum_m dY[m][co] * X[m + (kh - 1) W + (kw - 1)][ci]      (flattened pixel index m; borders masked)
// The generic 16-bit kernel (conv_wgrad.hip) fetches 32 KB per 64-row slice for a 128 x 128 tile of dW (64 FLOP per byte of LDS fill, the regime
// in which the forward tiles sit at the L2 -> LDS limit).  Here an 8-wave workgroup owns 128 co x (3 kw x 128 ci) of dW
// and one chunk of the M reduction: per slice the 64 rows of dY and the 66 source pixels of X (one image for all three
// kw: operand row = reduction row + kw) are 32.5 KB of fill for 6.3 MFLOP -- 190 FLOP per byte -- and a wave (64 co x 32
// ci x 3 kw = six accumulators) needs ten transposed reads per six MFMAs instead of eight per four.  What a shifted row
// must not see (left / right image border, rows above / below, the neighbouring image) is masked per LANE: a lane of a
// ds_read_b64_tr_b16 supplies the address of ONE reduction row, so redirecting it to a zero row zeroes that row's
// contribution for every column of the transposed block.  Four slice buffers, three slices of LDS-DMA in flight, one
// barrier per slice placed in front of the LAST 16-row step so that the next slice's first fragments are read while
// that step's MFMAs run.  Same chunked, deterministic output as the generic kernels (slab per chunk + wgrad_reduce_kernel).
// ---------------------------------------------------------------------------------
constexpr int kW3Threads = 512;
constexpr int kW3XRows = 68;                       // 66 source pixels + one DMA group of 4; rows 66, 67 are only ever zero
constexpr int kW3ZeroRow = 66;
constexpr int kW3BufBytes = (kW3Rows + kW3XRows) * 256;
constexpr int kW3NBuf = 4;
constexpr int kW3Lds = kW3NBuf * kW3BufBytes;      // 135 168 B: one workgroup per CU

#ifdef YV4_MEASURE   // the FIRST form of the 3x3 weight gradient: the measurement build's A/B partner of the second form (same bits); the product takes the generic 16-bit kernel where the second form does not apply
template <bool BF16>
__global__ __launch_bounds__(kW3Threads, 2) void conv_wgrad3x3_h16_kernel(WgradArgs p, unsigned x_bytes, unsigned dy_bytes) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(3))) s16x4_t* lds_v4_t;
  extern __shared__ __attribute__((aligned(16))) char smem_w3[];
  constexpr int kRowB = 256;
  constexpr int kDBytes = kW3Rows * kRowB;           // dY part of a buffer; the X image follows it
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 2;                          // co half (64 rows of dW)
  const int wk = wave & 3;                           // ci slab (32 columns per kw)

  // tile: (co tile, kh, ci tile), ci fastest
  const int tiles_ci = p.Cin >> 7;
  int tile, chunk;
  if (!wgrad_tile_chunk(p.tiles, p.chunks, p.xcd_map, tile, chunk)) return;
  const int tci = tile % tiles_ci;
  const int kh = (tile / tiles_ci) % 3;
  const int tco = tile / (3 * tiles_ci);
  const int co0 = tco * 128, ci0 = tci * 128;
  const int m_lo = chunk * p.rows_per_chunk;
  const int m_hi = min(m_lo + p.rows_per_chunk, p.M);
  if (m_lo >= m_hi) return;
  const int NHW = p.N * p.H * p.W;

  const u32x4_t rsX = make_rsrc(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc(p.dy, dy_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem_w3;

  // ---- staging: a DMA instruction covers 4 rows x 16 chunks; wave w fills rows 8w .. 8w+7 of dY and of the X image,
  // wave 0 also the 17th group of the image (rows 64 .. 67: pixels 64, 65 + two zero rows)
  const int srow = lane >> 4;
  const int pc = lane & 15;
  auto swz_of = [](int row) { return ((row & 3) << 2) | ((row >> 2) & 3); };
  int d_col[2], x_col[3], x_row[3];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = 8 * wave + 4 * q + srow;
    const int lc = pc ^ swz_of(row);
    const int co = co0 + lc * 8;
    d_col[q] = co < p.Cout ? co : -1;
    x_col[q] = ci0 + lc * 8;
    x_row[q] = row;
  }
  {
    const int row = 64 + srow;
    x_col[2] = ci0 + (pc ^ swz_of(row)) * 8;
    x_row[2] = row;
  }
  const int x_shift = (kh - 1) * p.W - 1;            // image row ir <-> pixel m_slice + ir + x_shift
  auto issue = [&](int sl, int nsl) {
    const int buf = sl & (kW3NBuf - 1);
    const int m_base = m_lo + sl * kW3Rows;
    const bool live = sl < nsl;
    const unsigned lb = lds_base + (unsigned)(buf * kW3BufBytes + 8 * wave * kRowB);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = m_base + 8 * wave + 4 * q + srow;
      unsigned doff = kOOB;
      if (live && m < m_hi && d_col[q] >= 0) doff = (unsigned)((((int64_t)m * p.dy_cs) + p.dy_co + d_col[q]) * 2);
      lds_dma16(rsD, lb + (unsigned)(4 * q * kRowB), doff, 0u);
      const int pix = m_base + x_row[q] + x_shift;
      unsigned xoff = kOOB;
      if (live && (unsigned)pix < (unsigned)NHW) xoff = (unsigned)((((int64_t)pix * p.x_cs) + p.x_co + x_col[q]) * 2);
      lds_dma16(rsX, lb + (unsigned)(kDBytes + 4 * q * kRowB), xoff, 0u);
    }
    if (wave == 0) {
      const int pix = m_base + x_row[2] + x_shift;
      unsigned xoff = kOOB;
      if (live && x_row[2] < 66 && (unsigned)pix < (unsigned)NHW) xoff = (unsigned)((((int64_t)pix * p.x_cs) + p.x_co + x_col[2]) * 2);
      lds_dma16(rsX, lds_base + (unsigned)(buf * kW3BufBytes + kDBytes + 64 * kRowB), xoff, 0u);
    }
  };

  // ---- transposed fragment reads (see conv_wgrad_h16_kernel): lane = 16 g + 4 qq + pp supplies row (block + qq),
  // columns 4 pp .. 4 pp + 3 of its 16-column half
  const int g = lane >> 4, i16 = lane & 15;
  const int hh = g >> 1, colhalf = g & 1;
  const int qq = i16 >> 2, pp = i16 & 3;
  auto row_addr = [&](int row, int col_base) -> unsigned {
    const int chunk = (col_base + 16 * colhalf) / 8 + (pp >> 1);
    return (unsigned)(kRowB * row + 16 * (chunk ^ swz_of(row)) + 8 * (pp & 1));
  };
  unsigned d_rd[2][4][2];                            // dY: [co tile a][step s][j]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) d_rd[a][s][j] = row_addr(16 * s + 8 * hh + 4 * j + qq, wc * 64 + a * 32);
  const unsigned zero_rd = (unsigned)(kDBytes + kW3ZeroRow * kRowB);

  f32x16 acc[2][3];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int nsl = (m_hi - m_lo + kW3Rows - 1) / kW3Rows;
  // border masks of this lane's eight reduction rows of a slice: bit (s * 2 + j) * 3 + kw set = row contributes to tap kw
  auto slice_masks = [&](int sl) -> unsigned {
    unsigned mk = 0u;
    const int hw = p.H * p.W;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int m = m_lo + sl * kW3Rows + 16 * s + 8 * hh + 4 * j + qq;
        unsigned b3 = 0u;
        if (m < m_hi) {
          const int n = fd_div(m, p.fd_hw);
          const int rm = m - n * hw;
          const int ho = fd_div(rm, p.fd_wo);
          const int wo = rm - ho * p.W;
          if ((unsigned)(ho + kh - 1) < (unsigned)p.H)
            b3 = (wo > 0 ? 1u : 0u) | 2u | (wo + 1 < p.W ? 4u : 0u);
        }
        mk |= b3 << ((s * 2 + j) * 3);
      }
    return mk;
  };

  // measurement-only bits (YV4_W3_ABLATE): 1 no MFMAs, 2 no fragment reads, 4 no DMA after the prologue, 8 no border
  // masks, 16 no output
  s16x8_t fa[2][2] = {}, fb[2][3] = {};              // fragment sets: step s computes from set s & 1
#define YV4_W3_LOAD(SET, BUFP, S, MK)                                                                         \
  if (!YV4_ABLATE(p.ablate, 2)) {                                                                             \
    const char* db_ = (BUFP);                                                                                 \
    _Pragma("unroll") for (int a = 0; a < 2; ++a) {                                                           \
      const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(db_ + d_rd[a][S][0]));           \
      const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(db_ + d_rd[a][S][1]));           \
      fa[SET][a] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);                                   \
    }                                                                                                         \
    _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                                        \
      const unsigned r0_ = (((MK) >> (((S) * 2 + 0) * 3 + kw)) & 1u)                                          \
          ? (unsigned)kDBytes + row_addr(16 * (S) + 8 * hh + qq + kw, wk * 32) : zero_rd;                     \
      const unsigned r1_ = (((MK) >> (((S) * 2 + 1) * 3 + kw)) & 1u)                                          \
          ? (unsigned)kDBytes + row_addr(16 * (S) + 8 * hh + 4 + qq + kw, wk * 32) : zero_rd;                 \
      const s16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(db_ + r0_));                      \
      const s16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(db_ + r1_));                      \
      fb[SET][kw] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);                                  \
    }                                                                                                         \
  }
#define YV4_W3_MFMA(SET)                                                                                      \
  {                                                                                                           \
    _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                             \
      _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                                      \
        if (YV4_ABLATE(p.ablate, 1)) { acc[a][kw][0] += __builtin_bit_cast(float, (int)(fa[SET][a][0] + fb[SET][kw][0])); continue; } \
        if (BF16)                                                                                             \
          acc[a][kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_w, fa[SET][a]),      \
                                                               __builtin_bit_cast(bf16x8_w, fb[SET][kw]), acc[a][kw], 0, 0, 0); \
        else                                                                                                  \
          acc[a][kw] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_w, fa[SET][a]),        \
                                                              __builtin_bit_cast(f16x8_w, fb[SET][kw]), acc[a][kw], 0, 0, 0); \
      }                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                        \
  }
  // pieces per slice: 4 (5 on wave 0).  In slice t the wave issues DMA(t + 3) BEFORE the wait in front of the last
  // step, where it needs its own DMA(t + 1) landed: DMA(t + 2) and DMA(t + 3) may stay in flight.
#define YV4_W3_WAIT()                                                                                         \
  {                                                                                                           \
    if (wave == 0) asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");                               \
    else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");                                          \
  }

  issue(0, nsl);
  issue(1, nsl);
  issue(2, nsl);
  YV4_W3_WAIT();                                      // DMA(0) landed (newer: 1, 2)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  unsigned mk = slice_masks(0);
  YV4_W3_LOAD(0, smem_w3, 0, mk);
  for (int sl = 0; sl < nsl; ++sl) {
    const char* bufp = smem_w3 + (sl & (kW3NBuf - 1)) * kW3BufBytes;
    const char* nbufp = smem_w3 + ((sl + 1) & (kW3NBuf - 1)) * kW3BufBytes;
    const unsigned mkn = YV4_ABLATE(p.ablate, 8) ? 0xFFFFFFu : slice_masks(sl + 1);
    YV4_W3_LOAD(1, bufp, 1, mk);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3_MFMA(0);
    if (!YV4_ABLATE(p.ablate, 4)) issue(sl + 3, nsl);   // into the buffer slice sl - 1 read (freed by the previous barrier)
    else issue(nsl, nsl);                             // (the counted waits need the instruction count: all lanes out of range)
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3_LOAD(0, bufp, 2, mk);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3_MFMA(1);
    YV4_W3_LOAD(1, bufp, 3, mk);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3_MFMA(0);
    YV4_W3_WAIT();                                    // own DMA(sl + 1) landed; every read of slice sl has returned
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    YV4_W3_LOAD(0, nbufp, 0, mkn);                    // (beyond the last slice: zero-filled buffers, never used)
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3_MFMA(1);
    mk = mkn;
  }
#undef YV4_W3_WAIT
#undef YV4_W3_MFMA
#undef YV4_W3_LOAD
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the dummy tail DMAs must land before the LDS is released

  // D[row = co][col = ci]: row = (e&3) + 8*(e>>2) + 4*(lane>>5), col = lane&31
  const int r = lane & 31, h5 = lane >> 5;
  if (YV4_ABLATE(p.ablate, 16) && acc[0][0][0] != 123.f) return;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int kcol = (kh * 3 + kw) * p.Cin + ci0 + wk * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wc * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h5;
        if (co < p.Cout) {
          if (p.ws) p.ws[(size_t)chunk * p.ws_stride + (size_t)co * p.K + kcol] = acc[a][kw][e];
          else atomicAdd(&p.dw[(size_t)co * p.K + kcol], acc[a][kw][e]);
        }
      }
    }
}
#endif  // YV4_MEASURE

// ---------------------------------------------------------------------------------
// The same kernel with its loop overhead removed (round 5).  The disassembly of the kernel above has, per 64-row slice and
// wave, 24 MFMAs (768 matrix-pipe cycles) beside 340 VALU and 173 scalar instructions: 1 360 cycles of vector issue for 768
// of matrix work, two waves per SIMD -- the loop was bound by its address arithmetic, not by LDS or the matrix pipe
// (ablation, profiles/r05_wgrad3x3_v2.md: without the border masks alone 265 -> 204 us in the measurement build).  What
// the instructions were: the per-lane border masks (8 rows x 2 divisions by invariant divisors per slice), one 32-bit add
// per fragment read (buffer pointer + precomputed offset), a compare + select pair per masked read on top of the bit test,
// the DMA offsets rebuilt from the row index with 64-bit multiplies.  Here:
//   * border flags are computed ONCE per slice row by one wave (64 lanes = 64 rows) when the slice's DMA is issued and
//     left in 64 bytes of LDS beside the slice buffer, laid out so that a lane fetches the flags of its eight rows with one
//     ds_read_b64 a whole slice ahead of their use;
//   * fragment addresses are lane constants + the slice buffer's offset + an immediate (the swizzle is periodic in 16
//     rows, so the four 16-row steps differ by 4 096 bytes): 4 adds per slice for the 16 dY reads; a masked X read is
//     zero-row + flag * (lane constant) -- one bit-field extract and one multiply-add, no compare, no select;
//   * DMA offsets advance by a constant per slice and are range-checked as OFFSETS against lane-constant limits.
// The MFMAs, their order and the LDS images are the kernel's above: the results are bit-identical to it
// (tools/ab_w3g.sh compares the two in the measurement build; tests/test_gpu_h16.py::test_h16_wgrad3x3_kernel holds this one to
// fp64 per tap and to run-to-run bit-identity).
// ---------------------------------------------------------------------------------
constexpr int kW3FlagBase = kW3Lds;                  // kW3NBuf x 64 flag bytes behind the slice buffers
constexpr int kW3LdsV2 = kW3Lds + kW3NBuf * 64;

#ifndef YV4_W3V2_STAGGER
#define YV4_W3V2_STAGGER 1     // build-time A/B (tools/ab_prev.sh): 0 = all eight waves issue DMA(sl + 3) at the same point
#endif
// ABL (measurement build only, compile-time so that the timed kernel carries no extra branches): 1 no DMA inside the loop,
// 2 no workgroup barrier, 4 no MFMAs, 8 no fragment reads, 16 no border masks on the image reads -- wrong results on purpose, to
// time the kernel without a part
template <bool BF16, int ABL = 0>
__global__ __launch_bounds__(kW3Threads, 2) void conv_wgrad3x3_v2_h16_kernel(WgradArgs p, unsigned x_bytes, unsigned dy_bytes) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(3))) s16x4_t* lds_v4_t;
  typedef __attribute__((address_space(3))) unsigned long long* lds_u64_t;
  typedef __attribute__((address_space(3))) unsigned char* lds_u8_t;
  extern __shared__ __attribute__((aligned(16))) char smem_w3b[];
  constexpr int kRowB = 256;
  constexpr int kDBytes = kW3Rows * kRowB;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 2;
  const int wk = wave & 3;

  const int tiles_ci = p.Cin >> 7;
  int tile, chunk;
  if (!wgrad_tile_chunk(p.tiles, p.chunks, p.xcd_map, tile, chunk)) return;
  const int tci = tile % tiles_ci;
  const int kh = (tile / tiles_ci) % 3;
  const int tco = tile / (3 * tiles_ci);
  const int co0 = tco * 128, ci0 = tci * 128;
  const int m_lo = chunk * p.rows_per_chunk;
  const int m_hi = min(m_lo + p.rows_per_chunk, p.M);
  if (m_lo >= m_hi) return;
  const int NHW = p.N * p.H * p.W;

  const u32x4_t rsX = make_rsrc(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc(p.dy, dy_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem_w3b;

  // ---- staging (as above): wave w fills rows 8w .. 8w+7 of dY and of the X image, wave 0 also rows 64 .. 67 of the image.
  // Byte offsets of slice 0 and their limits; both advance by a constant per slice.
  const int srow = lane >> 4;
  const int pc = lane & 15;
  auto swz_of = [](int row) { return ((row & 3) << 2) | ((row >> 2) & 3); };
  const int x_shift = (kh - 1) * p.W - 1;            // image row ir <-> pixel m_slice + ir + x_shift
  const unsigned d_step = (unsigned)(kW3Rows * p.dy_cs * 2), x_step = (unsigned)(kW3Rows * p.x_cs * 2);
  unsigned d_off[2], d_lim[2], x_off[3], x_lim[3];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = 8 * wave + 4 * q + srow;
    const int lc = pc ^ swz_of(row);
    const int co = co0 + lc * 8;
    const unsigned cb = (unsigned)((p.dy_co + co) * 2);
    d_off[q] = (unsigned)(m_lo + row) * (unsigned)(p.dy_cs * 2) + cb;
    d_lim[q] = co < p.Cout ? (unsigned)m_hi * (unsigned)(p.dy_cs * 2) + cb : 0u;        // 0: never below -> out of range
    const unsigned xb_ = (unsigned)((p.x_co + ci0 + lc * 8) * 2);
    x_off[q] = (unsigned)(m_lo + row + x_shift) * (unsigned)(p.x_cs * 2) + xb_;          // (a negative pixel wraps to ~2^32)
    x_lim[q] = (unsigned)NHW * (unsigned)(p.x_cs * 2) + xb_;
  }
  {
    const int row = 64 + srow;
    const unsigned xb_ = (unsigned)((p.x_co + ci0 + (pc ^ swz_of(row)) * 8) * 2);
    x_off[2] = (unsigned)(m_lo + row + x_shift) * (unsigned)(p.x_cs * 2) + xb_;
    x_lim[2] = row < 66 ? (unsigned)NHW * (unsigned)(p.x_cs * 2) + xb_ : 0u;             // rows 66, 67 stay zero
  }
  // border flags of slice row r = lane (written by wave 1): position of the byte inside the slice's 64 flag bytes
  const int f_wr = (((lane & 3) * 2 + ((lane >> 3) & 1)) << 3) + ((lane >> 4) << 1) + ((lane >> 2) & 1);
  int f_m = m_lo + lane;                             // (wave 1) the row this lane decodes next
  auto issue = [&](int sl) {
    const int buf = sl & (kW3NBuf - 1);
    const unsigned lb = lds_base + (unsigned)(buf * kW3BufBytes + 8 * wave * kRowB);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      lds_dma16(rsD, lb + (unsigned)(4 * q * kRowB), d_off[q] < d_lim[q] ? d_off[q] : kOOB, 0u);
      lds_dma16(rsX, lb + (unsigned)(kDBytes + 4 * q * kRowB), x_off[q] < x_lim[q] ? x_off[q] : kOOB, 0u);
      d_off[q] += d_step;
      x_off[q] += x_step;
    }
    if (wave == 0) {
      lds_dma16(rsX, lds_base + (unsigned)(buf * kW3BufBytes + kDBytes + 64 * kRowB), x_off[2] < x_lim[2] ? x_off[2] : kOOB, 0u);
      x_off[2] += x_step;
    }
    if (wave == 1) {
      unsigned b3 = 0u;
      if (f_m < m_hi) {
        const int n = fd_div(f_m, p.fd_hw);
        const int rm = f_m - n * (p.H * p.W);
        const int ho = fd_div(rm, p.fd_wo);
        const int wo = rm - ho * p.W;
        if ((unsigned)(ho + kh - 1) < (unsigned)p.H) b3 = (wo > 0 ? 1u : 0u) | 2u | (wo + 1 < p.W ? 4u : 0u);
      }
      *(lds_u8_t)(smem_w3b + kW3FlagBase + buf * 64 + f_wr) = (unsigned char)b3;
      f_m += kW3Rows;
    }
  };

  // ---- transposed fragment reads: lane = 16 g + 4 qq + pp supplies row (block + qq), columns 4 pp .. 4 pp + 3 of its
  // 16-column half; step S adds 16 rows = 4 096 bytes (the swizzle only sees the row's low four bits)
  const int g = lane >> 4, i16 = lane & 15;
  const int hh = g >> 1, colhalf = g & 1;
  const int qq = i16 >> 2, pp = i16 & 3;
  auto row_addr = [&](int row, int col_base) -> int {
    const int chunk_ = (col_base + 16 * colhalf) / 8 + (pp >> 1);
    return kRowB * row + 16 * (chunk_ ^ swz_of(row)) + 8 * (pp & 1);
  };
  constexpr int kZeroRd = kDBytes + kW3ZeroRow * kRowB;
  int a_base[2][2];                                  // dY: [co tile a][j], step 0, buffer 0
  int b_dlt[2][3][4];                                // X: (address of row 16 S + 8 hh + 4 j + qq + kw) - (zero row), [j][kw][S]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int a = 0; a < 2; ++a) a_base[a][j] = row_addr(8 * hh + 4 * j + qq, wc * 64 + a * 32);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int S = 0; S < 4; ++S) b_dlt[j][kw][S] = kDBytes + row_addr(16 * S + 8 * hh + 4 * j + qq + kw, wk * 32) - kZeroRd;
  }
  const int f_rd = kW3FlagBase + ((qq * 2 + hh) << 3);

  f32x16 acc[2][3];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int nsl = (m_hi - m_lo + kW3Rows - 1) / kW3Rows;
  s16x8_t fa[2][2] = {}, fb[2][3] = {};              // fragment sets: step s computes from set s & 1
  // FL: the eight flag bytes of this lane's rows of the slice ([S][j], bits kw); BO: the slice buffer's byte offset
#define YV4_W3B_LOAD(SET, BO, S, FL)                                                                          \
  if constexpr (!(ABL & 8)) {                                                                                 \
    const char* ab_ = smem_w3b + (BO) + 4096 * (S);                                                           \
    _Pragma("unroll") for (int a = 0; a < 2; ++a) {                                                           \
      const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(ab_ + a_base[a][0]));            \
      const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(ab_ + a_base[a][1]));            \
      fa[SET][a] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);                                   \
    }                                                                                                         \
    const unsigned fw_ = (unsigned)((FL) >> (((S) >> 1) * 32));                                               \
    const int zb_ = (BO) + kZeroRd;                                                                           \
    _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                                        \
      const int f0_ = (ABL & 16) ? 1 : (int)((fw_ >> ((((S) & 1) * 2 + 0) * 8 + kw)) & 1u);                   \
      const int f1_ = (ABL & 16) ? 1 : (int)((fw_ >> ((((S) & 1) * 2 + 1) * 8 + kw)) & 1u);                   \
      const int r0_ = __mul24(f0_, b_dlt[0][kw][S]) + zb_;                                   \
      const int r1_ = __mul24(f1_, b_dlt[1][kw][S]) + zb_;                                   \
      const s16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(smem_w3b + r0_));                 \
      const s16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(smem_w3b + r1_));                 \
      fb[SET][kw] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);                                  \
    }                                                                                                         \
  }
#define YV4_W3B_MFMA(SET)                                                                                     \
  {                                                                                                           \
    _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                             \
      _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                                      \
        if constexpr (ABL & 4) { asm volatile("" :: "v"(fa[SET][a]), "v"(fb[SET][kw])); continue; }          \
        if (BF16)                                                                                             \
          acc[a][kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_w, fa[SET][a]),      \
                                                               __builtin_bit_cast(bf16x8_w, fb[SET][kw]), acc[a][kw], 0, 0, 0); \
        else                                                                                                  \
          acc[a][kw] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_w, fa[SET][a]),        \
                                                              __builtin_bit_cast(f16x8_w, fb[SET][kw]), acc[a][kw], 0, 0, 0); \
      }                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                        \
  }
  // pieces per slice: 4 (5 on wave 0); DMA(t + 2) and DMA(t + 3) may stay in flight at the wait of slice t
#define YV4_W3B_WAIT()                                                                                        \
  {                                                                                                           \
    if (wave == 0) asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");                               \
    else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");                                          \
  }

  issue(0);
  issue(1);
  issue(2);
  YV4_W3B_WAIT();                                     // DMA(0) landed (newer: 1, 2); the flag bytes are written
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  unsigned long long fl = *(lds_u64_t)(smem_w3b + f_rd);
  YV4_W3B_LOAD(0, 0, 0, fl);
  for (int sl = 0; sl < nsl; ++sl) {
    const int bo = (sl & (kW3NBuf - 1)) * kW3BufBytes;
    const int nb = (sl + 1) & (kW3NBuf - 1);
    const int nbo = nb * kW3BufBytes;
    // flags of slice sl + 1: written when its DMA was issued (two barriers ago), wanted after this slice's barrier
    const unsigned long long fln = *(lds_u64_t)(smem_w3b + f_rd + nb * 64);
    YV4_W3B_LOAD(1, bo, 1, fl);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_MFMA(0);
    // DMA(sl + 3) into the buffer slice sl - 1 read (freed by the previous barrier): waves 0-3 issue their 4-5 pieces
    // here, waves 4-7 (their partners on the SIMDs) one MFMA step later -- issued by all eight waves at the same point
    // the pieces' 400-500 issue cycles left the matrix pipe idle (compile-time ablation: -10 % without the DMA)
    if constexpr (!(ABL & 1)) { if (wave < 4 || !YV4_W3V2_STAGGER) issue(sl + 3); }
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_LOAD(0, bo, 2, fl);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_MFMA(1);
    if constexpr (!(ABL & 1)) { if (wave >= 4 && YV4_W3V2_STAGGER) issue(sl + 3); }
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_LOAD(1, bo, 3, fl);
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_MFMA(0);
    if constexpr (!(ABL & 1)) YV4_W3B_WAIT()          // own DMA(sl + 1) landed; every read of slice sl has returned
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!(ABL & 2)) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    YV4_W3B_LOAD(0, nbo, 0, fln);                     // (beyond the last slice: zero-filled buffers, never used)
    __builtin_amdgcn_sched_barrier(0);
    YV4_W3B_MFMA(1);
    fl = fln;
  }
#undef YV4_W3B_WAIT
#undef YV4_W3B_MFMA
#undef YV4_W3B_LOAD
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the dummy tail DMAs must land before the LDS is released

  // D[row = co][col = ci]: row = (e&3) + 8*(e>>2) + 4*(lane>>5), col = lane&31
  const int r = lane & 31, h5 = lane >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int kcol = (kh * 3 + kw) * p.Cin + ci0 + wk * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wc * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h5;
        if (co < p.Cout) {
          if (p.ws) p.ws[(size_t)chunk * p.ws_stride + (size_t)co * p.K + kcol] = acc[a][kw][e];
          else atomicAdd(&p.dw[(size_t)co * p.K + kcol], acc[a][kw][e]);
        }
      }
    }
}

// The tiles of one reduction chunk read the same rows of dY and (shifted by a row) of the activation; workgroups go to the
// eight XCDs round-robin, so with the plain (tile, chunk) grid a chunk's tiles sit on different XCDs and every XCD's L2
// fetches those rows for itself.  With the mapping of wgrad_tile_chunk they share one L2.
static const int g_w3_xcd = YV4_ENV_INT("YV4_W3_XCD", 0);   // measured: 112 -> 115 / 113 -> 122 us on 128->128 @76 / 256->256 @38 -- off
bool w3_xcd_map(long long tiles, long long chunks) { return g_w3_xcd && tiles >= 2 && chunks >= 16; }

// domain of conv_wgrad3x3_h16_kernel
bool wgrad3x3_applies(const yv4_conv_desc* d, int dtype) {
  static const int mode = YV4_ENV_INT("YV4_WGRAD3", 1);
  return mode && dtype != YV4_F32 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->Ho == d->H &&
         d->Wo == d->W && (d->Cin & 127) == 0 && (long long)d->N * d->H * d->W < (1LL << 30);
}

int wgrad3x3_launch(WgradArgs& a, int dtype, long long xb, long long db, long long ch, void* stream, bool w3_v2_ok) {
  const long long tl = (long long)((a.Cout + 127) / 128) * 3 * (a.Cin / 128);
#ifdef YV4_MEASURE
  static LdsAttrOnce once3b, once3h;
  if (int rc = ensure_dyn_lds(once3b, reinterpret_cast<const void*>(conv_wgrad3x3_h16_kernel<true>), (size_t)kW3Lds, "conv_wgrad3x3_h16")) return rc;
  if (int rc = ensure_dyn_lds(once3h, reinterpret_cast<const void*>(conv_wgrad3x3_h16_kernel<false>), (size_t)kW3Lds, "conv_wgrad3x3_h16")) return rc;
#endif
  a.tiles = (int)tl;
  a.chunks = (int)ch;
  a.xcd_map = w3_xcd_map(tl, ch) && tl * (ch + 8) < (1LL << 31) ? 1 : 0;
  static const int w3_ablate = YV4_ENV_INT("YV4_W3_ABLATE", 0);
  a.ablate = w3_ablate;
  const dim3 grid3 = wgrad_grid(tl, ch, a.xcd_map);
  // (the second form range-checks 32-bit byte OFFSETS: both maps well below 4 GB, so that a row in front of the map --
  // a wrapped offset -- can never fall below a limit)
  if (w3_v2_ok) {
    static LdsAttrOnce once3vb, once3vh;
    if (int rc = ensure_dyn_lds(once3vb, reinterpret_cast<const void*>(conv_wgrad3x3_v2_h16_kernel<true>), (size_t)kW3LdsV2, "conv_wgrad3x3_v2_h16")) return rc;
    if (int rc = ensure_dyn_lds(once3vh, reinterpret_cast<const void*>(conv_wgrad3x3_v2_h16_kernel<false>), (size_t)kW3LdsV2, "conv_wgrad3x3_v2_h16")) return rc;
#ifdef YV4_MEASURE
    static const int w3abl = YV4_ENV_INT("YV4_W3V2_ABL", 0);
#define YV4_W3ABL(N)                                                                                                   \
    if (w3abl == N && dtype == YV4_BF16) {                                                                             \
      static LdsAttrOnce once_abl;                                                                                     \
      if (int rc = ensure_dyn_lds(once_abl, reinterpret_cast<const void*>(conv_wgrad3x3_v2_h16_kernel<true, N>), (size_t)kW3LdsV2, "w3v2 abl")) return rc;   \
      hipLaunchKernelGGL((conv_wgrad3x3_v2_h16_kernel<true, N>), grid3, dim3(kW3Threads), (size_t)kW3LdsV2,           \
                         reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db);                        \
      YV4_CHECK_LAUNCH("w3v2 abl");                                                                                    \
      return YV4_OK;                                                                                                   \
    }
    YV4_W3ABL(1) YV4_W3ABL(2) YV4_W3ABL(3) YV4_W3ABL(4) YV4_W3ABL(8) YV4_W3ABL(12) YV4_W3ABL(5) YV4_W3ABL(13) YV4_W3ABL(15) YV4_W3ABL(16)
#undef YV4_W3ABL
#endif
    if (dtype == YV4_BF16)
      hipLaunchKernelGGL(conv_wgrad3x3_v2_h16_kernel<true>, grid3, dim3(kW3Threads), (size_t)kW3LdsV2,
                         reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db);
    else
      hipLaunchKernelGGL(conv_wgrad3x3_v2_h16_kernel<false>, grid3, dim3(kW3Threads), (size_t)kW3LdsV2,
                         reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db);
    YV4_CHECK_LAUNCH("conv_wgrad3x3_v2_h16");
    return YV4_OK;
  }
#ifdef YV4_MEASURE
  if (dtype == YV4_BF16)
    hipLaunchKernelGGL(conv_wgrad3x3_h16_kernel<true>, grid3, dim3(kW3Threads), (size_t)kW3Lds,
                       reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db);
  else
    hipLaunchKernelGGL(conv_wgrad3x3_h16_kernel<false>, grid3, dim3(kW3Threads), (size_t)kW3Lds,
                       reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db);
  YV4_CHECK_LAUNCH("conv_wgrad3x3_h16");
  return YV4_OK;
#else
  set_error("conv_wgrad3x3_h16: the first form exists in the measurement build only");   // wgrad_impl never asks for it
  return YV4_E_UNSUPPORTED;
#endif
}

}  // namespace yv4
