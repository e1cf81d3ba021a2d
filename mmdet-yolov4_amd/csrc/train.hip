// Training-side kernels of the YOLOv4 path on gfx950: the generic convolution weight gradient (fp32 MFMA, 16-bit MFMA
// and its second form), the deterministic slab reduce and the dispatcher over these and the two special 3x3 families
// (conv_wgrad3x3_h16.hip, conv_wgrad_fc_h16.hip); zero-dilation for the data gradient of strided convolutions; SPP
// max-pool backward, weight packing and nearest-resample backward.  Train-mode BatchNorm is in bn_train.hip.
//
// What they replace in the reference's training step:
//   cuDNN conv backward-filter / backward-data  (autograd of mmcv ConvModule, darknetcsp.py:15-35)
// The data gradient itself is the forward kernel again (conv_mfma_f32.hip) on dY with the
// weights transposed and flipped; for stride 2 dY is first zero-dilated (yv4_dilate2_fwd).
#include "train_common.h"
#include "wgrad_common.h"

namespace yv4 {

// ---------------------------------------------------------------------------------
// Weight gradient:  dW[co][k] += sum_m dY[m][co] * A[m][k],  A = im2col(x), k = (kh,kw,ci).
// A workgroup owns a 64 (co) x 64 (k) tile of dW and one chunk of the M = N*Ho*Wo reduction;
// slices of 32 rows of dY and of A go global -> LDS by LDS-DMA (rows of 64 floats, read back
// with ds_read_b32 along the row, so no swizzle is needed), each wave accumulates a 32x32 tile
// on v_mfma_f32_32x32x2_f32 with the reduction index m as the MFMA K dimension, and the
// chunk's partial tile is added to dW with float atomics (dW must be zero on entry).
// ---------------------------------------------------------------------------------
// T = float: rows of 64 floats (256 B), one LDS-DMA instruction of a wave covers 4 rows.
// T = _Float16 / __bf16: rows of 64 elements (128 B), one instruction covers 8 rows; the operands are
// widened to fp32 on the way from LDS to the MFMA (bf16 -> fp32 is a shift), so this form has the
// fp32 kernel's arithmetic and half its memory traffic.  (A v_mfma_f32_32x32x16 form needs both
// operands transposed on the way out of LDS -- ds_read_b64_tr_b16 -- and is next round's work.)
template <typename T>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(WgradArgs p, unsigned x_bytes, unsigned dy_bytes) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  constexpr int ES = (int)sizeof(T);
  constexpr int kChunkEl = 16 / ES;            // elements per 16-byte chunk: 4 or 8
  constexpr int kChunksPerRow = 64 / kChunkEl; // 16 or 8
  constexpr int kRowsPerDma = 64 / kChunksPerRow;   // rows covered by one wave-instruction: 4 or 8
  constexpr int kDmaPerWave = kWgRows / 4 / kRowsPerDma;  // instructions per wave per operand per slice: 2 or 1
  extern __shared__ __attribute__((aligned(16))) char smem_w[];
  // [2][32][64] dY slice, [2][32][64] A slice
  T* Ds = reinterpret_cast<T*>(smem_w);
  T* As = Ds + 2 * kWgRows * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const int tile_k = blockIdx.x % p.tiles_k;
  const int tile_c = blockIdx.x / p.tiles_k;
  const int co0 = tile_c * 64;
  const int k0 = tile_k * 64;
  const int m_lo = blockIdx.y * p.rows_per_chunk;
  const int m_hi = min(m_lo + p.rows_per_chunk, p.M);
  if (m_lo >= m_hi) return;

  const u32x4_t rsX = make_rsrc_t(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc_t(p.dy, dy_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem_w;

  // staging: lane -> (row within the instruction, 16-byte chunk of the 64-element row)
  const int srow = lane / kChunksPerRow;
  const int chunk = lane % kChunksPerRow;
  const int dco = co0 + chunk * kChunkEl;
  const bool dco_ok = dco < p.Cout;          // Cout % kChunkEl == 0 is required by the host
  const int kk = k0 + chunk * kChunkEl;
  const bool k_ok = kk < p.K;
  const int tap = k_ok ? kk / p.Cin : 0;
  const int ci = kk - tap * p.Cin;
  const int kh = tap / p.KW;
  const int kw = tap - kh * p.KW;

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  auto issue = [&](int m_base, int buf) {
#pragma unroll
    for (int q = 0; q < kDmaPerWave; ++q) {
      const int row0 = 8 * wave + kRowsPerDma * q;      // first row of this instruction within the slice
      const int m = m_base + row0 + srow;
      unsigned doff = kOOB, aoff = kOOB;
      if (m < m_hi) {
        if (dco_ok) doff = (unsigned)((((int64_t)m * p.dy_cs) + p.dy_co + dco) * ES);
        if (k_ok) {
          const int hw = p.Ho * p.Wo;
          const int n = fd_div(m, p.fd_hw);
          const int rm = m - n * hw;
          const int ho = fd_div(rm, p.fd_wo);
          const int wo = rm - ho * p.Wo;
          const int hi = ho * p.stride - p.pad + kh;
          const int wi = wo * p.stride - p.pad + kw;
          if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
            aoff = (unsigned)(((((int64_t)n * p.H + hi) * p.W + wi) * p.x_cs + p.x_co + ci) * ES);
        }
      }
      const unsigned lrow = (unsigned)((buf * kWgRows + row0) * 64 * ES);
      lds_dma16_t(rsD, lds_base + lrow, doff, 0u);
      lds_dma16_t(rsX, lds_base + (unsigned)(2 * kWgRows * 64 * ES) + lrow, aoff, 0u);
    }
  };

  const int nslices = (m_hi - m_lo + kWgRows - 1) / kWgRows;
  issue(m_lo, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int s = 0; s < nslices; ++s) {
    const int buf = s & 1;
    if (s + 1 < nslices) issue(m_lo + (s + 1) * kWgRows, buf ^ 1);
    const T* ds = Ds + buf * kWgRows * 64 + wm * 32 + r;   // dY^T operand: [m][co]
    const T* as = As + buf * kWgRows * 64 + wn * 32 + r;   // A operand:    [m][k]
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < kWgRows / 2; ++t) {
      const float a = (float)ds[(2 * t + h) * 64];
      const float b = (float)as[(2 * t + h) * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  // D[row = co][col = k]: row = (e&3) + 8*(e>>2) + 4*h, col = r
  const int kcol = k0 + wn * 32 + r;
  if (kcol < p.K) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int co = co0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (co < p.Cout) {
        if (p.ws) p.ws[(size_t)blockIdx.y * p.ws_stride + (size_t)co * p.K + kcol] = acc[e];
        else atomicAdd(&p.dw[(size_t)co * p.K + kcol], acc[e]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// Weight gradient on the 16-bit MFMA (v_mfma_f32_32x32x16_{f16,bf16}).
// Both operands of  dW[co][k] = sum_m dY[m][co] * A[m][k]  have the reduction index m as their
// SLOW memory dimension (NHWC: channels contiguous), while an MFMA lane needs 8 consecutive m of
// one column.  The slices therefore go global -> LDS row-major by LDS-DMA ([m][128 columns], 256-byte
// rows) and come out transposed through ds_read_b64_tr_b16: per 16-lane group a 4 (m) x 16 (column)
// block, lane i receiving column i -- two such reads are one lane's 8-element MFMA operand.
// Chunk swizzle (cdna_hip_programming.md T10, image (b)): the 16-byte chunk ch of row `row` lives at
// ch ^ (((row&3)<<2) | ((row>>2)&3)), applied on the DMA source side and in the read addresses;
// without it the four rows of a block share 16 banks.
// A workgroup (4 waves, 2x2, each 64 co x 64 k = 4 accumulator tiles) owns a 128 x 128 tile of dW
// and one chunk of the M reduction, 64 rows per slice, double-buffered (64 KB of LDS).
// ---------------------------------------------------------------------------------
constexpr int kWhRows = 64;    // reduction rows per slice
constexpr int kWhTile = 128;   // dW tile edge (co and k)

template <bool BF16, int NBUF>
__global__ __launch_bounds__(256, NBUF == 2 ? 2 : 1) void conv_wgrad_h16_kernel(WgradArgs p, unsigned x_bytes, unsigned dy_bytes) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(3))) s16x4_t* lds_v4_t;
  extern __shared__ __attribute__((aligned(16))) char smem_wh[];
  constexpr int kRowB = 256;                                  // 128 columns x 2 bytes
  constexpr int kOpBytes = kWhRows * kRowB;                   // one operand, one buffer: 16 KB
  // layout: [buf][operand (0 = dY, 1 = A)][64 rows][256 B]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  int tile_id, chunk;
  if (!wgrad_tile_chunk(p.tiles, p.chunks, p.xcd_map, tile_id, chunk)) return;
  const int tile_k = tile_id % p.tiles_k;
  const int tile_c = tile_id / p.tiles_k;
  const int co0 = tile_c * kWhTile;
  const int k0 = tile_k * kWhTile;
  const int m_lo = chunk * p.rows_per_chunk;
  const int m_hi = min(m_lo + p.rows_per_chunk, p.M);
  if (m_lo >= m_hi) return;

  const u32x4_t rsX = make_rsrc_t(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc_t(p.dy, dy_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem_wh;

  // ---- staging: instruction q of this wave fills rows 16*wave + 4q + lane/16, physical chunk lane%16
  const int srow = lane >> 4;
  const int pc = lane & 15;
  int d_col[4];            // dY column offset (elements) of the logical chunk, or -1
  int a_tap[4], a_kh[4], a_kw[4], a_ci[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lc = pc ^ ((srow << 2) | q);                    // swizzle: row&3 = srow, (row>>2)&3 = q
    const int co = co0 + lc * 8;
    d_col[q] = co < p.Cout ? co : -1;                          // Cout % 8 == 0 (host)
    const int kk = k0 + lc * 8;
    if (kk < p.K) {
      const int tap = kk / p.Cin;
      a_tap[q] = tap;
      a_ci[q] = kk - tap * p.Cin;
      a_kh[q] = tap / p.KW;
      a_kw[q] = tap - a_kh[q] * p.KW;
    } else {
      a_tap[q] = -1; a_ci[q] = 0; a_kh[q] = 0; a_kw[q] = 0;
    }
  }

  // (a slice past the end of the chunk is issued all the same, every lane out of range: the count of outstanding
  // instructions the waits below rely on stays fixed)
  // No branches in here: every lane decodes its four rows the same way and SELECTS between its offset and the
  // out-of-range one (the nested ifs and the wrap loop of the first form compiled to a dozen divergent branches per
  // slice in front of the fragment reads).
  auto issue = [&](int m_base, int buf) {
    const int hw = p.Ho * p.Wo;
    const unsigned lrow0 = (unsigned)(buf * 2 * kOpBytes + (16 * wave) * kRowB);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m_base + 16 * wave + srow + 4 * q;
      const int n = fd_div(m, p.fd_hw);
      const int rm = m - n * hw;
      const int ho = fd_div(rm, p.fd_wo);
      const int wo = rm - ho * p.Wo;
      const bool rowok = m < m_hi;
      const int hi = ho * p.stride - p.pad + a_kh[q];
      const int wi = wo * p.stride - p.pad + a_kw[q];
      const bool dok = rowok && d_col[q] >= 0;
      const bool aok = rowok && a_tap[q] >= 0 && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      const unsigned dval = (unsigned)m * (unsigned)(p.dy_cs * 2) + (unsigned)((p.dy_co + d_col[q]) * 2);
      const unsigned aval = (unsigned)((n * p.H + hi) * p.W + wi) * (unsigned)(p.x_cs * 2) + (unsigned)((p.x_co + a_ci[q]) * 2);
      const unsigned doff = dok ? dval : kOOB;
      const unsigned aoff = aok ? aval : kOOB;
      const unsigned lrow = lrow0 + (unsigned)(4 * q * kRowB);
      lds_dma16_t(rsD, lds_base + lrow, doff, 0u);
      lds_dma16_t(rsX, lds_base + (unsigned)kOpBytes + lrow, aoff, 0u);
    }
  };

  // ---- transposed fragment reads ----
  // lane = 16g + i: h = g>>1 (k half of the MFMA step), colhalf = g&1; inside the group lane 4q'+pp
  // addresses row q' of the block, columns 4pp..4pp+3
  const int g = lane >> 4, i16 = lane & 15;
  const int hh = g >> 1, colhalf = g & 1;
  const int qq = i16 >> 2, pp = i16 & 3;
  // byte offset inside an operand buffer of (block row m0 + qq, column c0 + 4pp), m0 = 16s + 8hh + 4j:
  //   256*(m0+qq) + 16*((c0/8 + (pp>>1)) ^ ((qq<<2) | ((2hh + j)&3))) + 8*(pp&1)
  auto frag_addr = [&](int col_base, int s, int j) -> unsigned {
    const int m0 = 16 * s + 8 * hh + 4 * j;
    const int chunk = (col_base + 16 * colhalf) / 8 + (pp >> 1);
    const int swz = (qq << 2) | ((2 * hh + j) & 3);
    return (unsigned)(kRowB * (m0 + qq) + 16 * (chunk ^ swz) + 8 * (pp & 1));
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  // NBUF slice buffers, NBUF - 1 slices of LDS-DMA in flight.  A 128 x 128 tile spends ~500 cycles of MFMA on a slice
  // whose 32 KB take the memory system several times that to deliver: the kernel runs at (bytes in flight) / latency.
  // NBUF = 2 (two workgroups per CU, each waiting out its one outstanding slice) keeps 2 x 32 KB in flight per CU,
  // NBUF = 4 (one workgroup, 128 KB of LDS) three slices -- and never drains the queue: the wait in front of slice s
  // leaves the (NBUF - 2) younger slices outstanding (8 DMA instructions per wave and slice).
  const int nslices = (m_hi - m_lo + kWhRows - 1) / kWhRows;
#pragma unroll
  for (int s0 = 0; s0 < NBUF - 1; ++s0) issue(m_lo + s0 * kWhRows, s0);
  for (int sl = 0; sl < nslices; ++sl) {
    const int buf = sl % NBUF;
    if (NBUF == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (NBUF == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (NBUF == 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // slice sl is in LDS; every wave is done with slice sl - 1
    asm volatile("" ::: "memory");
    issue(m_lo + (sl + NBUF - 1) * kWhRows, (sl + NBUF - 1) % NBUF);        // into the buffer slice sl - 1 left
    char* dbuf = smem_wh + buf * 2 * kOpBytes;
    char* abuf = dbuf + kOpBytes;
    __builtin_amdgcn_s_setprio(1);
    // two fragment sets: the eight reads of step s + 1 are issued in front of the four MFMAs of step s (one set, as the
    // compiler schedules the plain loop, makes every step wait out a fresh LDS round trip)
    s16x8_t fa[2][2], fb[2][2];
#define YV4_WH_LOAD(SET, S)                                                                                           \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                   \
      const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(dbuf + frag_addr(wm * 64 + t * 32, S, 0))); \
      const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(dbuf + frag_addr(wm * 64 + t * 32, S, 1))); \
      const s16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(abuf + frag_addr(wn * 64 + t * 32, S, 0))); \
      const s16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(abuf + frag_addr(wn * 64 + t * 32, S, 1))); \
      fa[SET][t] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);                                          \
      fb[SET][t] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);                                          \
    }
#define YV4_WH_MFMA(SET)                                                                                              \
    _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                                     \
      _Pragma("unroll") for (int b = 0; b < 2; ++b) {                                                                 \
        if (BF16)                                                                                                     \
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_w, fa[SET][a]),               \
                                                              __builtin_bit_cast(bf16x8_w, fb[SET][b]), acc[a][b], 0, 0, 0); \
        else                                                                                                          \
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_w, fa[SET][a]),                 \
                                                             __builtin_bit_cast(f16x8_w, fb[SET][b]), acc[a][b], 0, 0, 0);   \
      }                                                                                                               \
    __builtin_amdgcn_sched_barrier(0);
    static_assert(kWhRows / 16 == 4, "the step schedule below is written for four 16-row steps");
    YV4_WH_LOAD(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WH_LOAD(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WH_MFMA(0);
    YV4_WH_LOAD(0, 2);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WH_MFMA(1);
    YV4_WH_LOAD(1, 3);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WH_MFMA(0);
    YV4_WH_MFMA(1);
#undef YV4_WH_MFMA
#undef YV4_WH_LOAD
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the out-of-range slices issued past the end
  // D[row = co][col = k]: row = (e&3) + 8*(e>>2) + 4*(lane>>5), col = lane&31
  const int r = lane & 31, h5 = lane >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int kcol = k0 + wn * 64 + b * 32 + r;
      if (kcol >= p.K) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h5;
        if (co < p.Cout) {
          if (p.ws) p.ws[(size_t)chunk * p.ws_stride + (size_t)co * p.K + kcol] = acc[a][b][e];
          else atomicAdd(&p.dw[(size_t)co * p.K + kcol], acc[a][b][e]);
        }
      }
    }
}

// ---------------------------------------------------------------------------------
// The kernel above with its staging arithmetic removed from the lanes (round 5).  Per 64-row slice and wave the loop
// above issues 16 MFMAs (512 matrix-pipe cycles) and 119 VALU instructions of which 40 are 32-bit integer multiplies
// (quarter rate: 16 issue cycles each) -- the row decode (two divisions by invariant divisors) and the byte offsets of
// four rows per lane, rebuilt from the row index every slice: ~960 cycles of vector issue per 512 of matrix work, two
// waves per SIMD.  Here:
//   * LINEAR (1x1, stride 1, no padding -- 27 of YOLOv4-L's layers): both operands' offsets advance by a constant per
//     slice and are range-checked as offsets against lane-constant limits: an add, a compare and a select per piece;
//   * otherwise one wave decodes each of the slice's 64 rows ONCE (64 lanes = 64 rows) two slices ahead and leaves
//     {byte offset of the row's window origin, (hi0, wi0)} in an LDS table beside the slice buffers; a lane reads the
//     entries of its four rows, adds its taps' lane-constant offset and checks the window bounds -- no division, no multiply.
// Same tiles, same MFMAs in the same order, same slab output: dW is bit-identical to the kernel above.
// ---------------------------------------------------------------------------------
constexpr int kWhLds2 = 2 * 2 * kWhRows * 256;       // two slice buffers
constexpr int kWhTabBytes = kWhRows * 8;             // one row table
constexpr int kWhLdsV2 = kWhLds2 + 3 * kWhTabBytes;       // three tables: a slice's entries are read a slice ahead of its DMA

template <bool BF16, bool LINEAR>
__global__ __launch_bounds__(256, 2) void conv_wgrad_v2_h16_kernel(WgradArgs p, unsigned x_bytes, unsigned dy_bytes) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(3))) s16x4_t* lds_v4_t;
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) u32x2_t* lds_u2_t;
  extern __shared__ __attribute__((aligned(16))) char smem_wv[];
  constexpr int kRowB = 256;
  constexpr int kOpBytes = kWhRows * kRowB;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  int tile_id, chunk;
  if (!wgrad_tile_chunk(p.tiles, p.chunks, p.xcd_map, tile_id, chunk)) return;
  const int tile_k = tile_id % p.tiles_k;
  const int tile_c = tile_id / p.tiles_k;
  const int co0 = tile_c * kWhTile;
  const int k0 = tile_k * kWhTile;
  const int m_lo = chunk * p.rows_per_chunk;
  const int m_hi = min(m_lo + p.rows_per_chunk, p.M);
  if (m_lo >= m_hi) return;

  const u32x4_t rsX = make_rsrc_t(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc_t(p.dy, dy_bytes);
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  const unsigned lds_base = (unsigned)(unsigned long long)(lds_ptr_t)smem_wv;

  // ---- staging: instruction q of this wave fills rows 16*wave + 4q + lane/16, physical chunk lane%16
  const int srow = lane >> 4;
  const int pc = lane & 15;
  const unsigned d_step = (unsigned)(kWhRows * p.dy_cs * 2), x_step = (unsigned)(kWhRows * p.x_cs * 2);
  unsigned d_off[4], d_lim[4];       // dY: byte offset of this lane's 16 bytes at slice 0, and its limit (0: never)
  unsigned a_off[4], a_lim[4];       // LINEAR: the same for the activation
  unsigned a_tap[4];                 // general: byte offset of the lane's (tap, channel chunk) from the row's window origin
  int a_kh[4], a_kw[4];              // general: the tap (kh = -30000 for a column beyond K: never inside the map)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lc = pc ^ ((srow << 2) | q);                    // swizzle: row&3 = srow, (row>>2)&3 = q
    const int row = 16 * wave + srow + 4 * q;
    const int co = co0 + lc * 8;
    const unsigned cb = (unsigned)((p.dy_co + co) * 2);
    d_off[q] = (unsigned)(m_lo + row) * (unsigned)(p.dy_cs * 2) + cb;
    d_lim[q] = co < p.Cout ? (unsigned)m_hi * (unsigned)(p.dy_cs * 2) + cb : 0u;
    const int kk = k0 + lc * 8;
    int tap = 0, ci = 0;
    const bool kok = kk < p.K;
    if (kok) { tap = kk / p.Cin; ci = kk - tap * p.Cin; }
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const unsigned xb_ = (unsigned)((p.x_co + ci) * 2);
    if (LINEAR) {      // tap 0 only; input pixel = output pixel
      a_off[q] = (unsigned)(m_lo + row) * (unsigned)(p.x_cs * 2) + xb_;
      a_lim[q] = kok ? (unsigned)m_hi * (unsigned)(p.x_cs * 2) + xb_ : 0u;
    } else {
      a_kh[q] = kok ? kh : -30000;
      a_kw[q] = kw;
      a_tap[q] = (unsigned)(kh * p.W + kw) * (unsigned)(p.x_cs * 2) + xb_;
    }
  }
  // general form: the row table.  Entry of slice row r: {byte offset of input pixel (n, ho*s - p, wo*s - p) -- may be in
  // front of the map: arithmetic modulo 2^32 --, (hi0 << 16) | (wi0 & 0xFFFF)}; rows past the chunk get hi0 = -30000.
  int t_m = m_lo + lane;             // (wave 0) the row this lane decodes next
  auto table = [&](int sl) {
    if (LINEAR || wave != 0) return;
    unsigned off0 = 0u;
    int hi0 = -30000, wi0 = 0;
    if (t_m < m_hi) {
      const int n = fd_div(t_m, p.fd_hw);
      const int rm = t_m - n * (p.Ho * p.Wo);
      const int ho = fd_div(rm, p.fd_wo);
      const int wo = rm - ho * p.Wo;
      hi0 = ho * p.stride - p.pad;
      wi0 = wo * p.stride - p.pad;
      off0 = (unsigned)((n * p.H + hi0) * p.W + wi0) * (unsigned)(p.x_cs * 2);
    }
    u32x2_t ent;
    ent.x = off0;
    ent.y = ((unsigned)hi0 << 16) | ((unsigned)wi0 & 0xFFFFu);
    *(lds_u2_t)(smem_wv + kWhLds2 + (sl % 3) * kWhTabBytes + lane * 8) = ent;
    t_m += kWhRows;
  };
  // the table entries of this lane's four rows of slice `sl`: fetched a whole slice ahead of the DMA that uses them (an LDS
  // round trip in front of every slice's issue cost the streaming layers 7 %)
  u32x2_t te[4] = {};
  auto fetch = [&](int sl) {
    if (LINEAR) return;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      te[q] = *(lds_u2_t)(smem_wv + kWhLds2 + (sl % 3) * kWhTabBytes + (16 * wave + srow + 4 * q) * 8);
  };
  auto issue = [&](int sl) {
    const int buf = sl & 1;
    const unsigned lrow0 = (unsigned)(buf * 2 * kOpBytes + (16 * wave) * kRowB);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned lrow = lrow0 + (unsigned)(4 * q * kRowB);
      lds_dma16_t(rsD, lds_base + lrow, d_off[q] < d_lim[q] ? d_off[q] : kOOB, 0u);
      d_off[q] += d_step;
      unsigned aoff;
      if (LINEAR) {
        aoff = a_off[q] < a_lim[q] ? a_off[q] : kOOB;
        a_off[q] += x_step;
      } else {
        const int hi = ((int)te[q].y >> 16) + a_kh[q];
        const int wi = (int)(short)(te[q].y & 0xFFFFu) + a_kw[q];
        aoff = ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) ? te[q].x + a_tap[q] : kOOB;
      }
      lds_dma16_t(rsX, lds_base + (unsigned)kOpBytes + lrow, aoff, 0u);
    }
  };

  // ---- transposed fragment reads (conv_wgrad_h16_kernel)
  const int g = lane >> 4, i16 = lane & 15;
  const int hh = g >> 1, colhalf = g & 1;
  const int qq = i16 >> 2, pp = i16 & 3;
  auto frag_addr = [&](int col_base, int s_, int j) -> unsigned {
    const int m0 = 16 * s_ + 8 * hh + 4 * j;
    const int chunk_ = (col_base + 16 * colhalf) / 8 + (pp >> 1);
    const int swz = (qq << 2) | ((2 * hh + j) & 3);
    return (unsigned)(kRowB * (m0 + qq) + 16 * (chunk_ ^ swz) + 8 * (pp & 1));
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int nslices = (m_hi - m_lo + kWhRows - 1) / kWhRows;
  table(0);
  table(1);
  table(2);
  if (!LINEAR) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  fetch(0);
  issue(0);
  fetch(1);
  for (int sl = 0; sl < nslices; ++sl) {
    const int buf = sl & 1;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // slice sl is in LDS (and table sl + 2); every wave is done with slice sl - 1
    asm volatile("" ::: "memory");
    issue(sl + 1);                                   // into the buffer slice sl - 1 left; its table entries are in registers
    table(sl + 3);                                   // into the table whose entries (slice sl) every wave fetched two barriers ago
    fetch(sl + 2);                                   // written during slice sl - 1, visible since the barrier above
    char* dbuf = smem_wv + buf * 2 * kOpBytes;
    char* abuf = dbuf + kOpBytes;
    __builtin_amdgcn_s_setprio(1);
    s16x8_t fa[2][2], fb[2][2];
#define YV4_WV_LOAD(SET, S)                                                                                           \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                   \
      const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(dbuf + frag_addr(wm * 64 + t * 32, S, 0))); \
      const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(dbuf + frag_addr(wm * 64 + t * 32, S, 1))); \
      const s16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(abuf + frag_addr(wn * 64 + t * 32, S, 0))); \
      const s16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(abuf + frag_addr(wn * 64 + t * 32, S, 1))); \
      fa[SET][t] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);                                          \
      fb[SET][t] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);                                          \
    }
#define YV4_WV_MFMA(SET)                                                                                              \
    _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                                     \
      _Pragma("unroll") for (int b = 0; b < 2; ++b) {                                                                 \
        if (BF16)                                                                                                     \
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_w, fa[SET][a]),               \
                                                              __builtin_bit_cast(bf16x8_w, fb[SET][b]), acc[a][b], 0, 0, 0); \
        else                                                                                                          \
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_w, fa[SET][a]),                 \
                                                             __builtin_bit_cast(f16x8_w, fb[SET][b]), acc[a][b], 0, 0, 0);   \
      }                                                                                                               \
    __builtin_amdgcn_sched_barrier(0);
    YV4_WV_LOAD(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WV_LOAD(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WV_MFMA(0);
    YV4_WV_LOAD(0, 2);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WV_MFMA(1);
    YV4_WV_LOAD(1, 3);
    __builtin_amdgcn_sched_barrier(0);
    YV4_WV_MFMA(0);
    YV4_WV_MFMA(1);
#undef YV4_WV_MFMA
#undef YV4_WV_LOAD
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the out-of-range slice issued past the end
  const int r = lane & 31, h5 = lane >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int kcol = k0 + wn * 64 + b * 32 + r;
      if (kcol >= p.K) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h5;
        if (co < p.Cout) {
          if (p.ws) p.ws[(size_t)chunk * p.ws_stride + (size_t)co * p.K + kcol] = acc[a][b][e];
          else atomicAdd(&p.dw[(size_t)co * p.K + kcol], acc[a][b][e]);
        }
      }
    }
}

// dw[i] += sum over chunks of slab_c[i], in a FIXED order: the deterministic tail of the weight gradient.
// A workgroup owns 16 float4 columns; its 16 chunk lanes q each add the slabs c = q, q + 16, q + 32, ... in ascending
// order (independent loads, 4 in flight), the 16 lane sums are then added in lane order.  (One thread per column
// walking all chunks serially was latency-bound on the 1x1 layers: 361 chunks of a 64 KB dW took 100 us.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, int chunks, long long stride,
                                                           long long n, float* __restrict__ dw) {
  __shared__ float4 part[16][16];
  const long long n4 = n >> 2;
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4;
  const long long col = (long long)blockIdx.x * 16 + cl;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < n4) {
    const float* base = ws + 4 * col;
    int c = q;
    for (; c + 48 < chunks; c += 64) {
      const float4 b0 = *reinterpret_cast<const float4*>(base + (size_t)c * stride);
      const float4 b1 = *reinterpret_cast<const float4*>(base + (size_t)(c + 16) * stride);
      const float4 b2 = *reinterpret_cast<const float4*>(base + (size_t)(c + 32) * stride);
      const float4 b3 = *reinterpret_cast<const float4*>(base + (size_t)(c + 48) * stride);
      a.x += b0.x; a.y += b0.y; a.z += b0.z; a.w += b0.w;
      a.x += b1.x; a.y += b1.y; a.z += b1.z; a.w += b1.w;
      a.x += b2.x; a.y += b2.y; a.z += b2.z; a.w += b2.w;
      a.x += b3.x; a.y += b3.y; a.z += b3.z; a.w += b3.w;
    }
    for (; c < chunks; c += 16) {
      const float4 b = *reinterpret_cast<const float4*>(base + (size_t)c * stride);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
  }
  part[q][cl] = a;
  __syncthreads();
  if (q == 0 && col < n4) {
    float4 t = part[0][cl];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
      const float4 b = part[k][cl];
      t.x += b.x; t.y += b.y; t.z += b.z; t.w += b.w;
    }
    float4 d = reinterpret_cast<float4*>(dw)[col];
    d.x += t.x; d.y += t.y; d.z += t.z; d.w += t.w;
    reinterpret_cast<float4*>(dw)[col] = d;
  }
}

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

// test / ablation switch: route 16-bit inputs through the widening fp32-MFMA kernel instead of the
// 16-bit MFMA one (YV4_WGRAD_WIDEN=1 in the environment)
static const bool g_wgrad_widen = YV4_ENV_INT("YV4_WGRAD_WIDEN", 0) == 1;
// measurement switch: the XCD-aware (tile, chunk) mapping of the 16-bit weight-gradient kernels (wgrad_tile_chunk)
static const bool g_wgrad_xcd = YV4_ENV_INT("YV4_WGRAD_XCD", 1) != 0;

// split of the M reduction into chunks (shared by the launch and by yv4_conv_wgrad_workspace)
static void wgrad_chunks(const yv4_conv_desc* d, int dtype, long long* chunks, long long* rows) {
  const long long M = (long long)d->N * d->Ho * d->Wo;
  const int K = d->KH * d->KW * d->Cin;
  if (!g_wgrad_widen && wgrad_fc_cin(d, dtype)) {
    // one round of workgroups (two per CU; one for Cin 64), every one with at least four slices (wgrad_fc_cin)
    long long ch = wgrad_fc_cin(d, dtype) == 64 ? 256 : 512;
    long long rw = (M + ch - 1) / ch;
    rw = (rw + kFcRows - 1) / kFcRows * kFcRows;
    *rows = rw;
    *chunks = (M + rw - 1) / rw;
    return;
  }
  if (!g_wgrad_widen && wgrad3x3_applies(d, dtype)) {
    // one 8-wave workgroup per CU.  Measured (tools/wgrad_bench.py --det, batch 64): ONE full round of (co tile, kh, ci
    // tile, chunk) workgroups beats two (half the slab traffic and epilogues: 160 vs 179 us on 128->128 @76) unless the
    // tiles leave more than ~10 % of the CUs idle (512->1024 @19: 96 tiles x 2 chunks = 192 workgroups, 403 vs 342 us);
    // never one workgroup beyond a full round (it costs a whole round).
    const long long tl = (long long)((d->Cout + 127) / 128) * 3 * (d->Cin / 128);
    static const int cus = YV4_ENV_INT("YV4_WGRAD3_CUS", 256);
    long long ch = cus / tl;
    if (ch < 1 || tl * ch * 10 < (long long)cus * 9) ch = (2 * cus) / tl;
    const long long mx = (M + 8 * kW3Rows - 1) / (8 * kW3Rows);
    if (ch > mx) ch = mx;
    if (ch < 1) ch = 1;
    if (ch > 65535) ch = 65535;
    // XCD-aware mapping (wgrad_tile_chunk): a chunk's tiles on ONE XCD need the chunk count in whole groups of eight
    if (w3_xcd_map(tl, ch)) ch = ch / 8 * 8;
    long long rw = (M + ch - 1) / ch;
    rw = (rw + kW3Rows - 1) / kW3Rows * kW3Rows;
    *rows = rw;
    *chunks = (M + rw - 1) / rw;
    return;
  }
  if (dtype != YV4_F32 && !g_wgrad_widen) {
    const long long tl = (long long)((K + kWhTile - 1) / kWhTile) * ((d->Cout + kWhTile - 1) / kWhTile);
    // Chunks of the reduction: ONE round of two workgroups per CU and never a workgroup more (513 workgroups take two
    // rounds).  Measured over YOLOv4-L at batch 64 (tools/wgrad_bench.py --det, measure build, YV4_WGRAD_WGS): 512 beats
    // 1024 on every 1x1 layer (half the partial-sum slabs: 512->256 @38 56 -> 47 us) and on the stride-2 layers, network
    // 505 -> 525 TFLOP/s.  A dW of more than half a round of tiles cannot fill one round: then the chunk count with the
    // least (rounds / chunks), the smallest within 20 % of it (512->1024 s2 @38: 288 tiles x 3 chunks, 383 -> 312 us).
    static const int wg_target = YV4_ENV_INT("YV4_WGRAD_WGS", 512);
    static const int min_slices = YV4_ENV_INT("YV4_WGRAD_MINSL", 16);
    const long long mx = (M + min_slices * kWhRows - 1) / (min_slices * kWhRows);   // at least min_slices per chunk
    long long ch = wg_target / tl;
    if (2 * tl > wg_target) {
      const long long chmax = 4 * wg_target / tl > 1 ? 4 * wg_target / tl : 1;
      double best = 1e30;
      for (long long c = 1; c <= chmax; ++c) {
        const double sc = (double)((tl * c + wg_target - 1) / wg_target) / (double)c;
        if (sc < best) best = sc;
      }
      for (long long c = 1; c <= chmax; ++c)
        if ((double)((tl * c + wg_target - 1) / wg_target) / (double)c <= 1.2 * best) { ch = c; break; }
    }
    if (ch > mx) ch = mx;
    if (ch < 1) ch = 1;
    if (tl >= 2 && ch >= 16 && d->Cout >= 128) ch = ch / 8 * 8;   // whole groups of 8 chunks, one per XCD (wgrad_tile_chunk)
    if (ch > 65528) ch = 65528;
    long long rw = (M + ch - 1) / ch;
    rw = (rw + kWhRows - 1) / kWhRows * kWhRows;
    *rows = rw;
    *chunks = (M + rw - 1) / rw;
    return;
  }
  const long long tiles = (long long)((K + 63) / 64) * ((d->Cout + 63) / 64);
  long long ch = (256 * 4 + tiles - 1) / tiles;            // ~4 workgroups per CU, at least 8 slices each
  const long long mx = (M + 8 * kWgRows - 1) / (8 * kWgRows);
  if (ch > mx) ch = mx;
  if (ch < 1) ch = 1;
  if (ch > 65535) ch = 65535;
  long long rw = (M + ch - 1) / ch;
  rw = (rw + kWgRows - 1) / kWgRows * kWgRows;
  *rows = rw;
  *chunks = (M + rw - 1) / rw;
}

static int wgrad_impl(const yv4_conv_desc* d, int dtype, const void* x, const void* dy, float* dw, void* stream,
                      float* ws = nullptr, size_t ws_bytes = 0) {
  YV4_REQUIRE(d && x && dy && dw, "wgrad: null argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "wgrad: dtype must be f32, f16 or bf16");
  const int al = dtype == YV4_F32 ? 4 : 8;
  const int es = dtype == YV4_F32 ? 4 : 2;
  YV4_REQUIRE(d->Cin % al == 0 && d->x_cstride % al == 0 && d->x_coff % al == 0,
              "wgrad: input channels/stride/offset must be multiples of %d", al);
  YV4_REQUIRE(d->Cout % al == 0 && d->y_cstride % al == 0 && d->y_coff % al == 0,
              "wgrad: dY channels/stride/offset must be multiples of %d", al);
  YV4_REQUIRE(d->KH > 0 && d->KW > 0 && d->KH * d->KW <= 64 && d->stride > 0, "wgrad: bad kernel/stride");
  const int Ho = (d->H + 2 * d->pad - d->KH) / d->stride + 1;
  const int Wo = (d->W + 2 * d->pad - d->KW) / d->stride + 1;
  YV4_REQUIRE(Ho == d->Ho && Wo == d->Wo, "wgrad: Ho/Wo do not match the geometry");
  const long long M = (long long)d->N * d->Ho * d->Wo;
  const long long xb = (long long)d->N * d->H * d->W * d->x_cstride * es, db = M * d->y_cstride * es;
  YV4_REQUIRE(M < (1LL << 31) && xb < 0xFFFFFFF0LL && db < 0xFFFFFFF0LL, "wgrad: tensors of 4 GiB or more are not supported");
  WgradArgs a;
  a.x = x; a.dy = dy; a.dw = dw;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
  a.x_cs = d->x_cstride; a.x_co = d->x_coff; a.dy_cs = d->y_cstride; a.dy_co = d->y_coff;
  a.M = (int)M; a.K = d->KH * d->KW * d->Cin;
  a.fd_hw = make_fastdiv((unsigned)(d->Ho * d->Wo));
  a.fd_wo = make_fastdiv((unsigned)d->Wo);
  long long ch = 1, rw = M;
  wgrad_chunks(d, dtype, &ch, &rw);
  a.rows_per_chunk = (int)rw;
  const long long dw_elems = (long long)a.Cout * a.K;
  if (ws && ch > 1) {
    YV4_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)dw & 15) == 0 && dw_elems % 4 == 0,
                "wgrad: workspace / dw must be 16-byte aligned and Cout*K a multiple of 4");
    YV4_REQUIRE(ws_bytes >= (size_t)ch * dw_elems * sizeof(float), "wgrad: workspace too small (%zu bytes for %lld chunks)",
                ws_bytes, ch);
    a.ws = ws;
    a.ws_stride = dw_elems;
  }
  auto finish = [&]() -> int {
    if (!a.ws) return YV4_OK;
    const long long g = (dw_elems / 4 + 15) / 16;
    if (g > 0x7fffffffLL) { set_error("wgrad: dW too large"); return YV4_E_INVALID; }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a.ws, (int)ch,
                       a.ws_stride, dw_elems, dw);
    YV4_CHECK_LAUNCH("conv_wgrad reduce");
    return YV4_OK;
  };
  // (the second forms range-check 32-bit byte OFFSETS: both maps below 3 GB.  Beyond that the product takes the generic
  // 16-bit kernel further down; the first forms of the two special kernels exist in the measurement build only)
  static const int fcv2 = YV4_ENV_INT("YV4_WFC_V2", 1);
  const bool fc_v2_ok = fcv2 && xb < 0xC0000000LL && db < 0xC0000000LL;
#ifdef YV4_MEASURE
  const bool fc_any = true;
#else
  const bool fc_any = fc_v2_ok;
#endif
  if (const int fc = (g_wgrad_widen || !fc_any) ? 0 : wgrad_fc_cin(d, dtype)) {
    if (int rc = wgrad_fc_launch(a, dtype, fc, xb, db, ch, stream, fc_v2_ok)) return rc;
    return finish();
  }
  static const int w3v2 = YV4_ENV_INT("YV4_W3V2", 1);
  const bool w3_v2_ok = w3v2 && xb < 0xC0000000LL && db < 0xC0000000LL;
#ifdef YV4_MEASURE
  const bool w3_any = true;
#else
  const bool w3_any = w3_v2_ok;
#endif
  if (!g_wgrad_widen && w3_any && wgrad3x3_applies(d, dtype)) {
    if (int rc = wgrad3x3_launch(a, dtype, xb, db, ch, stream, w3_v2_ok)) return rc;
    return finish();
  }
  if (dtype != YV4_F32 && !g_wgrad_widen) {
    // 16-bit MFMA form: 128 x 128 tiles of dW, 64-row slices
    a.tiles_k = (a.K + kWhTile - 1) / kWhTile;
    const int tc = (a.Cout + kWhTile - 1) / kWhTile;
    const long long tl = (long long)a.tiles_k * tc;
    // slice buffers: 2 x two workgroups per CU.  (3 to 5 buffers for ONE workgroup per CU -- more bytes in flight, no
    // queue drain -- are 20-60 % slower on every layer, network 505 -> 408 TFLOP/s: with one wave per SIMD nothing
    // covers a wave's transposed-read -> MFMA chain.  Those instantiations exist in the measure build only.)
    static const int nbuf = YV4_ENV_INT("YV4_WGRAD_NBUF", 2);
    const size_t ldsh = (size_t)nbuf * 2 * kWhRows * 256;
    a.tiles = (int)tl;
    a.chunks = (int)ch;
    // (not for the few-channel layers at 304 / 608 pixels -- Cout < 128, half-empty dY tiles, pure streaming: inside the
    // training step they ran 25 % slower with it, tools/train_timeline.py)
    a.xcd_map = g_wgrad_xcd && tl >= 2 && ch >= 16 && a.Cout >= 128 && tl * (ch + 8) < (1LL << 31) ? 1 : 0;
    const dim3 grid = wgrad_grid(tl, ch, a.xcd_map);
    hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    static const int whv2 = YV4_ENV_INT("YV4_WGRAD_V2", 1);
    const bool linear = d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0;
    // (second form: offsets are range-checked as 32-bit byte offsets, window origins travel as 16-bit coordinates.  Not for
    // the few-channel windowed layers -- 32 -> 64 s2 @608 streams 2.3 GB through 288 columns of dW and is bound by its
    // bytes: the table's LDS round trip in front of every slice's DMA cost it 7 %, 836 -> 894 us)
    static const int whv2_min_cin = YV4_ENV_INT("YV4_WGRAD_V2_MINCIN", 64);
    if (whv2 && nbuf == 2 && xb < 0xC0000000LL && db < 0xC0000000LL && d->H < 16000 && d->W < 16000 &&
        (linear || d->Cin >= whv2_min_cin)) {
#define YV4_WV_LAUNCH(LIN)                                                                                             \
  {                                                                                                                    \
    static LdsAttrOnce once_b, once_h;                                                                                 \
    if (int rc = ensure_dyn_lds(once_b, reinterpret_cast<const void*>(conv_wgrad_v2_h16_kernel<true, LIN>), (size_t)kWhLdsV2, "conv_wgrad_v2_h16")) return rc;  \
    if (int rc = ensure_dyn_lds(once_h, reinterpret_cast<const void*>(conv_wgrad_v2_h16_kernel<false, LIN>), (size_t)kWhLdsV2, "conv_wgrad_v2_h16")) return rc; \
    if (dtype == YV4_BF16) hipLaunchKernelGGL((conv_wgrad_v2_h16_kernel<true, LIN>), grid, dim3(256), (size_t)kWhLdsV2, hs, a, (unsigned)xb, (unsigned)db);     \
    else hipLaunchKernelGGL((conv_wgrad_v2_h16_kernel<false, LIN>), grid, dim3(256), (size_t)kWhLdsV2, hs, a, (unsigned)xb, (unsigned)db);                      \
  }
      if (linear) YV4_WV_LAUNCH(true)
      else YV4_WV_LAUNCH(false)
#undef YV4_WV_LAUNCH
      YV4_CHECK_LAUNCH("conv_wgrad_v2_h16");
      return finish();
    }
#define YV4_WH_LAUNCH(NB)                                                                                              \
  {                                                                                                                    \
    static LdsAttrOnce once_b, once_h;                                                                                 \
    if (int rc = ensure_dyn_lds(once_b, reinterpret_cast<const void*>(conv_wgrad_h16_kernel<true, NB>), ldsh, "conv_wgrad_h16")) return rc;  \
    if (int rc = ensure_dyn_lds(once_h, reinterpret_cast<const void*>(conv_wgrad_h16_kernel<false, NB>), ldsh, "conv_wgrad_h16")) return rc; \
    if (dtype == YV4_BF16) hipLaunchKernelGGL((conv_wgrad_h16_kernel<true, NB>), grid, dim3(256), ldsh, hs, a, (unsigned)xb, (unsigned)db);  \
    else hipLaunchKernelGGL((conv_wgrad_h16_kernel<false, NB>), grid, dim3(256), ldsh, hs, a, (unsigned)xb, (unsigned)db);                  \
  }
#ifdef YV4_MEASURE
    if (nbuf == 3) YV4_WH_LAUNCH(3)
    else if (nbuf == 4) YV4_WH_LAUNCH(4)
    else if (nbuf == 5) YV4_WH_LAUNCH(5)
    else
#endif
    YV4_WH_LAUNCH(2)
#undef YV4_WH_LAUNCH
    YV4_CHECK_LAUNCH("conv_wgrad_h16");
    return finish();
  }
  a.tiles_k = (a.K + 63) / 64;
  const int tiles_c = (a.Cout + 63) / 64;
  const long long tiles = (long long)a.tiles_k * tiles_c;
  const long long chunks = ch;
  const size_t lds = (size_t)4 * kWgRows * 64 * es;
  YV4_DISPATCH_T(dtype, hipLaunchKernelGGL(conv_wgrad_kernel<T>, dim3((unsigned)tiles, (unsigned)chunks), dim3(256), lds,
                                           reinterpret_cast<hipStream_t>(stream), a, (unsigned)xb, (unsigned)db));
  YV4_CHECK_LAUNCH("conv_wgrad");
  return finish();
}

extern "C" int yv4_conv_wgrad(const yv4_conv_desc* d, const float* x, const float* dy, float* dw, void* stream) {
  return wgrad_impl(d, YV4_F32, x, dy, dw, stream);
}
extern "C" int yv4_conv_wgrad_h16(const yv4_conv_desc* d, int dtype, const void* x, const void* dy, float* dw,
                                  void* stream) {
  YV4_REQUIRE(dtype == YV4_F16 || dtype == YV4_BF16, "wgrad_h16: dtype must be YV4_F16 or YV4_BF16");
  return wgrad_impl(d, dtype, x, dy, dw, stream);
}

// Deterministic weight gradient: the chunks of the M reduction store their partials to slabs of `workspace` and one
// small kernel adds them to dw in chunk order -- same accumulate-into-dw contract as yv4_conv_wgrad[_h16], run-to-run
// bit-identical, and the partial exchange moves at store speed instead of the ~1.3 TB/s of float atomics.
extern "C" size_t yv4_conv_wgrad_workspace(const yv4_conv_desc* d, int dtype) {
  if (!d || d->N <= 0 || d->Ho <= 0 || d->Wo <= 0) return 0;
  long long ch = 1, rw = 0;
  wgrad_chunks(d, dtype, &ch, &rw);
  if (ch <= 1) return 0;
  return (size_t)ch * (size_t)d->Cout * (size_t)(d->KH * d->KW * d->Cin) * sizeof(float);
}
extern "C" int yv4_conv_wgrad_det(const yv4_conv_desc* d, int dtype, const void* x, const void* dy, float* dw,
                                  float* workspace, size_t workspace_bytes, void* stream) {
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "wgrad_det: dtype must be f32, f16 or bf16");
  return wgrad_impl(d, dtype, x, dy, dw, stream, workspace, workspace_bytes);
}

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
