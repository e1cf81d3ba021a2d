// The generic convolution weight gradient on gfx950 (fp32 MFMA, 16-bit MFMA and its second form), the deterministic
// slab reduce and the dispatcher over these and the two special 3x3 families (conv_wgrad3x3_h16.hip,
// conv_wgrad_fc_h16.hip).  Weight packing is in pack_weights.hip, the backward halves of the data-movement ops
// (zero-dilation, SPP max-pool, nearest resample) in elementwise_bwd.hip, train-mode BatchNorm in bn_train.hip.
//
// What they replace in the reference's training step:
//   cuDNN conv backward-filter / backward-data  (autograd of mmcv ConvModule, darknetcsp.py:15-35)
// The data gradient itself is the forward kernel again (conv_mfma_f32.hip) on dY with the
// weights transposed and flipped; for stride 2 dY is first zero-dilated (yv4_dilate2_fwd, elementwise_bwd.hip).
#include "train_common.h"
#include "wgrad_common.h"
#include "conv_desc.h"

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

  const u32x4_t rsX = make_rsrc(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc(p.dy, dy_bytes);
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
      lds_dma16(rsD, lds_base + lrow, doff, 0u);
      lds_dma16(rsX, lds_base + (unsigned)(2 * kWgRows * 64 * ES) + lrow, aoff, 0u);
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

  const u32x4_t rsX = make_rsrc(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc(p.dy, dy_bytes);
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
      lds_dma16(rsD, lds_base + lrow, doff, 0u);
      lds_dma16(rsX, lds_base + (unsigned)kOpBytes + lrow, aoff, 0u);
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

  const u32x4_t rsX = make_rsrc(p.x, x_bytes);
  const u32x4_t rsD = make_rsrc(p.dy, dy_bytes);
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
      lds_dma16(rsD, lds_base + lrow, d_off[q] < d_lim[q] ? d_off[q] : kOOB, 0u);
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
      lds_dma16(rsX, lds_base + (unsigned)kOpBytes + lrow, aoff, 0u);
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
  // `ch` chunks wanted: whole slices of `unit` rows per chunk, and the chunks that leaves
  auto split = [&](long long ch, int unit) {
    *rows = ((M + ch - 1) / ch + unit - 1) / unit * unit;
    *chunks = (M + *rows - 1) / *rows;
  };
  if (!g_wgrad_widen && wgrad_fc_cin(d, dtype)) {
    // one round of workgroups (two per CU; one for Cin 64), every one with at least four slices (wgrad_fc_cin)
    split(wgrad_fc_cin(d, dtype) == 64 ? 256 : 512, kFcRows);
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
    split(ch, kW3Rows);
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
    split(ch, kWhRows);
    return;
  }
  const long long tiles = (long long)((K + 63) / 64) * ((d->Cout + 63) / 64);
  long long ch = (256 * 4 + tiles - 1) / tiles;            // ~4 workgroups per CU, at least 8 slices each
  const long long mx = (M + 8 * kWgRows - 1) / (8 * kWgRows);
  if (ch > mx) ch = mx;
  if (ch < 1) ch = 1;
  if (ch > 65535) ch = 65535;
  split(ch, kWgRows);
}

static int wgrad_impl(const yv4_conv_desc* d, int dtype, const void* x, const void* dy, float* dw, void* stream,
                      float* ws = nullptr, size_t ws_bytes = 0) {
  YV4_REQUIRE(d && x && dy && dw, "wgrad: null argument");
  YV4_REQUIRE(dtype == YV4_F32 || dtype == YV4_F16 || dtype == YV4_BF16, "wgrad: dtype must be f32, f16 or bf16");
  const int es = dtype == YV4_F32 ? 4 : 2;
  ConvDescRules rules{dtype == YV4_F32 ? 4 : 8};
  rules.align_cout = rules.align_y = true; rules.acts = 0;      // (dY, the descriptor's y view, is an operand: aligned like x)
  if (int rc = check_conv_desc(d, "wgrad", rules)) return rc;
  const long long M = (long long)d->N * d->Ho * d->Wo;
  const long long xb = (long long)d->N * d->H * d->W * d->x_cstride * es, db = M * d->y_cstride * es;
  YV4_REQUIRE(desc_addressable(xb) && desc_addressable(db), "wgrad: tensors of 4 GiB or more are not supported");
  WgradArgs a = wgrad_args(d, x, dy, dw);
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
