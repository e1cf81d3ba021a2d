// Shared by the weight-gradient translation units (conv_wgrad.hip: the generic kernels and the dispatcher;
// conv_wgrad3x3_h16.hip and conv_wgrad_fc_h16.hip: the two special 3x3 families): the MFMA fragment types, the
// kernels' argument block, the (tile, chunk) mapping and the families' host functions.  (LDS-DMA helpers: lds_dma.h)
#pragma once
#include "yv4_common.h"
#include "lds_dma.h"

namespace yv4 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_w __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_w __attribute__((ext_vector_type(8)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));

struct WgradArgs {
  const void* x;
  const void* dy;
  float* dw;
  int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
  int x_cs, x_co, dy_cs, dy_co;
  int M, K;
  int tiles_k, rows_per_chunk;
  int tiles = 0, chunks = 0, xcd_map = 0;   // see wgrad_tile_chunk
  int ablate = 0;                           // measurement build only (YV4_WFC_ABLATE)
  FastDiv fd_hw, fd_wo;     // m / (Ho*Wo), r / Wo: the per-slice row decode sits inside the pipelined loop
  // deterministic form: chunk c of the M reduction stores its partial dW to slab c of ws ([chunks][Cout][K], plain
  // stores); wgrad_reduce_kernel then adds the slabs to dw in chunk order.  ws == nullptr: float atomics into dw.
  float* ws = nullptr;
  long long ws_stride = 0;
};

// The argument block of a descriptor (its y view is dY) and its tensors, as conv_args (conv_f32_common.h).  The dispatcher
// sets the chunking and the deterministic slabs, a launch function its family's fields.
static inline WgradArgs wgrad_args(const yv4_conv_desc* d, const void* x, const void* dy, float* dw) {
  WgradArgs a{};
  a.x = x; a.dy = dy; a.dw = dw;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
  a.x_cs = d->x_cstride; a.x_co = d->x_coff; a.dy_cs = d->y_cstride; a.dy_co = d->y_coff;
  a.M = (int)((long long)d->N * d->Ho * d->Wo); a.K = d->KH * d->KW * d->Cin;
  a.fd_hw = make_fastdiv((unsigned)(d->Ho * d->Wo)); a.fd_wo = make_fastdiv((unsigned)d->Wo);
  return a;
}

constexpr int kWgRows = 32;   // reduction rows per slice: the generic fp32 / widening kernel
constexpr int kW3Rows = 64;   // the 3x3 kernels (conv_wgrad3x3_h16.hip)
constexpr int kFcRows = 64;   // the few-channel kernels (conv_wgrad_fc_h16.hip)

// Which (dW tile, reduction chunk) a workgroup serves.  All tiles of ONE chunk read the same rows of dY and of the
// activation (each its own columns, but whole 128-byte lines), and a layer whose dW has several tiles re-reads its
// operands once per tile column / row -- from HBM, when the tiles of a chunk sit on different XCDs: workgroups go to
// the 8 XCDs round-robin by linear id and every XCD has its own L2.  With xcd_map the grid is one-dimensional and
// workgroup L serves chunk 8 g + (L mod 8), tile j of it, with L / 8 = g * tiles + j: a chunk's tiles are neighbours in
// the launch order of ONE XCD, so the re-reads hit that XCD's L2, while the eight XCDs still sweep the reduction range
// side by side.  (Dealing each XCD one contiguous eighth of the (chunk, tile) pairs instead was measured too: the same
// gain on the 1x1 layers, but 20-30 % SLOWER on the HBM-bound few-channel layers at 304 / 608 pixels, whose XCDs then
// stream from eight distant regions.)  Batch 64, same box: 64->128 s2 @304 623 -> 461 us, 128->256 s2 @152 487 -> 379,
// 256->256 1x1 @38 41 -> 32; network 449 -> 478 TFLOP/s.  The chunk count is rounded to a multiple of 8 for it
// (wgrad_chunks).  Slabs and their summation order are indexed by the chunk, not by the workgroup: the result does
// not depend on the mapping.
__device__ __forceinline__ bool wgrad_tile_chunk(const int tiles, const int chunks, const int xcd_map, int& tile, int& chunk) {
  if (!xcd_map) {
    tile = (int)blockIdx.x;
    chunk = (int)blockIdx.y;
    return true;
  }
  const unsigned L = blockIdx.x;
  const unsigned j = L >> 3;
  const unsigned g = j / (unsigned)tiles;
  tile = (int)(j - g * (unsigned)tiles);
  chunk = (int)(g * 8u + (L & 7u));
  return chunk < chunks;
}
static inline dim3 wgrad_grid(long long tiles, long long chunks, int xcd_map) {
  if (!xcd_map) return dim3((unsigned)tiles, (unsigned)chunks);
  return dim3((unsigned)((chunks + 7) / 8 * 8 * tiles), 1u);
}

// ---- the two special families, as the dispatcher (wgrad_chunks, wgrad_impl in conv_wgrad.hip) sees them: the domain
// test and one launch function each.  A launch function sets the ensure_dyn_lds attributes, fills the family's fields
// of the argument block, launches on `stream` and returns a status; the deterministic slab reduce stays with the caller.
// (hidden: these cross translation units, not the library's boundary)
#pragma GCC visibility push(hidden)
int wgrad_fc_cin(const yv4_conv_desc* d, int dtype);
int wgrad_fc_launch(WgradArgs& a, int dtype, int fc, long long xb, long long db, long long ch, void* stream, bool use_v2);
bool wgrad3x3_applies(const yv4_conv_desc* d, int dtype);
bool w3_xcd_map(long long tiles, long long chunks);
int wgrad3x3_launch(WgradArgs& a, int dtype, long long xb, long long db, long long ch, void* stream, bool w3_v2_ok);
#pragma GCC visibility pop

}  // namespace yv4
