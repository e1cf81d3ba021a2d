// Host-side routing helpers shared by the fp32 and the 16-bit convolution dispatchers (conv_mfma_f32.hip,
// conv_mfma_h16.hip): what a tile id means, the rule by which a wide kernel takes a layer, the split-K arithmetic.
#pragma once
#include "yv4.h"

namespace yv4 {

// YV4_TILE_* / YV4_HTILE_* name a kernel family; the *_SHAPE(i) forms of the wide families also pin the workgroup tile
// shape i.  {family, shape}, shape -1 when none is pinned (an id of no family comes back as it is).
struct TileId { int tile, shape; };
inline TileId decode_tile_f32(int tile) {
  for (int i = 0; i <= 4; ++i) {
    if (tile == YV4_TILE_W3x3_SHAPE(i)) return {YV4_TILE_W3x3, i};
    if (tile == YV4_TILE_WIDE_SHAPE(i)) return {YV4_TILE_WIDE, i};
  }
  return {tile, -1};
}
inline TileId decode_tile_h16(int tile) {
  for (int i = 0; i <= 6; ++i) {
    if (tile == YV4_HTILE_W3x3_SHAPE(i)) return {YV4_HTILE_W3x3, i};
    if (i <= 4 && tile == YV4_HTILE_WIDE_SHAPE(i)) return {YV4_HTILE_WIDE, i};
  }
  return {tile, -1};
}

// A wide kernel takes a layer with at least min_out_per_cu outputs per CU (256 CUs) when one of its tile shapes fills
// the rounds to within max_waste_pct percent: eff is the picked shape's cost relative to a perfectly divided layer
// (wide_pick, conv_wide_common.h).  kAnyFill as max_waste_pct: the output count alone decides.
constexpr int kAnyFill = 1 << 30;
inline bool fills_rounds(long long M, int Cout, int min_out_per_cu, int max_waste_pct, double eff) {
  return M * Cout >= 256LL * min_out_per_cu && eff * 100.0 <= 100.0 + max_waste_pct;
}

// Split-K of the 64 x 64 tiles (single-image plans): `bk` is the kernel's K slice (32 floats / 64 16-bit elements),
// `cround` the channel rounding of a workspace row (4 / 8).  Ways: double while tiles x ways stays under `target`
// workgroups (~2 per CU) and every split keeps at least min_slices K slices; at most 32; 1 = do not split.
inline int splitk_ways(long long tiles, int nk, long long target, int min_slices) {
  int ks = 1;
  while (tiles * ks < target && nk / (ks * 2) >= min_slices && ks < 32) ks *= 2;
  return ks;
}
inline size_t splitk_workspace_bytes(const yv4_conv_desc* d, int ks, int cround) {
  if (ks <= 1) return 0;
  return (size_t)ks * (size_t)((long long)d->N * d->Ho * d->Wo) * (size_t)((d->Cout + cround - 1) / cround * cround) * sizeof(float);
}
// slices per split, the number of non-empty splits (72 slices 16 ways = 15 splits of 5, the last of 2), the slabs
template <class Args>
inline void splitk_set(Args& a, int ks, int bk, int cround, float* workspace) {
  const int nk = a.K / bk;
  a.ks_slices = (nk + ks - 1) / ks;
  a.ksplit = (nk + a.ks_slices - 1) / a.ks_slices;
  a.ws_cs = (a.Cout + cround - 1) / cround * cround;
  a.ws = workspace;
}
// the finish kernel: one thread per `cround` channels of a pixel, grid-stride from at most 2048 workgroups of 256
template <class Args>
inline unsigned splitk_finish_grid(const Args& a, int cround) {
  const long long g = ((long long)a.M * (a.ws_cs / cround) + 255) / 256;
  return (unsigned)(g > 2048 ? 2048 : g);
}

}  // namespace yv4
