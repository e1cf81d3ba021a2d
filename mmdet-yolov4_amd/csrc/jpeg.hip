// Device half of the baseline JPEG decoder (include/yv4.h, "baseline JPEG decoding"): quantised coefficients ->
// interleaved 8-bit pixels for a batch of images of different sizes and samplings, two launches per batch.
//
// The arithmetic is libjpeg's default decode, restated (tests/_jpeg_ref.py holds the same rules in numpy and is held
// byte for byte against libjpeg-turbo's output):
//   * jidctint "islow": 13-bit constants FIX(x) = int(x * 8192 + 0.5); the column pass on dequantised values descales by
//     (v + 1024) >> 11, the row pass by (v + (1 << 17)) >> 18, then the range-limit table indexed by v & 1023 --
//     including its wrap-around (no encoder's output reaches it; a hand-made file does: DESIGN 19).  All in 32-bit integers
//     (this file is compiled with -fwrapv: a hostile coefficient wraps, it does not invoke undefined behaviour).
//   * fancy upsampling over ceil(width / 2) (x ceil(height / 2)) real chroma samples, edges replicated, never the MCU
//     padding.  h2v2: s = 3 * near + far vertically, then (3 * s + s_left + 8) >> 4 / (3 * s + s_right + 7) >> 4.
//     h2v1: (3 * c + c_left + 1) >> 2 / (3 * c + c_right + 2) >> 2.
//   * YCbCr -> RGB with 16-bit fixed-point constants FX(x) = int(x * 65536 + 0.5), arithmetic shifts, clamp to 0..255.
//
// idct_kernel: one 8x8 block per 8 lanes, 32 blocks per 256-thread workgroup.  Lane j loads row j of the block (one
// 16-byte load) times the quantisation row, the block is transposed through LDS (row stride 9 words: conflict-free for
// the row writes and the column reads of the 4 blocks of a 32-lane group), lane j runs column j of pass 1, the
// workspace goes back through LDS, lane j runs row j of pass 2 and stores its 8 samples as one 8-byte store into the
// component's plane on the MCU-padded grid.
// pixel_kernel: four pixels of a row per thread, 256 x 4 pixel tiles; reads the luma word and the chroma samples its
// filters need (4 of each component in 4:2:2, 8 in 4:2:0) and writes 12 bytes as three words where the address allows,
// byte by byte otherwise (a row's tail, a pitch that breaks the alignment).
// A workgroup finds its image by binary search over the table's unit_base / tile_base prefix sums.
// orient_kernel: an image whose EXIF orientation (2 .. 8) is applied has no tile in pixel_kernel and a launch of its
// own: a 32 x 32 pixel tile of the decoded picture is computed as above (a quad per thread, contiguous reads of the
// planes) into LDS, one word a pixel, and read back so that consecutive lanes write consecutive pixels of an OUTPUT row
// -- for 5 .. 8 that is a column of the tile; at a row pitch of 33 words the 32 lanes of a half-wave read 32 distinct
// banks (ds_read_b32: bank = word % 32 within a half-wave), and so do the quad writes.  A batch without such an image
// launches the two kernels above and nothing else.
#include "yv4_common.h"

namespace yv4 {

constexpr int kFix_0_298631336 = 2446, kFix_0_390180644 = 3196, kFix_0_541196100 = 4433, kFix_0_765366865 = 6270,
              kFix_0_899976223 = 7373, kFix_1_175875602 = 9633, kFix_1_501321110 = 12299, kFix_1_847759065 = 15137,
              kFix_1_961570560 = 16069, kFix_2_053119869 = 16819, kFix_2_562915447 = 20995, kFix_3_072711026 = 25172;

// one 8-point pass of the islow IDCT: v[0..7] in, out[0..7] = the eight sums BEFORE the descale
__device__ __forceinline__ void idct8(const int (&v)[8], int (&o)[8]) {
  int z2 = v[2], z3 = v[6];
  int z1 = (z2 + z3) * kFix_0_541196100;
  int tmp2 = z1 + z3 * (-kFix_1_847759065);
  int tmp3 = z1 + z2 * kFix_0_765366865;
  int tmp0 = (v[0] + v[4]) << 13;
  int tmp1 = (v[0] - v[4]) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * kFix_1_175875602;
  tmp0 *= kFix_0_298631336; tmp1 *= kFix_2_053119869; tmp2 *= kFix_3_072711026; tmp3 *= kFix_1_501321110;
  z1 *= -kFix_0_899976223; z2 *= -kFix_2_562915447; z3 *= -kFix_1_961570560; z4 *= -kFix_0_390180644;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// libjpeg's IDCT range-limit table, as arithmetic: index i = v & 1023 of [128..255 | 255 x 384 | 0 x 384 | 0..127]
__device__ __forceinline__ unsigned range_limit(int v) {
  const int i = v & 1023;
  return (unsigned)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

// the image whose [base, next base) holds work unit u; BASE: &yv4_jpeg_image::unit_base / ::tile_base
template <int64_t yv4_jpeg_image::*BASE>
__device__ __forceinline__ int find_image(const yv4_jpeg_image* t, int N, int64_t u) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t[mid].*BASE <= u) lo = mid; else hi = mid;
  }
  return lo;
}

typedef short short8_t __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8_t __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const yv4_jpeg_image* __restrict__ table, int N,
                                                        const int16_t* __restrict__ coef,
                                                        const uint16_t* __restrict__ quant, uint8_t* __restrict__ work) {
  __shared__ int lds[32 * 72];
  const int n = find_image<&yv4_jpeg_image::unit_base>(table, N, (int64_t)blockIdx.x);
  const yv4_jpeg_image g = table[n];
  const int64_t nb0 = (int64_t)g.blocks_w[0] * g.blocks_h[0];
  const int64_t nb1 = g.ncomp == 3 ? (int64_t)g.blocks_w[1] * g.blocks_h[1] : 0;       // chroma planes are equal in size
  const int64_t blocks = nb0 + 2 * nb1;
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int64_t lb = ((int64_t)blockIdx.x - g.unit_base) * 32 + slot;      // block of the image, planes back to back
  const bool live = lb < blocks;
  // the block's component, by selects (indexing the table entry with a run-time component would put it in scratch)
  const int comp = lb < nb0 ? 0 : (lb < nb0 + nb1 ? 1 : 2);
  const int64_t pb = lb - (comp == 0 ? 0 : (comp == 1 ? nb0 : nb0 + nb1));  // block within its plane
  const int tq = comp == 0 ? g.tq[0] : (comp == 1 ? g.tq[1] : g.tq[2]);
  const int bw = comp == 0 ? g.blocks_w[0] : g.blocks_w[1];
  const int64_t plane = comp == 0 ? g.plane_off[0] : (comp == 1 ? g.plane_off[1] : g.plane_off[2]);
  int* tile = lds + slot * 72;
  int v[8], o[8];
  if (live) {
    const short8_t cr = *reinterpret_cast<const short8_t*>(coef + g.coef_off + lb * 64 + j * 8);
    const ushort8_t qr = *reinterpret_cast<const ushort8_t*>(quant + ((size_t)n * 4 + tq) * 64 + j * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[j * 9 + k] = (int)cr[k] * (int)qr[k];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[k * 9 + j];       // column j
    idct8(v, o);
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[k * 9 + j] = (o[k] + 1024) >> 11;
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[j * 9 + k];       // row j
    idct8(v, o);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= range_limit((o[k] + (1 << 17)) >> 18) << (8 * k);
      hi |= range_limit((o[k + 4] + (1 << 17)) >> 18) << (8 * k);
    }
    const int64_t by = pb / bw, bx = pb - by * bw;
    uint2 px;
    px.x = lo; px.y = hi;
    *reinterpret_cast<uint2*>(work + plane + (by * 8 + j) * ((int64_t)bw * 8) + bx * 8) = px;
  }
}

// Y, Cb, Cr (8-bit) -> the pixel's three output bytes, first byte lowest
__device__ __forceinline__ unsigned ycc_pixel(int Y, int cb8, int cr8, int rgb) {
  const int cb = cb8 - 128, cr = cr8 - 128;
  int R = Y + ((91881 * cr + 32768) >> 16);
  int B = Y + ((116130 * cb + 32768) >> 16);
  int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  R = min(max(R, 0), 255); G = min(max(G, 0), 255); B = min(max(B, 0), 255);
  return (unsigned)(rgb ? R : B) | ((unsigned)G << 8) | ((unsigned)(rgb ? B : R) << 16);
}

__global__ __launch_bounds__(256) void jpeg_pixel_kernel(const yv4_jpeg_image* __restrict__ table, int N,
                                                         const uint8_t* __restrict__ work, uint8_t* __restrict__ out,
                                                         int rgb) {
  const int n = find_image<&yv4_jpeg_image::tile_base>(table, N, (int64_t)blockIdx.x);
  const yv4_jpeg_image g = table[n];
  const int tiles_x = (g.width + 255) >> 8;
  const int t = (int)((int64_t)blockIdx.x - g.tile_base);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int x0 = (tx * 64 + (threadIdx.x & 63)) * 4;      // four pixels of one row per thread
  const int y = ty * 4 + (threadIdx.x >> 6);
  if (x0 >= g.width || y >= g.height) return;
  const int count = min(4, g.width - x0);
  // planes are 8-byte aligned with a pitch that is a multiple of 8, and x0 one of 4: the word may reach past the image's
  // width, never past the plane's row
  const unsigned yw = *reinterpret_cast<const unsigned*>(work + g.plane_off[0] + (int64_t)y * (g.blocks_w[0] * 8) + x0);
  unsigned px[4];
  if (g.ncomp == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ((yw >> (8 * k)) & 255u) * 0x010101u;
  } else {
    const int cw = (g.width + g.hs - 1) / g.hs, ch = (g.height + g.vs - 1) / g.vs;      // real chroma samples
    const int pitch = g.blocks_w[1] * 8;
    int c4[2][4];                                                                        // Cb, Cr of the four pixels
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint8_t* p = work + g.plane_off[1 + c];
      if (g.hs == 1) {
        const unsigned w4 = *reinterpret_cast<const unsigned*>(p + (int64_t)y * pitch + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) c4[c][k] = (int)((w4 >> (8 * k)) & 255u);
      } else {
        // the pixels x0 .. x0 + 3 lie over the samples cx0, cx0 + 1 and filter with cx0 - 1 .. cx0 + 2, edges replicated
        const int cx0 = x0 >> 1;
        int col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = min(max(cx0 - 1 + k, 0), cw - 1);
        if (g.vs == 1) {
          const uint8_t* r = p + (int64_t)y * pitch;
          const int s0 = r[col[0]], s1 = r[col[1]], s2 = r[col[2]], s3 = r[col[3]];
          c4[c][0] = (3 * s1 + s0 + 1) >> 2;
          c4[c][1] = (3 * s1 + s2 + 2) >> 2;
          c4[c][2] = (3 * s2 + s1 + 1) >> 2;
          c4[c][3] = (3 * s2 + s3 + 2) >> 2;
        } else {
          const int cy = y >> 1;
          const int cf = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);    // the far row, edge replicated
          const uint8_t* rn = p + (int64_t)cy * pitch;
          const uint8_t* rf = p + (int64_t)cf * pitch;
          int s[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] = 3 * rn[col[k]] + rf[col[k]];
          c4[c][0] = (3 * s[1] + s[0] + 8) >> 4;
          c4[c][1] = (3 * s[1] + s[2] + 7) >> 4;
          c4[c][2] = (3 * s[2] + s[1] + 8) >> 4;
          c4[c][3] = (3 * s[2] + s[3] + 7) >> 4;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ycc_pixel((int)((yw >> (8 * k)) & 255u), c4[0][k], c4[1][k], rgb);
  }
  uint8_t* o = out + g.out_off + (int64_t)y * g.out_pitch + 3 * x0;
  if (count == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {      // 12 bytes as three words
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
    o4[0] = px[0] | (px[1] << 24);
    o4[1] = (px[1] >> 8) | (px[2] << 16);
    o4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {                                                             // a row's tail, or a pitch that breaks alignment
    for (int k = 0; k < count; ++k) {
      o[3 * k] = (uint8_t)px[k];
      o[3 * k + 1] = (uint8_t)(px[k] >> 8);
      o[3 * k + 2] = (uint8_t)(px[k] >> 16);
    }
  }
}

// The four pixels x0 .. x0 + 3 (x0 % 4 == 0, x0 < width) of row y of image g -> px, three output bytes each: the arithmetic
// of jpeg_pixel_kernel, for jpeg_orient_kernel.  It is a second copy on purpose: as a function the compiler schedules it
// differently, and the kernel every untagged decode runs keeps the machine code it was measured with.
__device__ __forceinline__ void pixel_quad(const yv4_jpeg_image& g, const uint8_t* __restrict__ work, int x0, int y,
                                           int rgb, unsigned (&px)[4]) {
  // planes are 8-byte aligned with a pitch that is a multiple of 8, and x0 one of 4: the word may reach past the image's
  // width, never past the plane's row
  const unsigned yw = *reinterpret_cast<const unsigned*>(work + g.plane_off[0] + (int64_t)y * (g.blocks_w[0] * 8) + x0);
  if (g.ncomp == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ((yw >> (8 * k)) & 255u) * 0x010101u;
  } else {
    const int cw = (g.width + g.hs - 1) / g.hs, ch = (g.height + g.vs - 1) / g.vs;      // real chroma samples
    const int pitch = g.blocks_w[1] * 8;
    int c4[2][4];                                                                        // Cb, Cr of the four pixels
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint8_t* p = work + g.plane_off[1 + c];
      if (g.hs == 1) {
        const unsigned w4 = *reinterpret_cast<const unsigned*>(p + (int64_t)y * pitch + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) c4[c][k] = (int)((w4 >> (8 * k)) & 255u);
      } else {
        // the pixels x0 .. x0 + 3 lie over the samples cx0, cx0 + 1 and filter with cx0 - 1 .. cx0 + 2, edges replicated
        const int cx0 = x0 >> 1;
        int col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = min(max(cx0 - 1 + k, 0), cw - 1);
        if (g.vs == 1) {
          const uint8_t* r = p + (int64_t)y * pitch;
          const int s0 = r[col[0]], s1 = r[col[1]], s2 = r[col[2]], s3 = r[col[3]];
          c4[c][0] = (3 * s1 + s0 + 1) >> 2;
          c4[c][1] = (3 * s1 + s2 + 2) >> 2;
          c4[c][2] = (3 * s2 + s1 + 1) >> 2;
          c4[c][3] = (3 * s2 + s3 + 2) >> 2;
        } else {
          const int cy = y >> 1;
          const int cf = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);    // the far row, edge replicated
          const uint8_t* rn = p + (int64_t)cy * pitch;
          const uint8_t* rf = p + (int64_t)cf * pitch;
          int s[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] = 3 * rn[col[k]] + rf[col[k]];
          c4[c][0] = (3 * s[1] + s[0] + 8) >> 4;
          c4[c][1] = (3 * s[1] + s[2] + 7) >> 4;
          c4[c][2] = (3 * s[2] + s[1] + 8) >> 4;
          c4[c][3] = (3 * s[2] + s[3] + 7) >> 4;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ycc_pixel((int)((yw >> (8 * k)) & 255u), c4[0][k], c4[1][k], rgb);
  }
}

constexpr int kOrientTile = 32, kOrientPitch = kOrientTile + 1;

__global__ __launch_bounds__(256) void jpeg_orient_kernel(const yv4_jpeg_image* __restrict__ table, int n,
                                                          const uint8_t* __restrict__ work, uint8_t* __restrict__ out,
                                                          int rgb) {
  __shared__ unsigned lds[kOrientTile * kOrientPitch];
  const yv4_jpeg_image g = table[n];
  const int tiles_x = (g.width + kOrientTile - 1) / kOrientTile;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int x_base = tx * kOrientTile, y_base = ty * kOrientTile;      // the tile's corner in the decoded picture D
  {
    const int lx = (threadIdx.x & 7) * 4, ly = threadIdx.x >> 3;         // a quad of D per thread: 8 x 32 of them
    if (x_base + lx < g.width && y_base + ly < g.height) {
      unsigned px[4];
      pixel_quad(g, work, x_base + lx, y_base + ly, rgb, px);
#pragma unroll
      for (int k = 0; k < 4; ++k) lds[ly * kOrientPitch + lx + k] = px[k];      // columns past the width: never read back
    }
  }
  __syncthreads();
  const int o = g.orientation;
  const bool transpose = o >= 5;
  const bool flip_y = o == 3 || o == 4 || o == 6 || o == 7;      // D's row h-1-a instead of a
  const bool flip_x = o == 2 || o == 3 || o == 7 || o == 8;      // D's column w-1-b instead of b
#pragma unroll
  for (int it = 0; it < kOrientTile * kOrientTile / 256; ++it) {
    const int fast = threadIdx.x & 31, slow = (threadIdx.x >> 5) + 8 * it;
    // consecutive lanes walk an output row: D's rows for 5 .. 8 (a column of the tile), D's columns otherwise
    const int ly = transpose ? fast : slow, lx = transpose ? slow : fast;
    const int dy = y_base + ly, dx = x_base + lx;
    if (dy >= g.height || dx >= g.width) continue;
    const int a = flip_y ? g.height - 1 - dy : dy, b = flip_x ? g.width - 1 - dx : dx;
    const int oy = transpose ? b : a, ox = transpose ? a : b;
    const unsigned px = lds[ly * kOrientPitch + lx];
    uint8_t* q = out + g.out_off + (int64_t)oy * g.out_pitch + 3 * ox;
    q[0] = (uint8_t)px;
    q[1] = (uint8_t)(px >> 8);
    q[2] = (uint8_t)(px >> 16);
  }
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_jpeg_reconstruct(const yv4_jpeg_image* table, const yv4_jpeg_image* table_dev, int N,
                                    const int16_t* coef, int64_t coef_elems, const uint16_t* quant, uint8_t* work,
                                    int64_t work_bytes, uint8_t* out, int64_t out_bytes, int rgb, void* stream) {
  YV4_REQUIRE(table && table_dev && coef && quant && work && out, "jpeg_reconstruct: null pointer");
  YV4_REQUIRE(N > 0 && coef_elems > 0 && work_bytes > 0 && out_bytes > 0, "jpeg_reconstruct: empty batch or buffer");
  YV4_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 15) == 0 && (reinterpret_cast<uintptr_t>(quant) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(work) & 7) == 0 && (reinterpret_cast<uintptr_t>(table_dev) & 7) == 0,
              "jpeg_reconstruct: coef / quant must be 16-byte, work / table_dev 8-byte aligned");
  // the kernels trust the table: everything they index with is checked here, on the host copy
  int64_t units = 0, tiles = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_image& g = table[n];
    YV4_REQUIRE(g.width >= 1 && g.width <= 65535 && g.height >= 1 && g.height <= 65535 && (g.ncomp == 1 || g.ncomp == 3),
                "jpeg_reconstruct: image %d: bad size or component count", n);
    const bool samp_ok = g.ncomp == 1 ? (g.hs == 1 && g.vs == 1)
                                      : ((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2));
    YV4_REQUIRE(samp_ok, "jpeg_reconstruct: image %d: sampling %dx%d", n, g.hs, g.vs);
    const int mx = (g.width + 8 * g.hs - 1) / (8 * g.hs), my = (g.height + 8 * g.vs - 1) / (8 * g.vs);
    int64_t blocks = 0;
    for (int c = 0; c < g.ncomp; ++c) {
      YV4_REQUIRE(g.blocks_w[c] == mx * (c ? 1 : g.hs) && g.blocks_h[c] == my * (c ? 1 : g.vs),
                  "jpeg_reconstruct: image %d: the block grid of component %d does not follow from its size", n, c);
      YV4_REQUIRE(g.tq[c] >= 0 && g.tq[c] <= 3, "jpeg_reconstruct: image %d: quantisation table selector", n);
      const int64_t nb = (int64_t)g.blocks_w[c] * g.blocks_h[c];
      YV4_REQUIRE(g.plane_off[c] >= 0 && (g.plane_off[c] & 7) == 0 && g.plane_off[c] <= work_bytes - nb * 64,
                  "jpeg_reconstruct: image %d: plane %d leaves the workspace", n, c);
      blocks += nb;
    }
    YV4_REQUIRE(g.coef_off >= 0 && (g.coef_off & 63) == 0 && g.coef_off <= coef_elems - blocks * 64,
                "jpeg_reconstruct: image %d: its coefficients leave the buffer", n);
    YV4_REQUIRE(g.orientation >= 0 && g.orientation <= 8, "jpeg_reconstruct: image %d: orientation %d", n, g.orientation);
    const int ow = g.orientation >= 5 ? g.height : g.width, oh = g.orientation >= 5 ? g.width : g.height;      // the output's
    YV4_REQUIRE(g.out_pitch >= 3 * ow && g.out_off >= 0 &&
                    g.out_off <= out_bytes - ((int64_t)(oh - 1) * g.out_pitch + 3 * ow),
                "jpeg_reconstruct: image %d: its pixels leave the output buffer", n);
    YV4_REQUIRE(g.unit_base == units && g.tile_base == tiles, "jpeg_reconstruct: image %d: unit_base / tile_base", n);
    units += (blocks + 31) / 32;
    if (g.orientation < 2) tiles += (int64_t)((g.width + 255) / 256) * ((g.height + 3) / 4);
  }
  YV4_REQUIRE(units < (1ll << 31) && tiles < (1ll << 31), "jpeg_reconstruct: the batch is too large for one launch");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)units), dim3(256), 0, s, table_dev, N, coef, quant, work);
  YV4_CHECK_LAUNCH("jpeg_idct");
  if (tiles > 0) {      // every image of the batch may be an oriented one
    hipLaunchKernelGGL(jpeg_pixel_kernel, dim3((unsigned)tiles), dim3(256), 0, s, table_dev, N, work, out, rgb ? 1 : 0);
    YV4_CHECK_LAUNCH("jpeg_pixel");
  }
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_image& g = table[n];
    if (g.orientation < 2) continue;
    const unsigned grid = (unsigned)((g.width + kOrientTile - 1) / kOrientTile) * (unsigned)((g.height + kOrientTile - 1) / kOrientTile);
    hipLaunchKernelGGL(jpeg_orient_kernel, dim3(grid), dim3(256), 0, s, table_dev, n, work, out, rgb ? 1 : 0);
    YV4_CHECK_LAUNCH("jpeg_orient");
  }
  return YV4_OK;
}
