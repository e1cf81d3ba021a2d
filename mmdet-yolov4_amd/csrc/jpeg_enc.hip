// The baseline JPEG encoder on the device (include/yv4.h, "baseline JPEG encoding"): the kernels around the shared core
// of jpeg_enc_core.h.  Two seams, two entry points:
//   yv4_jpeg_encode_coefficients   pixels -> quantised coefficients, one lane per 8x8 block (colour conversion, box
//                                  downsampling, islow FDCT, quantisation, dummy blocks), 128 bytes out per lane as eight
//                                  16-byte stores.  The pixel reads are bytes: an interleaved B G R row of 8 pixels is 24
//                                  bytes at any alignment, and a chroma sample gathers from two rows.
//   yv4_jpeg_encode_scan           coefficients -> the stuffed scan bytes: bits per block; their running sum in scan
//                                  order (per workgroup in LDS, across workgroups in a launch of its own); the pack, every
//                                  word ORed atomically into a zero-filled stream; the 0xFF count per word, its running
//                                  sum the same way, and the stuffed write, every byte by exactly one lane.
// No workgroup waits on another inside a launch, and nothing depends on the order lanes arrive in: two runs give the
// same bytes.  Every launch is a flat grid of YV4_JPEG_ENC_WG_BLOCKS lanes a workgroup; a workgroup finds its image by
// bisection over the table's dense workgroup bases, which the host validated.
#include <hip/hip_runtime.h>

#include "yv4_common.h"
#include "jpeg_enc_core.h"

namespace yv4 {

using namespace jpegenc;

constexpr int kWg = YV4_JPEG_ENC_WG_BLOCKS;

// the image workgroup g belongs to: the last one whose base is <= g.  stuff: the stuffing grid's bases.
__device__ __forceinline__ int image_of(const yv4_jpeg_enc_image* __restrict__ t, int N, int64_t g, bool stuff) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((stuff ? t[mid].swg_base : t[mid].wg_base) <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// exclusive running sum over the workgroup's kWg lanes; *total: their sum.  All lanes call it.
template <class T>
__device__ __forceinline__ T wg_exclusive(T v, T* lds, T* total) {
  const int t = (int)threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < kWg; d <<= 1) {
    const T a = t >= d ? lds[t - d] : (T)0;
    __syncthreads();
    lds[t] += a;
    __syncthreads();
  }
  *total = lds[kWg - 1];
  const T ex = lds[t] - v;
  __syncthreads();
  return ex;
}

struct AtomicOr {
  uint32_t* words;
  __host__ __device__ void operator()(int64_t k, uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(words + k, v);
#else
    words[k] |= v;
#endif
  }
};

__device__ __forceinline__ void load_tables(Tables* tabs) {
  if (threadIdx.x < 4) build_table(tabs, (int)threadIdx.x);
  __syncthreads();
}

// stage 1: one lane per block of the coefficient layout
__global__ __launch_bounds__(kWg) void jpeg_enc_coef_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                           const uint8_t* __restrict__ pixels, int rgb,
                                                           int16_t* __restrict__ coef) {
  const int n = image_of(table, N, blockIdx.x, false);
  const yv4_jpeg_enc_image& im = table[n];
  const int64_t i = ((int64_t)blockIdx.x - im.wg_base) * kWg + (int)threadIdx.x;
  if (i >= im.nblocks) return;
  alignas(16) int16_t o[64];
  block_coef(im, pixels, i, rgb, o);
  int4* dst = reinterpret_cast<int4*>(coef + im.coef_off + i * 64);      // coef 16-byte aligned, coef_off % 64 == 0
  const int4* src = reinterpret_cast<const int4*>(o);
#pragma unroll
  for (int k = 0; k < 8; ++k) dst[k] = src[k];
}

// stage 2a: bits of every block in scan order, and each workgroup's sum
__global__ __launch_bounds__(kWg) void jpeg_enc_count_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                            const int16_t* __restrict__ coef, uint8_t* __restrict__ work) {
  __shared__ Tables tabs;
  __shared__ uint32_t lds[kWg];
  load_tables(&tabs);
  const int n = image_of(table, N, blockIdx.x, false);
  const yv4_jpeg_enc_image& im = table[n];
  const Work w = work_of(work, im);
  const int64_t g = (int64_t)blockIdx.x - im.wg_base, j = g * kWg + (int)threadIdx.x;
  uint32_t bits = 0;
  if (j < im.nblocks) {
    bits = block_bits(im, coef, j, tabs);
    w.bits[j] = bits;
  }
  uint32_t total;
  wg_exclusive(bits, lds, &total);
  if (threadIdx.x == 0) w.wgsum[g] = total;
}

// stages 2b and 3b: the workgroup sums of one image -> their exclusive running sums, in place, one workgroup per image.
// stuff == 0: the block scan's sums; leaves the scan's bit count, padded to a byte, in totals[0].  stuff != 0: the 0xFF
// counts; leaves their sum in totals[1] and the image's stuffed byte count in sizes.
__global__ __launch_bounds__(kWg) void jpeg_enc_wgscan_kernel(const yv4_jpeg_enc_image* __restrict__ table,
                                                             uint8_t* __restrict__ work, int stuff,
                                                             int64_t* __restrict__ sizes) {
  __shared__ uint64_t lds[kWg];
  const yv4_jpeg_enc_image& im = table[blockIdx.x];
  const Work w = work_of(work, im);
  uint64_t* a = stuff ? w.sff : w.wgsum;
  const int64_t count = stuff ? enc_swgs(im.nblocks) : enc_wgs(im.nblocks);
  uint64_t carry = 0;
  for (int64_t base = 0; base < count; base += kWg) {
    const int64_t k = base + (int)threadIdx.x;
    const uint64_t v = k < count ? a[k] : 0;
    uint64_t total;
    const uint64_t ex = wg_exclusive(v, lds, &total);
    if (k < count) a[k] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (stuff) {
      w.totals[1] = carry;
      sizes[blockIdx.x] = (int64_t)((w.totals[0] >> 3) + carry);
    } else {
      w.totals[0] = (carry + 7) & ~(uint64_t)7;
    }
  }
}

// the words the packed stream will touch, zeroed (stuffing grid: one lane per word)
__global__ __launch_bounds__(kWg) void jpeg_enc_zero_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                           uint8_t* __restrict__ work) {
  const int n = image_of(table, N, blockIdx.x, true);
  const yv4_jpeg_enc_image& im = table[n];
  const Work w = work_of(work, im);
  const int64_t k = ((int64_t)blockIdx.x - im.swg_base) * kWg + (int)threadIdx.x;
  if (k < enc_words(im.nblocks) && k <= (int64_t)(w.totals[0] >> 5)) w.words[k] = 0;
}

// stage 2c: the pack
__global__ __launch_bounds__(kWg) void jpeg_enc_pack_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                           const int16_t* __restrict__ coef, uint8_t* __restrict__ work) {
  __shared__ Tables tabs;
  __shared__ uint32_t lds[kWg];
  load_tables(&tabs);
  const int n = image_of(table, N, blockIdx.x, false);
  const yv4_jpeg_enc_image& im = table[n];
  const Work w = work_of(work, im);
  const int64_t g = (int64_t)blockIdx.x - im.wg_base, j = g * kWg + (int)threadIdx.x;
  const uint32_t bits = j < im.nblocks ? w.bits[j] : 0;
  uint32_t total;
  const uint32_t ex = wg_exclusive(bits, lds, &total);
  if (j < im.nblocks) block_pack(im, coef, j, w.wgsum[g] + ex, bits, tabs, AtomicOr{w.words});
}

// stage 3a: 0xFF bytes per word of the stream, and each workgroup's sum
__global__ __launch_bounds__(kWg) void jpeg_enc_ffcount_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                              uint8_t* __restrict__ work) {
  __shared__ uint32_t lds[kWg];
  const int n = image_of(table, N, blockIdx.x, true);
  const yv4_jpeg_enc_image& im = table[n];
  const Work w = work_of(work, im);
  const int64_t g = (int64_t)blockIdx.x - im.swg_base, k = g * kWg + (int)threadIdx.x;
  const int64_t nbytes = (int64_t)(w.totals[0] >> 3);
  if (g * kWg * 4 >= nbytes) {      // past the stream (the grid covers the bound): the whole workgroup leaves
    if (threadIdx.x == 0) w.sff[g] = 0;
    return;
  }
  uint32_t total;
  wg_exclusive(word_ffs(w.words, k, nbytes), lds, &total);
  if (threadIdx.x == 0) w.sff[g] = total;
}

// stage 3c: the stuffed bytes
__global__ __launch_bounds__(kWg) void jpeg_enc_stuff_kernel(const yv4_jpeg_enc_image* __restrict__ table, int N,
                                                            uint8_t* __restrict__ work, uint8_t* __restrict__ out) {
  __shared__ uint32_t lds[kWg];
  const int n = image_of(table, N, blockIdx.x, true);
  const yv4_jpeg_enc_image& im = table[n];
  const Work w = work_of(work, im);
  const int64_t g = (int64_t)blockIdx.x - im.swg_base, k = g * kWg + (int)threadIdx.x;
  const int64_t nbytes = (int64_t)(w.totals[0] >> 3);
  if (g * kWg * 4 >= nbytes) return;
  uint32_t total;
  const uint32_t ex = wg_exclusive(word_ffs(w.words, k, nbytes), lds, &total);
  word_stuff(w.words, k, nbytes, w.sff[g] + ex, out + im.out_off);
}

}  // namespace yv4

using namespace yv4;

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static const int64_t kAny = (int64_t)1 << 62;      // a buffer the entry point does not touch

extern "C" int yv4_jpeg_encode_coefficients(const yv4_jpeg_enc_image* table, const yv4_jpeg_enc_image* table_dev, int N,
                                            const uint8_t* pixels, int64_t pixel_bytes, int rgb, int16_t* coef,
                                            int64_t coef_elems, void* stream) {
  YV4_REQUIRE(table && table_dev && pixels && coef, "jpeg_encode_coefficients: null pointer");
  YV4_REQUIRE(aligned(table_dev, 8) && aligned(coef, 16), "jpeg_encode_coefficients: table_dev must be 8-byte, coef 16-byte aligned");
  const int st = jpeg_enc_validate(table, N, pixel_bytes, coef_elems, kAny, kAny, "jpeg_encode_coefficients");
  if (st != YV4_OK) return st;
  const int64_t nwg = table[N - 1].wg_base + enc_wgs(table[N - 1].nblocks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3((unsigned)nwg), dim3(kWg), 0, s, table_dev, N, pixels, rgb != 0, coef);
  YV4_CHECK_LAUNCH("jpeg_enc_coef");
  return YV4_OK;
}

extern "C" int yv4_jpeg_encode_scan(const yv4_jpeg_enc_image* table, const yv4_jpeg_enc_image* table_dev, int N,
                                    const int16_t* coef, int64_t coef_elems, uint8_t* work, int64_t work_bytes, uint8_t* out,
                                    int64_t out_bytes, int64_t* sizes, void* stream) {
  YV4_REQUIRE(table && table_dev && coef && work && out && sizes, "jpeg_encode_scan: null pointer");
  YV4_REQUIRE(aligned(table_dev, 8) && aligned(coef, 2) && aligned(work, 8) && aligned(sizes, 8),
              "jpeg_encode_scan: table_dev, work and sizes must be 8-byte, coef 2-byte aligned");
  const int st = jpeg_enc_validate(table, N, kAny, coef_elems, work_bytes, out_bytes, "jpeg_encode_scan");
  if (st != YV4_OK) return st;
  const unsigned nwg = (unsigned)(table[N - 1].wg_base + enc_wgs(table[N - 1].nblocks));
  const unsigned nswg = (unsigned)(table[N - 1].swg_base + enc_swgs(table[N - 1].nblocks));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(nwg), dim3(kWg), 0, s, table_dev, N, coef, work);
  YV4_CHECK_LAUNCH("jpeg_enc_count");
  hipLaunchKernelGGL(jpeg_enc_wgscan_kernel, dim3((unsigned)N), dim3(kWg), 0, s, table_dev, work, 0, sizes);
  YV4_CHECK_LAUNCH("jpeg_enc_wgscan");
  hipLaunchKernelGGL(jpeg_enc_zero_kernel, dim3(nswg), dim3(kWg), 0, s, table_dev, N, work);
  YV4_CHECK_LAUNCH("jpeg_enc_zero");
  hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3(nwg), dim3(kWg), 0, s, table_dev, N, coef, work);
  YV4_CHECK_LAUNCH("jpeg_enc_pack");
  hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3(nswg), dim3(kWg), 0, s, table_dev, N, work);
  YV4_CHECK_LAUNCH("jpeg_enc_ffcount");
  hipLaunchKernelGGL(jpeg_enc_wgscan_kernel, dim3((unsigned)N), dim3(kWg), 0, s, table_dev, work, 1, sizes);
  YV4_CHECK_LAUNCH("jpeg_enc_wgscan");
  hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(nswg), dim3(kWg), 0, s, table_dev, N, work, out);
  YV4_CHECK_LAUNCH("jpeg_enc_stuff");
  return YV4_OK;
}
