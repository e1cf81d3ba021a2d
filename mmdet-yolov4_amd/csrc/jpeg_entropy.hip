// The Huffman scan of the baseline JPEG decoder on the device (include/yv4.h, "the Huffman scan on the device"): file
// bytes -> the int16 coefficients yv4_jpeg_reconstruct reads, for a batch of images in one launch.
//
// jpeg_entropy_kernel: one lane per SEGMENT (a run of whole MCUs that starts on a byte boundary with the DC predictors
// zero: one per restart interval, or the whole scan), one wave of 64 lanes per workgroup over up to 64 consecutive
// segments of one image.  The workgroup copies its image's packed Huffman tables (at most six, 1344 bytes each) into LDS
// once, then every lane runs jpeg::decode_segment (jpeg_entropy_core.h, the code the host entry runs too).  Segments
// are independent by construction: no speculation, no communication between lanes, no waiting; every loop is bounded
// by a count the host validated.  The lanes of a wave diverge freely -- a wave costs what its slowest segment costs,
// and a batch what its slowest image costs, the images being spread over the CUs.
// A lane that meets an error raises its image's status word to the error's code (atomicMax: the same outcome on every
// run) and stops.  Reads stay inside the segment's bytes and stores on the image's block grid whatever the bytes hold.
#include "yv4_common.h"
#include "jpeg_entropy_core.h"

namespace yv4 {

int jpeg_entropy_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs, int N,
                          int64_t nseg, int64_t nwg, int64_t bytes_len, int64_t nhuff, int64_t coef_elems,
                          int64_t* coef_lo, int64_t* coef_hi);

constexpr int kHuffWords = (int)(sizeof(yv4_jpeg_huff) / 4);
static_assert(sizeof(yv4_jpeg_huff) == 1344 && sizeof(yv4_jpeg_huff) % 4 == 0, "yv4_jpeg_huff is copied as 32-bit words");
static_assert(sizeof(yv4_jpeg_scan) == 96 && sizeof(yv4_jpeg_segment) == 40 && sizeof(yv4_jpeg_wg) == 16,
              "the table structures of include/yv4.h");

__global__ __launch_bounds__(YV4_JPEG_WG_SEGMENTS) void jpeg_entropy_kernel(
    const yv4_jpeg_scan* __restrict__ scans, const yv4_jpeg_segment* __restrict__ segs,
    const yv4_jpeg_wg* __restrict__ wgs, const uint8_t* __restrict__ bytes, const yv4_jpeg_huff* __restrict__ huff,
    int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ yv4_jpeg_huff tabs[YV4_JPEG_MAX_HUFF];
  __shared__ uint8_t zigzag[64];
  const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;
  zigzag[threadIdx.x] = kZigzag[threadIdx.x];
  const yv4_jpeg_wg wg = wgs[blockIdx.x];
  const yv4_jpeg_scan sc = scans[wg.image];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + sc.huff_base);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
  for (int i = threadIdx.x; i < sc.nhuff * kHuffWords; i += YV4_JPEG_WG_SEGMENTS) dst[i] = src[i];
  __syncthreads();
  if ((int)threadIdx.x >= wg.count) return;
  const yv4_jpeg_segment sg = segs[sc.seg_base + wg.first_seg + (int)threadIdx.x];
  const int e = jpeg::decode_segment(sc, sg, bytes + sc.data_off, tabs, zigzag, coef + sc.coef_off);
  if (e) atomicMax(status + wg.image, e);
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_jpeg_entropy_decode_device(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                              const yv4_jpeg_wg* wgs, const yv4_jpeg_scan* scans_dev,
                                              const yv4_jpeg_segment* segs_dev, const yv4_jpeg_wg* wgs_dev, int N,
                                              int64_t nseg, int64_t nwg, const uint8_t* bytes, int64_t bytes_len,
                                              const yv4_jpeg_huff* huff, int64_t nhuff, int16_t* coef,
                                              int64_t coef_elems, int32_t* status, void* stream) {
  YV4_REQUIRE(scans && segs && wgs && scans_dev && segs_dev && wgs_dev && bytes && huff && coef && status,
              "jpeg_entropy_decode_device: null pointer");
  YV4_REQUIRE((reinterpret_cast<uintptr_t>(scans_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(segs_dev) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(wgs_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(huff) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(coef) & 1) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
              "jpeg_entropy_decode_device: scans_dev / segs_dev must be 8-byte, wgs_dev / huff / status 4-byte aligned");
  int64_t lo, hi;
  const int st = jpeg_entropy_validate(scans, segs, wgs, N, nseg, nwg, bytes_len, nhuff, coef_elems, &lo, &hi);
  if (st != YV4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(coef + lo, 0, (size_t)(hi - lo) * sizeof(int16_t), s) != hipSuccess ||
      hipMemsetAsync(status, 0, (size_t)N * sizeof(int32_t), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("jpeg_entropy_decode_device: the zero-fill of the coefficients failed");
    return YV4_E_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)nwg), dim3(YV4_JPEG_WG_SEGMENTS), 0, s, scans_dev, segs_dev,
                     wgs_dev, bytes, huff, coef, status);
  YV4_CHECK_LAUNCH("jpeg_entropy");
  return YV4_OK;
}
