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
//
// jpeg_sync_kernel, jpeg_chunk_scan_kernel, jpeg_chunk_decode_kernel (further down): many lanes per segment, one per chunk
// of its bytes, entered through self-synchronised states (include/yv4.h, "self-synchronising chunks").
#include "yv4_common.h"
#include "jpeg_common.h"
#include "jpeg_entropy_core.h"

namespace yv4 {

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

// ---- self-synchronising chunks (include/yv4.h): many lanes per segment ------------------------------------------------
// The mapping of all three kernels' decode passes is the one above with chunks for segments: one wave per run of up to
// 64 consecutive chunks of one image (yv4_jpeg_wg), the image's tables and the zigzag order in LDS -- 8.1 KB a
// workgroup, so that LDS admits 19 workgroups on a CU and the waves of several share each SIMD.  No lane waits on
// another workgroup: a synchronisation round is a launch, and a round reads the exit words the round before wrote.
static_assert(sizeof(yv4_jpeg_chunk) == 16 && sizeof(yv4_jpeg_entry) == 48, "the chunk structures of include/yv4.h");

__device__ __forceinline__ void jpeg_load_tables(yv4_jpeg_huff* tabs, uint8_t* zigzag, const yv4_jpeg_huff* huff,
                                                 const yv4_jpeg_scan& sc) {
  const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;
  zigzag[threadIdx.x] = kZigzag[threadIdx.x];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + sc.huff_base);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
  for (int i = threadIdx.x; i < sc.nhuff * kHuffWords; i += YV4_JPEG_WG_CHUNKS) dst[i] = src[i];
  __syncthreads();
}

// One synchronisation round (jpeg::sync_chunk).  A workgroup none of whose chunks has to be decoded again carries its
// exit words over and leaves without loading the tables.
__global__ __launch_bounds__(YV4_JPEG_WG_CHUNKS) void jpeg_sync_kernel(
    const yv4_jpeg_scan* __restrict__ scans, const yv4_jpeg_segment* __restrict__ segs,
    const yv4_jpeg_chunk* __restrict__ chunks, const yv4_jpeg_wg* __restrict__ wgs, const uint8_t* __restrict__ bytes,
    const yv4_jpeg_huff* __restrict__ huff, yv4_jpeg_entry* entries, int chunk_bytes, int round) {
  __shared__ yv4_jpeg_huff tabs[YV4_JPEG_MAX_HUFF];
  __shared__ uint8_t zigzag[64];
  const yv4_jpeg_wg wg = wgs[blockIdx.x];
  const bool live = (int)threadIdx.x < wg.count;
  const int64_t g = (int64_t)wg.first_seg + (live ? (int)threadIdx.x : 0);
  const yv4_jpeg_chunk ck = chunks[g];
  uint64_t prev = jpeg::kChunkInvalid;
  if (round > 0 && ck.index > 0) prev = entries[g - 1].exit[(round + 1) & 1];
  const bool need = live && (round == 0 || (ck.index > 0 && prev != jpeg::kChunkInvalid && prev != entries[g].entry));
  if (!__syncthreads_or(need)) {
    if (live) entries[g].exit[round & 1] = entries[g].exit[(round + 1) & 1];
    return;
  }
  const yv4_jpeg_scan sc = scans[wg.image];
  jpeg_load_tables(tabs, zigzag, huff, sc);
  if (!live) return;
  const yv4_jpeg_segment sg = segs[ck.seg];
  jpeg::sync_chunk(sc, sg, bytes + sc.data_off, tabs, zigzag, ck, chunk_bytes, round, prev, entries + g);
}

// The exclusive sums over one segment's chunks (blocks completed, DC sums per component) and the checks
// (jpeg::check_chunk): one workgroup of 256 lanes per segment, 256 chunks a step, the sums of the steps before carried
// in registers.  A chunk that is not proven marks its image undecided.
constexpr int kScanLanes = 256;
__global__ __launch_bounds__(kScanLanes) void jpeg_chunk_scan_kernel(
    const yv4_jpeg_scan* __restrict__ scans, const yv4_jpeg_segment* __restrict__ segs,
    const yv4_jpeg_chunk* __restrict__ chunks, const int32_t* __restrict__ seg_first, yv4_jpeg_entry* entries,
    int32_t* undecided, int fin) {
  __shared__ long long nb[kScanLanes];
  __shared__ uint32_t d0[kScanLanes], d1[kScanLanes], d2[kScanLanes];
  const int t = threadIdx.x;
  const int64_t c0 = seg_first[blockIdx.x], c1 = seg_first[blockIdx.x + 1];
  const int image = chunks[c0].image;
  const yv4_jpeg_scan sc = scans[image];
  const yv4_jpeg_segment sg = segs[blockIdx.x];
  long long carry = 0;
  uint32_t cd0 = 0, cd1 = 0, cd2 = 0;
  bool bad = false;
  for (int64_t base = c0; base < c1; base += kScanLanes) {
    const int64_t g = base + t;
    const bool live = g < c1;
    const long long own = live ? entries[g].nblk : 0;
    const uint32_t o0 = live ? entries[g].dc[0] : 0, o1 = live ? entries[g].dc[1] : 0, o2 = live ? entries[g].dc[2] : 0;
    nb[t] = own; d0[t] = o0; d1[t] = o1; d2[t] = o2;
    __syncthreads();
    for (int off = 1; off < kScanLanes; off <<= 1) {
      const bool take = t >= off;
      const long long a = take ? nb[t - off] : 0;
      const uint32_t x0 = take ? d0[t - off] : 0, x1 = take ? d1[t - off] : 0, x2 = take ? d2[t - off] : 0;
      __syncthreads();
      nb[t] += a; d0[t] += x0; d1[t] += x1; d2[t] += x2;
      __syncthreads();
    }
    if (live) {
      const yv4_jpeg_chunk ck = chunks[g];
      const uint64_t prev = ck.index > 0 ? entries[g - 1].exit[fin] : jpeg::kChunkInvalid;
      const uint32_t dcs[3] = {cd0 + d0[t] - o0, cd1 + d1[t] - o1, cd2 + d2[t] - o2};
      if (!jpeg::check_chunk(sc, sg, ck, fin, prev, carry + nb[t] - own, dcs, entries + g)) bad = true;
    }
    carry += nb[kScanLanes - 1];
    cd0 += d0[kScanLanes - 1]; cd1 += d1[kScanLanes - 1]; cd2 += d2[kScanLanes - 1];
    __syncthreads();
  }
  if (bad) atomicOr(undecided + image, 1);
}

// The storing decode: every chunk of a decided image again from its proven entry.  An error, or a pass that does not
// end where the counting pass ended, marks the image undecided as well.
__global__ __launch_bounds__(YV4_JPEG_WG_CHUNKS) void jpeg_chunk_decode_kernel(
    const yv4_jpeg_scan* __restrict__ scans, const yv4_jpeg_segment* __restrict__ segs,
    const yv4_jpeg_chunk* __restrict__ chunks, const yv4_jpeg_wg* __restrict__ wgs, const uint8_t* __restrict__ bytes,
    const yv4_jpeg_huff* __restrict__ huff, const yv4_jpeg_entry* __restrict__ entries, int16_t* __restrict__ coef,
    int32_t* undecided, int chunk_bytes, int fin) {
  __shared__ yv4_jpeg_huff tabs[YV4_JPEG_MAX_HUFF];
  __shared__ uint8_t zigzag[64];
  const yv4_jpeg_wg wg = wgs[blockIdx.x];
  if (__syncthreads_or(undecided[wg.image] != 0)) return;
  const yv4_jpeg_scan sc = scans[wg.image];
  jpeg_load_tables(tabs, zigzag, huff, sc);
  if ((int)threadIdx.x >= wg.count) return;
  const int64_t g = (int64_t)wg.first_seg + (int)threadIdx.x;
  const yv4_jpeg_chunk ck = chunks[g];
  const yv4_jpeg_segment sg = segs[ck.seg];
  const yv4_jpeg_entry en = entries[g];
  jpeg::ChunkPass p;
  const int e = jpeg::decode_chunk<true>(sc, sg, bytes + sc.data_off, tabs, zigzag, ck.index, ck.count, chunk_bytes,
                                         en.entry, en.first_block, en.pred, coef + sc.coef_off, &p);
  const uint64_t want = fin ? en.exit[1] : en.exit[0];
  if (e || p.exit != want || p.nblk != en.nblk) atomicOr(undecided + wg.image, 2);
}

}  // namespace yv4

using namespace yv4;

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// What both device entries do between the validation and the first launch: the zero-fill of coef[lo, hi), of the status
// words and, for the chunk decode, of the undecided words.
static int jpeg_zero_fill(const char* who, int16_t* coef, int64_t lo, int64_t hi, int32_t* status, int32_t* undecided, int N,
                          hipStream_t s) {
  if (hipMemsetAsync(coef + lo, 0, (size_t)(hi - lo) * sizeof(int16_t), s) != hipSuccess ||
      hipMemsetAsync(status, 0, (size_t)N * sizeof(int32_t), s) != hipSuccess ||
      (undecided && hipMemsetAsync(undecided, 0, (size_t)N * sizeof(int32_t), s) != hipSuccess)) {
    (void)hipGetLastError();
    set_error("%s: the zero-fill of the coefficients failed", who);
    return YV4_E_LAUNCH;
  }
  return YV4_OK;
}

extern "C" int yv4_jpeg_entropy_decode_device(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                              const yv4_jpeg_wg* wgs, const yv4_jpeg_scan* scans_dev,
                                              const yv4_jpeg_segment* segs_dev, const yv4_jpeg_wg* wgs_dev, int N,
                                              int64_t nseg, int64_t nwg, const uint8_t* bytes, int64_t bytes_len,
                                              const yv4_jpeg_huff* huff, int64_t nhuff, int16_t* coef,
                                              int64_t coef_elems, int32_t* status, void* stream) {
  YV4_REQUIRE(scans && segs && wgs && scans_dev && segs_dev && wgs_dev && bytes && huff && coef && status,
              "jpeg_entropy_decode_device: null pointer");
  YV4_REQUIRE(aligned(scans_dev, 8) && aligned(segs_dev, 8) && aligned(wgs_dev, 4) && aligned(huff, 4) && aligned(coef, 2) &&
                  aligned(status, 4),
              "jpeg_entropy_decode_device: scans_dev / segs_dev must be 8-byte, wgs_dev / huff / status 4-byte aligned");
  int64_t lo, hi;
  const int st = jpeg_entropy_validate(scans, segs, wgs, N, nseg, nwg, bytes_len, nhuff, coef_elems, &lo, &hi);
  if (st != YV4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = jpeg_zero_fill("jpeg_entropy_decode_device", coef, lo, hi, status, nullptr, N, s)) return rc;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)nwg), dim3(YV4_JPEG_WG_SEGMENTS), 0, s, scans_dev, segs_dev,
                     wgs_dev, bytes, huff, coef, status);
  YV4_CHECK_LAUNCH("jpeg_entropy");
  return YV4_OK;
}

extern "C" int yv4_jpeg_entropy_decode_device_sync(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                                   const yv4_jpeg_chunk* chunks, const int32_t* seg_first,
                                                   const yv4_jpeg_wg* wgs, const yv4_jpeg_scan* scans_dev,
                                                   const yv4_jpeg_segment* segs_dev, const yv4_jpeg_chunk* chunks_dev,
                                                   const int32_t* seg_first_dev, const yv4_jpeg_wg* wgs_dev, int N,
                                                   int64_t nseg, int64_t nchunk, int64_t nwg, const uint8_t* bytes,
                                                   int64_t bytes_len, const yv4_jpeg_huff* huff, int64_t nhuff,
                                                   int32_t chunk_bytes, int32_t max_rounds, yv4_jpeg_entry* entries_dev,
                                                   int16_t* coef, int64_t coef_elems, int32_t* status,
                                                   int32_t* undecided, void* stream) {
  YV4_REQUIRE(scans && segs && chunks && seg_first && wgs && scans_dev && segs_dev && chunks_dev && seg_first_dev &&
                  wgs_dev && bytes && huff && entries_dev && coef && status && undecided,
              "jpeg_entropy_decode_device_sync: null pointer");
  YV4_REQUIRE(aligned(scans_dev, 8) && aligned(segs_dev, 8) && aligned(entries_dev, 8) && aligned(chunks_dev, 4) &&
                  aligned(seg_first_dev, 4) && aligned(wgs_dev, 4) && aligned(huff, 4) && aligned(coef, 2) &&
                  aligned(status, 4) && aligned(undecided, 4),
              "jpeg_entropy_decode_device_sync: scans_dev / segs_dev / entries_dev must be 8-byte, the other tables 4-byte "
              "aligned");
  int64_t lo, hi;
  const int st = jpeg_sync_validate(scans, segs, chunks, seg_first, wgs, N, nseg, nchunk, nwg, bytes_len, nhuff, chunk_bytes,
                                    max_rounds, coef_elems, &lo, &hi);
  if (st != YV4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = jpeg_zero_fill("jpeg_entropy_decode_device_sync", coef, lo, hi, status, undecided, N, s)) return rc;
  for (int r = 0; r <= max_rounds; ++r) {
    hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)nwg), dim3(YV4_JPEG_WG_CHUNKS), 0, s, scans_dev, segs_dev,
                       chunks_dev, wgs_dev, bytes, huff, entries_dev, (int)chunk_bytes, r);
    YV4_CHECK_LAUNCH("jpeg_sync");
  }
  const int fin = max_rounds & 1;
  hipLaunchKernelGGL(jpeg_chunk_scan_kernel, dim3((unsigned)nseg), dim3(kScanLanes), 0, s, scans_dev, segs_dev, chunks_dev,
                     seg_first_dev, entries_dev, undecided, fin);
  YV4_CHECK_LAUNCH("jpeg_chunk_scan");
  hipLaunchKernelGGL(jpeg_chunk_decode_kernel, dim3((unsigned)nwg), dim3(YV4_JPEG_WG_CHUNKS), 0, s, scans_dev, segs_dev,
                     chunks_dev, wgs_dev, bytes, huff, entries_dev, coef, undecided, (int)chunk_bytes, fin);
  YV4_CHECK_LAUNCH("jpeg_chunk_decode");
  return YV4_OK;
}
