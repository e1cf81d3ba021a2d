// The library's stable LSD radix sort (rs_sort) and the carving of the workspaces it sorts in, shared by the hard and
// soft NMS split paths (nms_split.hip, soft_nms.hip), the top-k slot tables of test-time augmentation (tta.hip), the
// COCO evaluation (coco_eval.hip) and the flat-table mAP (map_flat.hip).  Kernels live in an unnamed namespace: each translation unit that includes this
// header gets its own copies.
#pragma once
#include "yv4_common.h"

namespace yv4 {
namespace {

// ---- stable LSD radix sort, 8 bits per pass (this path is cold: >= 10 000 candidates of one image; three launches per
// pass, nothing tuned).  Per pass: (a) every workgroup counts the digits of its tile of 1 024 keys -> hist[digit][tile];
// (b) one workgroup turns the digit-major table into exclusive offsets; (c) every workgroup scatters its tile, a key's
// position = offset[digit][tile] + its rank among the tile's earlier keys with the same digit.  A workgroup is ONE wave:
// tile order = (round, lane), so a rank is the running count of the digit over earlier rounds plus the number of lower
// lanes with the same digit in this round (eight ballots) -- no cross-wave ordering to get wrong.
constexpr int kRsLanes = 64;
constexpr int kRsRounds = 16;
constexpr int kRsTile = kRsLanes * kRsRounds;

// bytes of `hist` for rs_sort over n keys: the digit-major counters of a pass, hist[256][tiles]
inline size_t rs_hist_bytes(int64_t n) { return (size_t)256 * (size_t)((n + kRsTile - 1) / kRsTile) * 4; }

// Workspaces are carved into 256-byte aligned pieces: take(bytes) returns the piece's offset, `off` is the total so far.
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += align256(bytes); return o; }
};

// The pieces the hard and the soft split path have in common (n candidates of one image): three key and three label
// buffers (a / b and the sorts' other ping-pong side t), the segment bounds of up to kSplitMaxClasses labels and the
// sorts' counters.  Each path appends its own scratch to `carve`.
constexpr int kSplitMaxClasses = 65535;   // labels are < 65536 (16 radix bits)
struct SplitSortLayout {
  size_t keys_a, keys_b, keys_t, lab_a, lab_b, lab_t, seg, hist;
  Carve carve;
  explicit SplitSortLayout(int64_t n) {
    keys_a = carve.take((size_t)n * 8);
    keys_b = carve.take((size_t)n * 8);
    keys_t = carve.take((size_t)n * 8);
    lab_a = carve.take((size_t)n * 4);
    lab_b = carve.take((size_t)n * 4);
    lab_t = carve.take((size_t)n * 4);
    seg = carve.take((size_t)(kSplitMaxClasses + 2) * 8);
    hist = carve.take(rs_hist_bytes(n));
  }
};

template <class K>
__global__ __launch_bounds__(kRsLanes) void rs_hist_kernel(const K* __restrict__ keys, int64_t n, int shift,
                                                          uint32_t* __restrict__ hist, int ntiles) {
  __shared__ uint32_t cnt[256];
  const int lane = threadIdx.x;
  for (int i = lane; i < 256; i += kRsLanes) cnt[i] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRsTile;
#pragma unroll 4
  for (int r = 0; r < kRsRounds; ++r) {
    const int64_t idx = base + r * kRsLanes + lane;
    if (idx < n) atomicAdd(&cnt[(unsigned)(keys[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (int i = lane; i < 256; i += kRsLanes) hist[(int64_t)i * ntiles + blockIdx.x] = cnt[i];
}

// exclusive scan of `total` counters in place (their sum is n < 2^31): a thread sums its contiguous chunk, thread 0 scans
// the 1 024 chunk sums, the thread walks its chunk again
__global__ __launch_bounds__(1024) void rs_scan_kernel(uint32_t* __restrict__ h, int64_t total) {
  __shared__ uint32_t part[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (total + 1023) / 1024;
  const int64_t lo = t * chunk < total ? t * chunk : total;
  const int64_t hi = lo + chunk < total ? lo + chunk : total;
  uint32_t su = 0u;
  for (int64_t i = lo; i < hi; ++i) su += h[i];
  part[t] = su;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0u;
    for (int i = 0; i < 1024; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
  }
  __syncthreads();
  uint32_t run = part[t];
  for (int64_t i = lo; i < hi; ++i) { const uint32_t v = h[i]; h[i] = run; run += v; }
}

template <class K, class V, bool HAS_V>
__global__ __launch_bounds__(kRsLanes) void rs_scatter_kernel(const K* __restrict__ kin, K* __restrict__ kout,
                                                             const V* __restrict__ vin, V* __restrict__ vout, int64_t n,
                                                             int shift, const uint32_t* __restrict__ offs, int ntiles) {
  __shared__ uint32_t run[256];
  const int lane = threadIdx.x;
  for (int i = lane; i < 256; i += kRsLanes) run[i] = offs[(int64_t)i * ntiles + blockIdx.x];
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRsTile;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int r = 0; r < kRsRounds; ++r) {           // (uniform trip count: the barriers below are reached by every lane)
    const int64_t idx = base + r * kRsLanes + lane;
    const bool valid = idx < n;
    const K k = valid ? kin[idx] : (K)0;
    const unsigned d = (unsigned)(k >> shift) & 255u;
    unsigned long long peers = __ballot(valid);    // lanes of this round with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const unsigned rank = (unsigned)__popcll(peers & below);
    if (valid) {
      const uint32_t pos = run[d] + rank;
      kout[pos] = k;
      if (HAS_V) vout[pos] = vin[idx];
    }
    __syncthreads();                               // every read of run[] of this round is done
    if (valid && rank + 1u == (unsigned)__popcll(peers)) run[d] += (uint32_t)__popcll(peers);   // the group's highest lane
    __syncthreads();
  }
}

// Sorts `bits` low bits (a multiple of 16: an even number of passes) of n keys, ascending and stable; values follow when
// HAS_V.  The input is only read; the result lands in (kx, vx), (ky, vy) is the other side of the ping-pong.  `what`
// names the caller in the error message of a failed launch.
template <class K, class V, bool HAS_V>
static int rs_sort(const K* kin, K* kx, K* ky, const V* vin, V* vx, V* vy, int64_t n, int bits, uint32_t* hist, hipStream_t s,
                   const char* what = "nms_split: radix sort") {
  const int ntiles = (int)((n + kRsTile - 1) / kRsTile);   // rs_hist_bytes(n) = 256 * ntiles counters
  const K* sk = kin;
  const V* sv = vin;
  for (int pass = 0; pass * 8 < bits; ++pass) {
    K* dk = (pass & 1) ? kx : ky;
    V* dv = (pass & 1) ? vx : vy;
    hipLaunchKernelGGL(rs_hist_kernel<K>, dim3((unsigned)ntiles), dim3(kRsLanes), 0, s, sk, n, pass * 8, hist, ntiles);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, s, hist, (int64_t)256 * ntiles);
    hipLaunchKernelGGL((rs_scatter_kernel<K, V, HAS_V>), dim3((unsigned)ntiles), dim3(kRsLanes), 0, s, sk, dk, sv, dv, n,
                       pass * 8, hist, ntiles);
    sk = dk;
    sv = dv;
  }
  YV4_CHECK_LAUNCH(what);
  return YV4_OK;
}

}  // namespace
}  // namespace yv4
