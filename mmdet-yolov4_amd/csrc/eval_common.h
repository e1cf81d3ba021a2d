// Helpers shared by the evaluation kernels (eval.hip, map_eval.hip, map_flat.hip, flex_eval.hip, coco_eval.hip,
// recall.hip): the descending-score key, the problem search over an offset table, the offsets-from-sorted-keys kernel,
// the radix sorts' sizing, the box overlap of one pair and the three chunk primitives of the per-class walk of map_flat.hip / flex_eval.hip (the kernels keep their
// definitions: what counts, which IEEE operation gives precision and recall, what the AP mode selects).
// Translation units including this header must be built with -ffp-contract=off.
#pragma once
#include "radix_sort.h"
#include "yv4_common.h"

namespace yv4 {

// float32 score -> a 32-bit key that ascends as the score DEscends.  float32 -> float64 is monotone and injective, so
// ordering the float32 scores orders COCOeval's float64 ones; -0 and +0 compare equal there and share a key here.
__device__ __forceinline__ uint32_t desc_key(float s) {
  const uint32_t b = __float_as_uint(s + 0.f);
  const uint32_t u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~u;
}

// the last p in [lo, hi) with off[p] <= i (problems without elements share their offset with the next one and are
// stepped over); I: the problem index type of the caller (int, or int64_t beside 64-bit offsets)
template <typename I>
__device__ __forceinline__ I find_problem(const int64_t* __restrict__ off, I lo, I hi, int64_t i) {
  while (hi - lo > 1) {     // invariant: off[lo] <= i < off[hi]
    const I mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// first position of the n sorted keys that is >= key
template <typename K>
__device__ __forceinline__ int64_t key_lower_bound(const K* __restrict__ keys, int64_t n, K key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// off[q] = first sorted position whose (key >> kShift) is >= q, q = 0 .. Q (all 0 without keys)
template <typename K, int kShift>
__global__ __launch_bounds__(256) void offsets_kernel(const K* __restrict__ keys, int64_t n, int Q,
                                                      int64_t* __restrict__ off) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > Q) return;
  off[q] = n > 0 ? key_lower_bound<K>(keys, n, (K)(uint32_t)q << kShift) : 0;
}

// radix bits of a 64-bit key whose high word holds 0 .. max_hi above a 32-bit score key
static inline int key_bits_hi32(int max_hi) { return max_hi < 65535 ? 48 : 64; }
// the sorts' counters: reserves one tile more than rs_sort counts
static inline size_t sort_hist_bytes(int64_t n) { return rs_hist_bytes(n + kRsTile); }

// ---- the reference's numpy box overlap (bbox_overlaps.py:4-48) for one pair: map_eval.hip and recall.hip -------------
// np.maximum / np.minimum: a NaN in either operand is the result (fmaxf would drop it)
__device__ __forceinline__ float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }

__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x) * (b.w - b.y); }

// out = the overlap of a (a float4: the box of the first argument) and b (of the second); iof divides by a's area.
// fp32, the reference's operation order.  A statement macro on purpose: as a function of any signature (float4 by value
// or by reference, eight scalars) it changed how the compiler pairs the loads and subtractions of bbox_overlaps_kernel,
// and with them that kernel's machine code; expanded in place the kernel compiles to the bytes it had with the
// expression written out (tools/kernel_isa_diff.py).
#define YV4_BOX_OVERLAP(out, a, b, iof, eps)                                                \
  do {                                                                                      \
    const float xs_ = np_max((a).x, (b).x), ys_ = np_max((a).y, (b).y);                     \
    const float xe_ = np_min((a).z, (b).z), ye_ = np_min((a).w, (b).w);                     \
    const float overlap_ = np_max(xe_ - xs_, 0.f) * np_max(ye_ - ys_, 0.f);                 \
    float uni_ = box_area(a);                                                               \
    if (!(iof)) uni_ = (uni_ + box_area(b)) - overlap_;                                     \
    uni_ = np_max(uni_, eps);                                                               \
    (out) = overlap_ / uni_;                                                                \
  } while (0)

// ---- the chunked walk of a list by a workgroup of kEvalWaves waves: thread = position inside a chunk of kEvalThreads ---
// Each primitive puts ONE barrier between its LDS writes and its reads and takes its LDS arrays from the kernel.  Before
// the same array is written again every thread must have passed another barrier: another primitive's in the same loop
// body, or a __syncthreads() that closes the body.
constexpr int kEvalLanes = 64;
constexpr int kEvalWaves = 4;
constexpr int kEvalThreads = kEvalLanes * kEvalWaves;

struct ChunkCount {
  int incl;       // flagged positions of the chunk up to and including this thread's
  int total;      // flagged positions of the chunk
};

__device__ __forceinline__ ChunkCount chunk_count_finish(unsigned long long ballot, const int (&s_cnt)[kEvalWaves]) {
  const int lane = threadIdx.x & (kEvalLanes - 1), w = threadIdx.x >> 6;
  const unsigned long long le = ~0ull >> (63 - lane);     // lanes <= mine
  int pre = 0, tot = 0;
#pragma unroll
  for (int v = 0; v < kEvalWaves; ++v) {
    const int a = s_cnt[v];
    if (v < w) pre += a;
    tot += a;
  }
  return {pre + (int)__popcll(ballot & le), tot};
}

// forward counts of one predicate: a ballot inside the wave, the waves' totals through s_cnt
__device__ __forceinline__ ChunkCount chunk_count(bool flag, int (&s_cnt)[kEvalWaves]) {
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & (kEvalLanes - 1)) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  return chunk_count_finish(b, s_cnt);
}

// ... of two predicates behind one barrier
__device__ __forceinline__ void chunk_count2(bool flag0, bool flag1, int (&s_cnt0)[kEvalWaves], int (&s_cnt1)[kEvalWaves],
                                             ChunkCount& c0, ChunkCount& c1) {
  const unsigned long long b0 = __ballot(flag0), b1 = __ballot(flag1);
  if ((threadIdx.x & (kEvalLanes - 1)) == 0) {
    s_cnt0[threadIdx.x >> 6] = __popcll(b0);
    s_cnt1[threadIdx.x >> 6] = __popcll(b1);
  }
  __syncthreads();
  c0 = chunk_count_finish(b0, s_cnt0);
  c1 = chunk_count_finish(b1, s_cnt1);
}

// backward maximum, the chunks taken last to first.  v: this position's value (the caller's filler outside the list);
// carry: the maximum over the chunks above, updated to include this one.  Returns the maximum over this position and
// everything above it: shuffles inside the wave, the waves above through s_wmax, the chunks above through carry.
template <typename T>      // float or double: fmax is overloaded
__device__ __forceinline__ T chunk_suffix_max(T v, T& carry, T (&s_wmax)[kEvalWaves]) {
  const int lane = threadIdx.x & (kEvalLanes - 1), w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < kEvalLanes; o <<= 1) {
    const T u = __shfl_down(v, o);
    if (lane + o < kEvalLanes) v = fmax(v, u);
  }
  if (lane == 0) s_wmax[w] = v;
  __syncthreads();
  T above = carry, all = carry;
#pragma unroll
  for (int x = 0; x < kEvalWaves; ++x) {
    const T m = s_wmax[x];
    if (x > w) above = fmax(above, m);
    all = fmax(all, m);
  }
  carry = all;
  return fmax(v, above);
}

// acc += the chunk's terms at the positions with `step`, in position order: every thread adds them all into its own
// copy of the single float64 accumulator, so the copies stay identical
__device__ __forceinline__ void chunk_ordered_sum(double term, bool step, double& acc, double (&s_term)[kEvalThreads],
                                                  unsigned long long (&s_mask)[kEvalWaves]) {
  s_term[threadIdx.x] = term;
  const unsigned long long m = __ballot(step);
  if ((threadIdx.x & (kEvalLanes - 1)) == 0) s_mask[threadIdx.x >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < kEvalWaves; ++v) {
    unsigned long long mm = s_mask[v];
    while (mm) {
      acc += s_term[v * kEvalLanes + (__ffsll(mm) - 1)];
      mm &= mm - 1;
    }
  }
}

}  // namespace yv4
