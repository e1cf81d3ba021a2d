// Proposal recall (include/yv4.h, "proposal recall"): mmdet/core/evaluation/recall.py's _recalls for every image and
// every proposal number of a dataset in one launch, behind yv4_map_rank (C = 1), which leaves the boxes image-major in
// descending-score order.  The definition is restated in tests/_recall_ref.py.
//   One workgroup of four waves per pair (image i, proposal number k).  G = the image's gts, n = its boxes,
//   cols = min(n, prop_nums[M-1]), c = min(cols, prop_nums[k]).  The (G x c) IoU block is never stored: every IoU is
//   computed from the two boxes (eval_common.h's YV4_BOX_OVERLAP, the expression of bbox_overlaps_kernel) when a row is
//   scanned.
//   State per row: its current maximum over the live columns and the first column that holds it; the removed columns
//   are a bit mask.  A row scan is one wave's: lane = column inside a chunk of 64, then a butterfly that keeps the lowest
//   column among equal IoUs.
//   A greedy step (recall.py:24-31) is a workgroup reduction to the lowest row with the largest maximum; that value is
//   recorded, the row and its column leave, and only the live rows whose cached column was the removed one are
//   scanned again (the plain form scans every row at every step).  A removed row holds -1, as the reference's block
//   does; once the winner is -1 no live column is left and every further step records -1.
//   Forms: a pair with G + c <= the LDS cap keeps its boxes and its state in LDS; a larger one reads the boxes from the
//   tables and keeps its state in its own slice of the workspace.  Nothing is truncated.
//   Counts: thread t owns threshold t and counts the recorded values that reach it (float32 widened, compared in
//   float64); one 64-bit integer atomicAdd per pair and threshold.  No float atomics: two runs give identical bytes.
#include <climits>

#include "eval_common.h"

namespace yv4 {
namespace {

constexpr int kRcMaxNums = 16;                 // proposal numbers of a call (they travel as a kernel argument)
constexpr int kRcMaxThrs = kEvalThreads;       // thresholds of a call: one thread each
constexpr int kRcLdsBoxes = 1280;              // the LDS form's cap on G + c (boxes: 20 KiB, state: 15 KiB)
constexpr int kRcLdsWords = kRcLdsBoxes / 64;  // the column mask of the LDS form
constexpr int kRcMaxBlocks = 1 << 18;          // the grid; pairs beyond it are taken in a grid-stride loop

struct RcNums {
  int32_t v[kRcMaxNums];
};

// an image's slice of an offset table of `total` elements, clamped to it
__device__ __forceinline__ void rc_slice(const int64_t* __restrict__ off, int64_t i, int64_t total, int64_t& lo, int64_t& n) {
  lo = off[i];
  n = off[i + 1] - lo;
  if (lo < 0 || lo > total) { lo = 0; n = 0; }
  if (n > total - lo) n = total - lo;
  if (n < 0) n = 0;
}

// (value, index): the larger value wins, the lower index among equal values -- argmax's first occurrence
__device__ __forceinline__ bool rc_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the best (value, index) of a wave in every lane; x travels with it
__device__ __forceinline__ void rc_wave_best(float& v, int& i, int& x) {
#pragma unroll
  for (int o = kEvalLanes / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o), ox = __shfl_xor(x, o);
    if (rc_better(ov, oi, v, i)) { v = ov; i = oi; x = ox; }
  }
}

// One wave scans a row over the live columns of [0, c): its maximum and the first column holding it.  Without a live
// column the row is the reference's all -1 row: maximum -1 at column 0.
__device__ __forceinline__ void rc_scan_row(const float4 a, const float4* pb, int c, const unsigned long long* mask,
                                            float eps, float& best, int& arg) {
  const int lane = threadIdx.x & (kEvalLanes - 1);
  best = -1.f;
  arg = INT_MAX;
  for (int lo = 0; lo < c; lo += kEvalLanes) {
    const int col = lo + lane;
    if (col < c && !(mask && ((mask[lo >> 6] >> lane) & 1ull))) {
      const float4 b = pb[col];
      float v;
      YV4_BOX_OVERLAP(v, a, b, 0, eps);
      if (v > best) { best = v; arg = col; }          // strictly: a lane's columns ascend
    }
  }
  int x = 0;
  rc_wave_best(best, arg, x);
  if (arg == INT_MAX) arg = 0;
}

struct RcShared {
  float val[kEvalWaves];
  int row[kEvalWaves], arg[kEvalWaves];
  int n;                                        // rows on the list
};

// The G greedy steps of one pair.  gb (G) / pb (c) boxes; rmax, rarg, list (G) and mask (ceil(c / 64)) are the pair's
// own, in LDS or in the workspace; out (G) or null.  Returns, in thread t < T, the recorded values that reach thrs[t].
__device__ __forceinline__ long long rc_pair(const float4* gb, const float4* pb, int G, int c, float* rmax, int* rarg,
                                             int* list, unsigned long long* mask, RcShared& sh, float eps, double thr,
                                             float* out) {
  const int tid = threadIdx.x, lane = tid & (kEvalLanes - 1), w = tid >> 6;
  for (int g = w; g < G; g += kEvalWaves) {               // every row's first scan: no column is removed yet
    float best;
    int arg;
    rc_scan_row(gb[g], pb, c, nullptr, eps, best, arg);
    if (lane == 0) { rmax[g] = best; rarg[g] = arg; }
  }
  __syncthreads();
  long long cnt = 0;
  int j = 0;
  for (; j < G; ++j) {
    float bv = -2.f;                                        // below a removed row's -1: a thread without rows
    int br = INT_MAX, ba = 0;
    for (int g = tid; g < G; g += kEvalThreads) {
      const float v = rmax[g];
      if (v > bv) { bv = v; br = g; ba = rarg[g]; }         // strictly: a thread's rows ascend
    }
    rc_wave_best(bv, br, ba);
    if (lane == 0) { sh.val[w] = bv; sh.row[w] = br; sh.arg[w] = ba; }
    if (tid == 0) sh.n = 0;
    __syncthreads();                                        // A: the waves' candidates
    bv = sh.val[0]; br = sh.row[0]; ba = sh.arg[0];
#pragma unroll
    for (int v = 1; v < kEvalWaves; ++v)
      if (rc_better(sh.val[v], sh.row[v], bv, br)) { bv = sh.val[v]; br = sh.row[v]; ba = sh.arg[v]; }
    if (bv < 0.f) break;                                    // uniform: no live column is left
    if ((double)bv >= thr) ++cnt;
    if (tid == 0) {
      if (out) out[j] = bv;
      rmax[br] = -1.f;
      rarg[br] = -1;
      mask[ba >> 6] |= 1ull << (ba & 63);
    }
    for (int g = tid; g < G; g += kEvalThreads)             // the live rows that lose their cached column
      if (g != br && rarg[g] == ba) list[atomicAdd(&sh.n, 1)] = g;
    __syncthreads();                                        // B: the mask and the list
    const int nl = sh.n;
    for (int e = w; e < nl; e += kEvalWaves) {
      const int g = list[e];
      float best;
      int arg;
      rc_scan_row(gb[g], pb, c, mask, eps, best, arg);
      if (lane == 0) { rmax[g] = best; rarg[g] = arg; }
    }
    __syncthreads();                                        // C: the rows' new maxima
  }
  if (j < G) {                                              // the surplus steps record -1
    if (out)
      for (int x = j + tid; x < G; x += kEvalThreads) out[x] = -1.f;
    if (-1.0 >= thr) cnt += G - j;
  }
  return cnt;
}

__global__ __launch_bounds__(kEvalThreads) void recall_match_kernel(
    const float4* __restrict__ det4, const int64_t* __restrict__ det_off, const float4* __restrict__ gt4,
    const int64_t* __restrict__ gt_off, int N, int64_t D, int64_t Gt, RcNums nums, int M, const double* __restrict__ thrs,
    int T, float eps, int lds_cap, unsigned long long* w_mask, int64_t mask_words, float* w_rmax, int* w_rarg,
    int* w_list, float* gt_ious, unsigned long long* counts) {
  __shared__ float4 s_box[kRcLdsBoxes];
  __shared__ float s_rmax[kRcLdsBoxes];
  __shared__ int s_rarg[kRcLdsBoxes], s_list[kRcLdsBoxes];
  __shared__ unsigned long long s_mask[kRcLdsWords];
  __shared__ RcShared sh;
  const int tid = threadIdx.x;
  const double thr = tid < T ? thrs[tid] : 0.0;
  const int64_t pairs = (int64_t)N * M;
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t i = pair / M;
    const int k = (int)(pair % M);
    int64_t g0, gn, d0, dn;
    rc_slice(gt_off, i, Gt, g0, gn);
    if (gn == 0) continue;                                  // an image without gts records nothing (uniform)
    rc_slice(det_off, i, D, d0, dn);
    const int G = (int)gn;
    const int64_t cols = dn < nums.v[M - 1] ? dn : nums.v[M - 1];
    const int c = (int)(cols < nums.v[k] ? cols : nums.v[k]);
    float* out = gt_ious ? gt_ious + (int64_t)k * Gt + g0 : nullptr;
    long long cnt = 0;
    if (c == 0) {                                           // gts and no columns: G zeros (recall.py:21-23)
      if (out)
        for (int x = tid; x < G; x += kEvalThreads) out[x] = 0.f;
      if (0.0 >= thr) cnt = G;
    } else if (G + c <= lds_cap) {
      for (int x = tid; x < G; x += kEvalThreads) s_box[x] = gt4[g0 + x];
      for (int x = tid; x < c; x += kEvalThreads) s_box[G + x] = det4[d0 + x];
      for (int x = tid; x < (c + 63) / 64; x += kEvalThreads) s_mask[x] = 0;
      __syncthreads();
      cnt = rc_pair(s_box, s_box + G, G, c, s_rmax, s_rarg, s_list, s_mask, sh, eps, thr, out);
    } else {
      // the pair's slices of the workspace: rows at the gts' own positions, mask words at d0 / 64 + i (an image of n
      // boxes owns at most n / 64 + 1 words, so the images' slices are disjoint and end below D / 64 + N)
      const int64_t row0 = (int64_t)k * Gt + g0;
      unsigned long long* mask = w_mask + (int64_t)k * mask_words + d0 / 64 + i;
      for (int x = tid; x < (c + 63) / 64; x += kEvalThreads) mask[x] = 0;
      __syncthreads();
      cnt = rc_pair(gt4 + g0, det4 + d0, G, c, w_rmax + row0, w_rarg + row0, w_list + row0, mask, sh, eps, thr, out);
    }
    if (tid < T && cnt) atomicAdd(&counts[(int64_t)k * T + tid], (unsigned long long)cnt);
    __syncthreads();                                        // before the next pair stages its boxes
  }
}

static inline int64_t rc_mask_words(int64_t total_det, int N) { return total_det / 64 + N + 1; }

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" size_t yv4_recall_work(int64_t total_det, int64_t total_gt, int N, int M) {
  if (total_det < 0 || total_gt < 0 || N <= 0 || M <= 0 || M > kRcMaxNums) return 0;
  // mask words (8 bytes) first, then rmax | rarg | list, (M, total_gt) each
  return 8 * (size_t)M * (size_t)rc_mask_words(total_det, N) + 12 * (size_t)M * (size_t)total_gt + 8;
}

extern "C" int yv4_recall_match(const float* det4, const int64_t* det_off, const float* gt4, const int64_t* gt_off,
                                int64_t off_elems, int N, int64_t total_det, int64_t total_gt, const int32_t* prop_nums,
                                int M, const double* iou_thrs, int T, float eps, int lds_cap, void* work, size_t work_bytes,
                                float* gt_ious, int64_t gt_ious_elems, int64_t* counts, int64_t counts_elems,
                                void* stream) {
  YV4_REQUIRE(N > 0, "recall_match: N must be positive");
  YV4_REQUIRE(M > 0 && M <= kRcMaxNums, "recall_match: %d proposal numbers, 1 .. %d are taken", M, kRcMaxNums);
  YV4_REQUIRE(T > 0 && T <= kRcMaxThrs, "recall_match: %d thresholds, 1 .. %d are taken", T, kRcMaxThrs);
  YV4_REQUIRE((int64_t)N * M < 0x7fffffff, "recall_match: N x M pairs must fit 31 bits");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "recall_match: more than 2^31 boxes");
  YV4_REQUIRE(total_gt >= 0 && total_gt < 0x7fffffff, "recall_match: more than 2^31 gts");
  YV4_REQUIRE(lds_cap >= 0, "recall_match: negative lds_cap");
  YV4_REQUIRE(det_off && gt_off && prop_nums && iou_thrs && counts && work, "recall_match: null pointer");
  YV4_REQUIRE(total_det == 0 || det4, "recall_match: null det4");
  YV4_REQUIRE(total_gt == 0 || gt4, "recall_match: null gt4");
  for (int k = 0; k < M; ++k) YV4_REQUIRE(prop_nums[k] >= 0, "recall_match: proposal number %d is negative", k);
  YV4_REQUIRE(off_elems >= (int64_t)N + 1, "recall_match: det_off / gt_off hold %lld entries, %d images need %lld",
              (long long)off_elems, N, (long long)N + 1);
  YV4_REQUIRE(!gt_ious || gt_ious_elems >= (int64_t)M * total_gt, "recall_match: gt_ious holds %lld values, %d x %lld gts need %lld",
              (long long)gt_ious_elems, M, (long long)total_gt, (long long)((int64_t)M * total_gt));
  YV4_REQUIRE(counts_elems >= (int64_t)M * T, "recall_match: counts holds %lld values, %d x %d are needed",
              (long long)counts_elems, M, T);
  YV4_REQUIRE(work_bytes >= yv4_recall_work(total_det, total_gt, N, M), "recall_match: work holds %zu bytes, %zu needed",
              work_bytes, yv4_recall_work(total_det, total_gt, N, M));
  YV4_REQUIRE(((uintptr_t)work & 7) == 0, "recall_match: work must be 8-byte aligned");
  YV4_REQUIRE((((uintptr_t)det4 | (uintptr_t)gt4) & 15) == 0, "recall_match: boxes must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)M * (size_t)T, s) != hipSuccess) {
    set_error("recall_match: memset failed");
    return YV4_E_LAUNCH;
  }
  if (total_gt == 0) return YV4_OK;                         // no image records anything
  RcNums nums{};
  for (int k = 0; k < M; ++k) nums.v[k] = prop_nums[k];
  const int64_t words = rc_mask_words(total_det, N);
  unsigned long long* w_mask = reinterpret_cast<unsigned long long*>(work);
  float* w_rmax = reinterpret_cast<float*>(w_mask + (int64_t)M * words);
  int* w_rarg = reinterpret_cast<int*>(w_rmax + (int64_t)M * total_gt);
  int* w_list = w_rarg + (int64_t)M * total_gt;
  const int cap = lds_cap == 0 || lds_cap > kRcLdsBoxes ? kRcLdsBoxes : lds_cap;
  const int64_t pairs = (int64_t)N * M;
  hipLaunchKernelGGL(recall_match_kernel, dim3((unsigned)(pairs < kRcMaxBlocks ? pairs : kRcMaxBlocks)), dim3(kEvalThreads),
                     0, s, reinterpret_cast<const float4*>(det4), det_off, reinterpret_cast<const float4*>(gt4), gt_off, N,
                     total_det, total_gt, nums, M, iou_thrs, T, eps, cap, w_mask, words, w_rmax, w_rarg, w_list, gt_ious,
                     reinterpret_cast<unsigned long long*>(counts));
  YV4_CHECK_LAUNCH("recall_match");
  return YV4_OK;
}
