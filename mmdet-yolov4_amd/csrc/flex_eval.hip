// metric='fast-bbox' (mean_ap_flexible.py) from the flat result table: the two pieces that let yv4_map_rank,
// yv4_iou_coco_batched and yv4_match_coco_batched score it without a visit to the host.
//   yv4_flex_tables      the matching kernel's Q = P * B problem tables (problem p, breakdown b -> q = p * B + b) from
//                        yv4_map_rank's det_off / iou_off: the breakdowns of a problem share its IoU block
//   yv4_flex_accumulate  per (class, breakdown, threshold): the breakdown mask compacts the class's list, integer
//                        cumulative counts over the compacted list, precision and recall in float64 and the 'area' AP
// The definition is stated in include/yv4.h and restated in mmdet-yolov4_amd/eval_utils.py.  Every floating-point value
// is ONE IEEE operation of it (compiled with -ffp-contract=off), counts are integers, the float64 sum is a single
// accumulator in rank order.  No float atomics: two runs give identical bytes.
// The problem search and the chunk primitives of the walk are eval_common.h's.
#include "eval_common.h"

namespace yv4 {
namespace {

__global__ __launch_bounds__(256) void fx_tables_kernel(const int64_t* __restrict__ det_off, const int64_t* __restrict__ iou_off,
                                                        int P, int B, int64_t* __restrict__ q_det_off,
                                                        int64_t* __restrict__ q_iou_off) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t Q = (int64_t)P * B;
  if (q > Q) return;
  if (q == Q) {
    q_det_off[Q] = (int64_t)B * det_off[P];
    q_iou_off[Q] = iou_off[P];
    return;
  }
  const int64_t p = q / B, b = q % B;
  const int64_t lo = det_off[p];
  q_det_off[q] = (int64_t)B * lo + b * (det_off[p + 1] - lo);
  q_iou_off[q] = iou_off[p];
}

struct FxArgs {
  const int32_t* matched;
  const float* det4;
  const int32_t* cls_order;
  const int64_t* det_off;
  const int64_t* gt_off;
  const uint8_t* gt_bkd;
  const float* bounds;
  int64_t D, G;
  int N, B, T, shared_tp;
};

// the class's pos-th detection by descending score: bit 0 = it stays in breakdown b's list at threshold t, bit 1 = it
// counts as a true positive there.  base / n: the class's slice of the problem-major order; pc = class * N.
__device__ __forceinline__ int fx_flags(const FxArgs& a, int64_t base, int64_t n, int64_t pc, int b, int t, int64_t pos) {
  const int64_t s = a.cls_order[base + pos];
  if (s < base || s >= base + n) return 0;                // (never with the tables yv4_map_rank wrote)
  const int64_t p = find_problem(a.det_off, pc, pc + a.N, s), first = a.det_off[p];
  const int64_t nd = a.det_off[p + 1] - first, d = s - first;
  const int64_t blk = (int64_t)a.B * first * a.T + (int64_t)t * nd + d;      // breakdown 0's entry
  const int32_t mg_own = a.matched[blk + (int64_t)b * nd * a.T];
  const int32_t mg_tp = a.shared_tp ? a.matched[blk + (int64_t)(a.B - 1) * nd * a.T] : mg_own;
  bool in;
  if (mg_own > -1) {
    const int64_t g = a.gt_off[p] + mg_own;
    in = g < a.gt_off[p + 1] && g < a.G && a.gt_bkd[(int64_t)b * a.G + g] != 0;
  } else if (b == 0) {
    in = true;
  } else {
    const float4 box = reinterpret_cast<const float4*>(a.det4)[s];
    const float w = box.z - box.x, h = box.w - box.y;
    const float area = w * h;
    in = area >= a.bounds[2 * (b - 1)] && area < a.bounds[2 * (b - 1) + 1];
  }
  return (in ? 1 : 0) | (mg_tp > -1 ? 2 : 0);
}

// One workgroup of four waves per (class, breakdown, threshold).  The class's list is walked in chunks of 256 positions
// (thread = position inside the chunk), three times:
//   A  forwards   inclusive integer counts of `in` and `in & tp` (chunk_count2; the chunks' through a running sum every
//                 thread keeps) -> precision at the `in` positions, -1 elsewhere
//   B  backwards  precision's suffix maximum over the `in` positions (chunk_suffix_max), in place in `scratch`; a
//                 position outside the list holds -1, below every precision, so a chunk without an `in` position passes
//                 the carry through
//   C  forwards   the `in & tp` counts again: recall changes exactly there, and the recall before it is (count - 1) /
//                 num_gt whatever lies between; the terms go in rank order into one float64 accumulator that every
//                 thread carries identically
__global__ __launch_bounds__(kEvalThreads) void fx_accumulate_kernel(FxArgs a, const int64_t* __restrict__ num_gt,
                                                                     double* __restrict__ scratch, int64_t* __restrict__ num_det,
                                                                     double* __restrict__ recall, float* __restrict__ ap) {
  __shared__ int s_in[kEvalWaves], s_tp[kEvalWaves];
  __shared__ double s_wmax[kEvalWaves];
  __shared__ unsigned long long s_mask[kEvalWaves];
  __shared__ double s_term[kEvalThreads];
  const int tid = threadIdx.x;
  int id = blockIdx.x;                                    // (c * B + b) * T + t: the index of the outputs
  const int t = id % a.T; id /= a.T;
  const int b = id % a.B;
  const int c = id / a.B;
  const int64_t pc = (int64_t)c * a.N;
  int64_t base = a.det_off[pc];
  int64_t n = a.det_off[pc + a.N] - base;
  if (base < 0 || base > a.D) { base = 0; n = 0; }        // (never with the tables yv4_map_rank wrote)
  if (n > a.D - base) n = a.D - base;
  if (n < 0) n = 0;
  const int64_t ng = num_gt[(int64_t)c * a.B + b];
  const double den = ng >= 1 ? (double)ng : 1e-7;         // max(num_gt, 1e-7)
  const int64_t nchunks = (n + kEvalThreads - 1) / kEvalThreads;
  double* mine = scratch + ((int64_t)b * a.T + t) * a.D + base;

  // ---- A
  int64_t run_in = 0, run_tp = 0;
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int64_t pos = ch * kEvalThreads + tid;
    const int f = pos < n ? fx_flags(a, base, n, pc, b, t, pos) : 0;
    const bool fin = (f & 1) != 0, ftp = f == 3;
    ChunkCount ci, ct;
    chunk_count2(fin, ftp, s_in, s_tp, ci, ct);
    if (pos < n) {
      const int64_t k = run_in + ci.incl;
      const int64_t ctp = run_tp + ct.incl;
      mine[pos] = fin ? (double)ctp / (double)k : -1.0;
    }
    run_in += ci.total;
    run_tp += ct.total;
    __syncthreads();
  }
  if (tid == 0) {
    num_det[blockIdx.x] = run_in;
    recall[blockIdx.x] = run_in > 0 ? (double)run_tp / den : 0.0;
  }
  if (run_tp == 0) {                                      // (uniform) no term: the sum is empty
    if (tid == 0) ap[blockIdx.x] = 0.f;
    return;
  }

  // ---- B (the pad mpre[n + 1] = 0 starts the maximum)
  double carry = 0.0;
  for (int64_t ch = nchunks - 1; ch >= 0; --ch) {
    const int64_t pos = ch * kEvalThreads + tid;
    const double own = pos < n ? mine[pos] : -1.0;
    const double v = chunk_suffix_max(own, carry, s_wmax);
    if (own >= 0.0) mine[pos] = v;
    __syncthreads();
  }

  // ---- C
  run_tp = 0;
  double acc = 0.0;
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int64_t pos = ch * kEvalThreads + tid;
    const bool step = pos < n && fx_flags(a, base, n, pc, b, t, pos) == 3;
    const ChunkCount ct = chunk_count(step, s_tp);
    double term = 0.0;
    if (step) {
      const int64_t ctp = run_tp + ct.incl;
      const double r = (double)ctp / den, r_prev = (double)(ctp - 1) / den;      // mrec[0] = 0 = 0 / den
      term = (r - r_prev) * mine[pos];
    }
    chunk_ordered_sum(term, step, acc, s_term, s_mask);
    run_tp += ct.total;
  }
  // the closing step to mrec[n + 1] = 1 meets mpre[n + 1] = 0: it adds a zero
  if (tid == 0) ap[blockIdx.x] = (float)acc;
}

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" int yv4_flex_tables(const int64_t* det_off, const int64_t* iou_off, int P, int B, int64_t* q_det_off,
                               int64_t* q_iou_off, void* stream) {
  YV4_REQUIRE(det_off && iou_off && q_det_off && q_iou_off, "flex_tables: null pointer");
  YV4_REQUIRE(P > 0 && B > 0 && (int64_t)P * B < 0x7fffffff, "flex_tables: P x B problems must be positive and fit 31 bits");
  const int64_t Q = (int64_t)P * B;
  hipLaunchKernelGGL(fx_tables_kernel, dim3((unsigned)(Q / 256 + 1)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     det_off, iou_off, P, B, q_det_off, q_iou_off);
  YV4_CHECK_LAUNCH("flex_tables");
  return YV4_OK;
}

extern "C" size_t yv4_flex_accumulate_work(int64_t total_det, int num_thrs, int num_bkd) {
  if (total_det < 0 || num_thrs <= 0 || num_bkd <= 0) return 0;
  return 8 * (size_t)num_thrs * (size_t)num_bkd * (size_t)(total_det > 0 ? total_det : 1);
}

extern "C" int yv4_flex_accumulate(const int32_t* matched, const float* det4, const int32_t* cls_order, const int64_t* det_off,
                                   const int64_t* gt_off, const uint8_t* gt_bkd, const int64_t* num_gt,
                                   const float* area_bounds, int64_t total_det, int64_t total_gt, int N, int C, int num_bkd,
                                   int num_thrs, int shared_tp, void* work, int64_t* num_det, double* recall, float* ap,
                                   void* stream) {
  YV4_REQUIRE(N > 0 && C > 0 && (int64_t)N * C < 0x7fffffff, "flex_accumulate: N x C problems must be positive and fit 31 bits");
  YV4_REQUIRE(num_thrs > 0 && num_bkd > 0 && (int64_t)C * num_bkd * num_thrs < 0x7fffffff,
              "flex_accumulate: classes x breakdowns x thresholds must be positive and fit 31 bits");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "flex_accumulate: cls_order is int32, so fewer than 2^31 detections");
  YV4_REQUIRE(total_gt >= 0, "flex_accumulate: negative gt count");
  YV4_REQUIRE(det_off && gt_off && num_gt && work && num_det && recall && ap, "flex_accumulate: null pointer");
  YV4_REQUIRE(total_det == 0 || (matched && det4 && cls_order), "flex_accumulate: null detection pointer");
  YV4_REQUIRE(total_gt == 0 || gt_bkd, "flex_accumulate: null gt_bkd");
  YV4_REQUIRE(num_bkd == 1 || area_bounds, "flex_accumulate: null area_bounds");
  YV4_REQUIRE(((uintptr_t)work & 7) == 0, "flex_accumulate: work must be 8-byte aligned");
  YV4_REQUIRE(((uintptr_t)det4 & 15) == 0, "flex_accumulate: det4 must be 16-byte aligned");
  FxArgs a;
  a.matched = matched;
  a.det4 = det4;
  a.cls_order = cls_order;
  a.det_off = det_off;
  a.gt_off = gt_off;
  a.gt_bkd = gt_bkd;
  a.bounds = area_bounds;
  a.D = total_det;
  a.G = total_gt;
  a.N = N;
  a.B = num_bkd;
  a.T = num_thrs;
  a.shared_tp = shared_tp != 0;
  hipLaunchKernelGGL(fx_accumulate_kernel, dim3((unsigned)((int64_t)C * num_bkd * num_thrs)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a, num_gt, reinterpret_cast<double*>(work), num_det, recall, ap);
  YV4_CHECK_LAUNCH("flex_accumulate");
  return YV4_OK;
}
