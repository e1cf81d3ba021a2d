// VOC-style mAP kernels: the reference's numpy box overlaps and its two true/false-positive rules
//   mmdet/core/evaluation/bbox_overlaps.py:4-48   bbox_overlaps(bboxes1, bboxes2, mode, eps)
//   mmdet/core/evaluation/mean_ap.py:153-237      tpfp_default
//   mmdet/core/evaluation/mean_ap.py:59-150       tpfp_imagenet
// (called per image and class, once per IoU threshold, from eval_map), batched like eval.hip: one call evaluates every
// (image, class) problem of a dataset, every IoU threshold and every area range.  Problem p owns boxes
// [off1[p], off1[p+1]) / [off2[p], off2[p+1]) and the row-major (n1 x n2) IoU block at iou_off[p].
// Arithmetic is the reference's fp32 expression order (compiled with -ffp-contract=off): bit-exact.
// The problem search over an offset table is eval_common.h's find_problem.
#include "eval_common.h"

namespace yv4 {
namespace {

// One thread per pair (the expression is eval_common.h's YV4_BOX_OVERLAP; np_max / np_min / box_area live there too).
// The reference swaps its operands when rows > cols (bbox_overlaps.py:27-30) and transposes the result back; per pair
// that only turns area1 + area2 into area2 + area1, and an IEEE add is commutative, so no bit of the result depends on
// the swap ('iof' keeps the FIRST argument's area through the swap, line 43).  This kernel
// therefore never swaps.
__global__ __launch_bounds__(256) void bbox_overlaps_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                            const int64_t* __restrict__ off1,
                                                            const int64_t* __restrict__ off2,
                                                            const int64_t* __restrict__ iou_off, int P, int iof,
                                                            float eps, float* __restrict__ iou) {
  const int64_t total = iou_off[P];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int p = find_problem(iou_off, 0, P, i);
    const int64_t n2 = off2[p + 1] - off2[p];
    const int64_t local = i - iou_off[p];
    const float4 a = reinterpret_cast<const float4*>(b1)[off1[p] + local / n2];
    const float4 b = reinterpret_cast<const float4*>(b2)[off2[p] + local % n2];
    YV4_BOX_OVERLAP(iou[i], a, b, iof, eps);
  }
}

// ---- tpfp, pass 1 of the default rule: one thread per detection -------------------------------------------------------
// Row maximum and its first-occurrence argmax (ious.max(axis=1) / ious.argmax(axis=1)), then for every threshold the
// detection reaches, an integer atomicMin of its rank into winner[t][gt].  The reference's sequential rule "the first
// detection in score order that hits a gt is its true positive, later ones are false positives" is exactly "the
// detection of minimum rank among those with argmax == g and max >= thr_t": a detection whose best gt is ignored or out
// of the area range is neither and never marks the gt covered, and for a gt that is neither, every such detection
// competes, so the minimum does not depend on the area range.  An integer minimum is order-independent: deterministic.
__global__ __launch_bounds__(256) void tpfp_rowmax_kernel(const float* __restrict__ iou, const int64_t* __restrict__ det_off,
                                                          const int64_t* __restrict__ gt_off,
                                                          const int64_t* __restrict__ iou_off, int P, int64_t D,
                                                          int64_t G, const int32_t* __restrict__ rank,
                                                          const float* __restrict__ thrs, int T,
                                                          float* __restrict__ row_max, int32_t* __restrict__ row_arg,
                                                          int32_t* __restrict__ det_prob, int32_t* __restrict__ winner) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const int p = find_problem(det_off, 0, P, d);
  const int64_t ng = gt_off[p + 1] - gt_off[p];
  float best = -INFINITY;
  int32_t arg = -1;
  if (ng > 0) {
    const float* row = iou + iou_off[p] + (d - det_off[p]) * ng;
    best = row[0];
    arg = 0;
    for (int64_t g = 1; g < ng; ++g) {
      const float v = row[g];
      if (v > best) { best = v; arg = (int32_t)g; }
    }
    const int32_t r = rank[d];
    for (int t = 0; t < T; ++t)
      if (best >= thrs[t]) atomicMin(&winner[(int64_t)t * G + gt_off[p] + arg], r);
  }
  row_max[d] = best;
  row_arg[d] = arg;
  det_prob[d] = p;          // the classification pass reads the problem instead of searching for it per (t, k)
}

// ---- tpfp, pass 1 of the imagenet rule: one thread per (problem, threshold) -------------------------------------------
// mean_ap.py:121-139 as written: detections in score order take the best still-uncovered gt whose IoU reaches the gt's
// own threshold min(ratio_g, thr_t) (strictly-greater comparison: the first maximum wins); the gt is covered whether it
// is ignored or not.  The walk does not depend on the area range.
__global__ __launch_bounds__(64) void tpfp_imagenet_walk_kernel(const float* __restrict__ iou, const int64_t* __restrict__ det_off,
                                                                const int64_t* __restrict__ gt_off,
                                                                const int64_t* __restrict__ iou_off, int P, int64_t D,
                                                                int64_t G, const int32_t* __restrict__ order,
                                                                const float* __restrict__ gt_ratio,
                                                                const float* __restrict__ thrs, int T,
                                                                uint8_t* __restrict__ covered, int32_t* __restrict__ matched,
                                                                int32_t* __restrict__ det_prob) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)P * T) return;
  const int p = (int)(id / T);
  const int t = (int)(id % T);
  const int64_t nd = det_off[p + 1] - det_off[p];
  const int64_t ng = gt_off[p + 1] - gt_off[p];
  const float* m = iou + iou_off[p];
  const float* ratio = gt_ratio + gt_off[p];
  const int32_t* ord = order + det_off[p];
  uint8_t* used = covered + ((int64_t)t * G + gt_off[p]);
  int32_t* out = matched + ((int64_t)t * D + det_off[p]);
  const float thr = thrs[t];
  for (int64_t g = 0; g < ng; ++g) used[g] = 0;
  for (int64_t s = 0; s < nd; ++s) {
    const int64_t d = ord[s];
    float best = -1.f;
    int32_t mg = -1;
    for (int64_t g = 0; g < ng; ++g) {
      if (used[g]) continue;
      const float v = m[d * ng + g];
      if (v >= np_min(ratio[g], thr) && v > best) { best = v; mg = (int32_t)g; }
    }
    if (mg >= 0) used[mg] = 1;
    out[d] = mg;
    if (t == 0) det_prob[det_off[p] + d] = p;
  }
}

// ---- tpfp, pass 2 of both rules: one thread per (threshold, area range, detection) ------------------------------------
// area == nullptr: the single "no range" column (everything in range).
__global__ __launch_bounds__(256) void tpfp_classify_kernel(const float* __restrict__ det, const float* __restrict__ gt,
                                                            const uint8_t* __restrict__ gt_ignore,
                                                            const int32_t* __restrict__ det_prob,
                                                            const int64_t* __restrict__ gt_off, int64_t D, int64_t G,
                                                            const int32_t* __restrict__ rank, const float* __restrict__ thrs,
                                                            int T, const float* __restrict__ area, int K, int imagenet,
                                                            const float* __restrict__ row_max,
                                                            const int32_t* __restrict__ row_arg,
                                                            const int32_t* __restrict__ winner,
                                                            const int32_t* __restrict__ matched, uint8_t* __restrict__ tp,
                                                            uint8_t* __restrict__ fp) {
  const int64_t total = (int64_t)T * K * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t d = i % D;
    const int k = (int)((i / D) % K);
    const int t = (int)(i / (D * K));
    const int p = det_prob[d];
    const float lo = area ? area[2 * k] : 0.f, hi = area ? area[2 * k + 1] : 0.f;
    int32_t g;
    if (imagenet) g = matched[(int64_t)t * D + d];
    else g = (row_arg[d] >= 0 && row_max[d] >= thrs[t]) ? row_arg[d] : -1;
    uint8_t is_tp = 0, is_fp = 0;
    if (g >= 0) {
      const int64_t gg = gt_off[p] + g;
      bool skip = gt_ignore[gg] != 0;
      if (!skip && area) {
        const float ga = box_area(reinterpret_cast<const float4*>(gt)[gg]);
        skip = (ga < lo) || (ga >= hi);
      }
      if (!skip) {
        if (imagenet || winner[(int64_t)t * G + gg] == rank[d]) is_tp = 1; else is_fp = 1;
      }
    } else if (!area) {
      is_fp = 1;
    } else {
      const float da = box_area(reinterpret_cast<const float4*>(det)[d]);
      is_fp = (da >= lo && da < hi) ? 1 : 0;
    }
    tp[i] = is_tp;
    fp[i] = is_fp;
  }
}

static inline unsigned map_blocks(long long n, int per) {
  long long b = (n + per - 1) / per;
  if (b > 256 * 32) b = 256 * 32;
  return (unsigned)b;
}

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" int yv4_bbox_overlaps_batched(const float* boxes1, const float* boxes2, const int64_t* off1, const int64_t* off2,
                                         const int64_t* iou_off, int P, int64_t total_pairs, int mode, float eps,
                                         float* iou, void* stream) {
  YV4_REQUIRE(P > 0 && off1 && off2 && iou_off, "bbox_overlaps: bad problem table");
  YV4_REQUIRE(mode == YV4_OVERLAPS_IOU || mode == YV4_OVERLAPS_IOF, "bbox_overlaps: mode must be YV4_OVERLAPS_IOU or _IOF");
  YV4_REQUIRE(total_pairs >= 0, "bbox_overlaps: negative pair count");
  if (total_pairs == 0) return YV4_OK;
  YV4_REQUIRE(boxes1 && boxes2 && iou, "bbox_overlaps: null pointer");
  YV4_REQUIRE((((uintptr_t)boxes1 | (uintptr_t)boxes2) & 15) == 0, "bbox_overlaps: boxes must be 16-byte aligned");
  hipLaunchKernelGGL(bbox_overlaps_kernel, dim3(map_blocks(total_pairs, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), boxes1, boxes2, off1, off2, iou_off, P,
                     mode == YV4_OVERLAPS_IOF ? 1 : 0, eps, iou);
  YV4_CHECK_LAUNCH("bbox_overlaps");
  return YV4_OK;
}

extern "C" size_t yv4_tpfp_work(int mode, int64_t total_det, int64_t total_gt, int num_thrs) {
  if (total_det < 0 || total_gt < 0 || num_thrs <= 0) return 0;
  const size_t D = (size_t)total_det, G = (size_t)total_gt, T = (size_t)num_thrs;
  // every detection's problem, int32 [D], in both; then
  if (mode == YV4_TPFP_IMAGENET) return 4 * D + 4 * T * D + T * G;   // matched int32 [T][D] | covered bytes [T][G]
  return 4 * D + 4 * T * G + 8 * D;                                   // winner int32 [T][G] | row_max float [D] | row_arg int32 [D]
}

extern "C" int yv4_tpfp_batched(int mode, const float* det, const float* gt, const uint8_t* gt_ignore,
                                const float* gt_ratio, const int32_t* order, const int32_t* rank, const int64_t* det_off,
                                const int64_t* gt_off, const int64_t* iou_off, int P, int64_t total_det, int64_t total_gt,
                                const float* iou, const float* iou_thrs, int num_thrs, const float* area_ranges,
                                int num_ranges, void* work, uint8_t* tp, uint8_t* fp, void* stream) {
  YV4_REQUIRE(mode == YV4_TPFP_DEFAULT || mode == YV4_TPFP_IMAGENET, "tpfp: mode must be YV4_TPFP_DEFAULT or _IMAGENET");
  YV4_REQUIRE(P > 0 && det_off && gt_off && iou_off, "tpfp: bad problem table");
  YV4_REQUIRE(total_det >= 0 && total_gt >= 0, "tpfp: negative box count");
  YV4_REQUIRE(total_det < 0x7f7f7f7f && total_gt < 0x7f7f7f7f, "tpfp: more than 2^31 boxes");
  YV4_REQUIRE(iou_thrs && num_thrs > 0, "tpfp: no IoU thresholds");
  YV4_REQUIRE(num_ranges > 0 && (area_ranges || num_ranges == 1), "tpfp: area_ranges may be null only with num_ranges == 1");
  if (total_det == 0) return YV4_OK;
  YV4_REQUIRE(det && work && tp && fp, "tpfp: null pointer");
  YV4_REQUIRE(mode != YV4_TPFP_DEFAULT || rank, "tpfp: the default rule needs rank");
  YV4_REQUIRE(total_gt == 0 || (gt && gt_ignore && iou), "tpfp: null ground-truth pointer");
  YV4_REQUIRE(mode != YV4_TPFP_IMAGENET || (order && (total_gt == 0 || gt_ratio)), "tpfp: the imagenet rule needs order and gt_ratio");
  YV4_REQUIRE((((uintptr_t)det | (uintptr_t)gt) & 15) == 0, "tpfp: boxes must be 16-byte aligned");
  YV4_REQUIRE(((uintptr_t)work & 3) == 0, "tpfp: work must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t D = total_det, G = total_gt;
  const int T = num_thrs;
  int32_t* winner = nullptr;
  int32_t* matched = nullptr;
  float* row_max = nullptr;
  int32_t* row_arg = nullptr;
  int32_t* det_prob = reinterpret_cast<int32_t*>(work);
  if (mode == YV4_TPFP_IMAGENET) {
    matched = det_prob + D;
    uint8_t* covered = reinterpret_cast<uint8_t*>(matched + (int64_t)T * D);
    const long long n = (long long)P * T;
    hipLaunchKernelGGL(tpfp_imagenet_walk_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, iou, det_off, gt_off,
                       iou_off, P, D, G, order, gt_ratio, iou_thrs, T, covered, matched, det_prob);
    YV4_CHECK_LAUNCH("tpfp imagenet walk");
  } else {
    winner = det_prob + D;
    row_max = reinterpret_cast<float*>(winner + (int64_t)T * G);
    row_arg = reinterpret_cast<int32_t*>(row_max + D);
    // every byte 0x7f: 0x7f7f7f7f, above any rank (total_det is checked against it)
    if (G > 0 && hipMemsetAsync(winner, 0x7f, sizeof(int32_t) * (size_t)T * (size_t)G, s) != hipSuccess) {
      set_error("tpfp: memset failed");
      return YV4_E_LAUNCH;
    }
    hipLaunchKernelGGL(tpfp_rowmax_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, iou, det_off, gt_off, iou_off,
                       P, D, G, rank, iou_thrs, T, row_max, row_arg, det_prob, winner);
    YV4_CHECK_LAUNCH("tpfp row maximum");
  }
  hipLaunchKernelGGL(tpfp_classify_kernel, dim3(map_blocks((long long)T * num_ranges * D, 256)), dim3(256), 0, s, det, gt,
                     gt_ignore, det_prob, gt_off, D, G, rank, iou_thrs, T, area_ranges, num_ranges,
                     mode == YV4_TPFP_IMAGENET ? 1 : 0, row_max, row_arg, winner, matched, tp, fp);
  YV4_CHECK_LAUNCH("tpfp classify");
  return YV4_OK;
}
