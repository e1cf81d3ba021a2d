// COCO error analysis (the C75 / C50 / Loc / Sim / Oth breakdown after Hoiem): the matching of all of its COCOeval runs
// in one pass.  The base run and the two per-category runs on relabelled ground truths ("every annotation of the same
// supercategory / of any other category becomes category c, ignore = 1, iscrowd = 1") differ only in which ground truths
// of the image a detection of category c may be matched to, so one wave per (image, category) problem computes the
// float64 IoU block of the problem's detections against ALL ground truths of the image once and runs the A x (T + 2)
// greedy walks on it, one per lane.  yv4_coco_rank orders the detections before and yv4_coco_accumulate turns the flags
// into precision curves afterwards, both unchanged (csrc/coco_eval.hip).  Entry points (declared in include/yv4.h):
//   yv4_coco_error_need    the doubles of workspace the problems need whose block does not fit LDS (device, one read-back)
//   yv4_coco_error_match   the gt counts, the IoU blocks and the walks
// Every floating-point value is ONE IEEE float64 operation of the definition, in its order (compiled with
// -ffp-contract=off); sums are integers.  Bit-exact against the definition; two runs give identical bytes.
#include "eval_common.h"

namespace yv4 {
namespace {

constexpr int kCrLanes = 64;
// Two LDS classes, one launch each, so that the many small problems do not pay the occupancy of the few large ones:
// a workgroup is one wave, a CU holds 160 KiB, so 18 KB per workgroup leaves 8 of them per CU and 76 KB leaves 2.
// (Measured, DESIGN 28: a small class of 1 024 pairs, 15 workgroups per CU, is slower on 6 x 120 problems -- the
// problems it turns away run two to a CU.)
constexpr int kCrSmallIou = 2048, kCrSmallGt = 256;                                   // 16 KB + 2 KB
constexpr int kCrLargeIou = YV4_COCO_ERROR_LDS_PAIRS, kCrLargeGt = YV4_COCO_ERROR_LDS_GTS;   // 72 KB + 4 KB

// 0: small LDS class, 1: large LDS class, 2: workspace
__host__ __device__ __forceinline__ int cr_class(int64_t nd, int64_t ng) {
  const int64_t pairs = nd * ng;
  if (pairs <= kCrSmallIou && ng <= kCrSmallGt) return 0;
  if (pairs <= kCrLargeIou && ng <= kCrLargeGt) return 1;
  return 2;
}

// doubles of workspace a problem needs per lane group: the IoU block and 64 lanes' matched bits (0: both in LDS)
__host__ __device__ __forceinline__ int64_t cr_problem_need(int64_t nd, int64_t ng) {
  if (nd == 0 || ng == 0 || cr_class(nd, ng) != 2) return 0;
  return nd * ng + ((ng + 31) / 32) * 32;          // words * 64 lanes * 4 bytes = words * 32 doubles
}

__global__ __launch_bounds__(256) void cr_need_kernel(const int64_t* __restrict__ det_off,
                                                      const int64_t* __restrict__ gt_img_off, int P, int K, int max_det,
                                                      int groups, unsigned long long* __restrict__ need) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int64_t nd = det_off[p + 1] - det_off[p];
  if (nd > max_det) nd = max_det;
  const int img = p / K;
  const int64_t n = cr_problem_need(nd, gt_img_off[img + 1] - gt_img_off[img]);
  if (n) atomicAdd(need, (unsigned long long)(n * groups));
}

// gts that count in each area range, per category (integer atomics: the sum does not depend on the arrival order)
__global__ __launch_bounds__(256) void cr_counts_kernel(const double* __restrict__ gt_area,
                                                        const uint8_t* __restrict__ gt_flag,
                                                        const int32_t* __restrict__ gt_cat, int64_t G, int K,
                                                        const double* __restrict__ area_rng, int A,
                                                        int32_t* __restrict__ counts) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int32_t k = gt_cat[g];
  if (k < 0 || k >= K || (gt_flag[g] & 2)) return;
  const double ar = gt_area[g];
  for (int a = 0; a < A; ++a)
    if (!(ar < area_rng[2 * a] || ar > area_rng[2 * a + 1])) atomicAdd(&counts[k * A + a], 1);
}

// One wave per (problem, group of 64 walks); kClass 0 / 1 serve the problems of their LDS class, kClass 1 also those
// of the workspace.  Walk w = a * (T + 2) + t: t < T the base walk at thrs[t] over the gts of category k, t == T the
// "Sim" walk at conf_thr over those of k's supercategory group, t == T + 1 the "Oth" walk at conf_thr over all of them.
template <int kClass>
__global__ __launch_bounds__(kCrLanes) void cr_match_kernel(
    const float* __restrict__ det, const uint32_t* __restrict__ order, const int64_t* __restrict__ det_off,
    const double* __restrict__ gt_box, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flag,
    const int32_t* __restrict__ gt_cat, const int64_t* __restrict__ gt_img_off, const int32_t* __restrict__ cat_group,
    int K, int max_det, const double* __restrict__ thrs, int T, double conf_thr, const double* __restrict__ area_rng,
    int A, double* __restrict__ work, int64_t work_len, int64_t* __restrict__ state, uint8_t* __restrict__ flags) {
  constexpr int kIou = kClass == 0 ? kCrSmallIou : kCrLargeIou;
  constexpr int kGt = kClass == 0 ? kCrSmallGt : kCrLargeGt;
  __shared__ double s_iou[kIou];
  __shared__ uint32_t s_gtm[(kGt / 32) * kCrLanes];
  __shared__ int64_t s_base;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t d0 = det_off[p];
  int64_t nd = det_off[p + 1] - d0;
  if (nd == 0) return;
  if (nd > max_det) nd = max_det;                       // only the first maxDets[-1] in rank order take part
  const int img = p / K, k = p - img * K;
  const int64_t g0 = gt_img_off[img];
  const int64_t G = gt_img_off[img + 1] - g0;
  const int cls = G == 0 ? 0 : cr_class(nd, G);
  if ((kClass == 0) != (cls == 0)) return;
  const int TW = T + 2, AW = A * TW;

  const int64_t pairs = nd * G;
  const int64_t words = (G + 31) / 32;
  const int64_t need = cr_problem_need(nd, G);
  double* iou = s_iou;
  uint32_t* gtm = s_gtm;
  if (need) {
    if (lane == 0) s_base = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(&state[0]), (unsigned long long)need);
    __syncthreads();
    const int64_t base = s_base;
    if (base + need > work_len) {                       // never with a workspace of the size yv4_coco_error_need reported
      if (lane == 0) state[1] = 1;
      return;
    }
    iou = work + base;
    gtm = reinterpret_cast<uint32_t*>(iou + pairs);
  }
  const int Gi = (int)G, ndi = (int)nd;                 // both below 2^31: total_gt is, and max_det is an int
  for (int d = 0; d < ndi; ++d) {                       // (no division: a row at a time, the gts over the lanes)
    const float* b = det + 5 * (int64_t)order[d0 + d];
    const double dx = (double)b[0], dy = (double)b[1];
    const double dw = (double)b[2] - dx, dh = (double)b[3] - dy;
    double* row = iou + (int64_t)d * G;
    for (int g = lane; g < Gi; g += kCrLanes) {
      const double* q = gt_box + 4 * (g0 + g);
      const double gx = q[0], gy = q[1], gw = q[2], gh = q[3];
      double v = 0.0;
      const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
      if (w > 0.0) {
        const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        if (h > 0.0) {
          const double inter = w * h;
          const double da = dw * dh;
          // a gt of another category is relabelled as a crowd of k; one of k keeps its own crowd bit
          const bool crowd = gt_cat[g0 + g] != k || (gt_flag[g0 + g] & 1);
          const double uni = crowd ? da : (da + gw * gh) - inter;
          v = inter / uni;
        }
      }
      row[g] = v;
    }
  }
  for (int64_t i = lane; i < words * kCrLanes; i += kCrLanes) gtm[i] = 0u;
  __syncthreads();

  const int aw = blockIdx.y * kCrLanes + lane;
  if (aw >= AW) return;
  const int a = aw / TW, t = aw - a * TW;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(t < T ? thrs[t] : conf_thr, 1 - 1e-10);
  const int32_t grp = cat_group[k];
  for (int d = 0; d < ndi; ++d) {
    const double* row = iou + (int64_t)d * G;
    // The definition walks the gts in the stable order "not ignored first" and never gives a match to a counted gt up
    // for an ignored one: the best counted candidate wins if there is one, else the best ignored one, each found with
    // `best` starting at the threshold and equality passing (among equal IoUs the later gt wins).  One sweep keeps both.
    // A foreign gt is ignored and crowd in every area range, so it competes among k's own ignored gts, in annotation
    // order.  The tests of a candidate only ever skip it, so the cheapest and most selective one -- an IoU below the
    // threshold is below `best` in either class -- comes first and the gt's fields are read for the few that pass it.
    double best0 = thr, best1 = thr;
    int m0 = -1, m1 = -1;
    for (int g = 0; g < Gi; ++g) {
      const double v = row[g];
      if (v < thr) continue;
      const int32_t gc = gt_cat[g0 + g];
      const bool own = gc == k;
      if (!own) {
        if (t < T) continue;
        if (t == T && !(gc >= 0 && gc < K && cat_group[gc] == grp)) continue;
      }
      const uint8_t fl = gt_flag[g0 + g];
      const double ar = gt_area[g0 + g];
      const bool ig = !own || (fl & 2) || ar < lo || ar > hi;
      const bool crowd = !own || (fl & 1);
      if (((gtm[(g >> 5) * kCrLanes + lane] >> (g & 31)) & 1u) && !crowd) continue;   // taken, and not a crowd
      if (!ig) {
        if (v < best0) continue;
        best0 = v;
        m0 = g;
      } else if (m0 < 0) {
        if (v < best1) continue;
        best1 = v;
        m1 = g;
      }
    }
    const int m = m0 >= 0 ? m0 : m1;
    bool dig;
    if (m >= 0) {
      gtm[(m >> 5) * kCrLanes + lane] |= 1u << (m & 31);
      dig = m0 < 0;
    } else {
      const float* b = det + 5 * (int64_t)order[d0 + d];
      const double da = ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
      dig = da < lo || da > hi;
    }
    flags[(d0 + d) * AW + aw] = (uint8_t)((m >= 0 ? 1 : 0) | (dig ? 2 : 0));
  }
}

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" int yv4_coco_error_need(const int64_t* det_off, const int64_t* gt_img_off, int P, int K, int max_det,
                                   int num_walks, int64_t* need, void* stream) {
  YV4_REQUIRE(det_off && gt_img_off && need, "coco_error_need: null pointer");
  YV4_REQUIRE(P > 0 && K > 0 && P % K == 0, "coco_error_need: bad problem table");
  YV4_REQUIRE(max_det > 0 && num_walks > 0, "coco_error_need: maxDets[-1] and the number of walks must be positive");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(need, 0, sizeof(int64_t), s) != hipSuccess) {
    set_error("coco_error_need: memset failed");
    return YV4_E_LAUNCH;
  }
  hipLaunchKernelGGL(cr_need_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, det_off, gt_img_off, P, K, max_det,
                     (num_walks + kCrLanes - 1) / kCrLanes, reinterpret_cast<unsigned long long*>(need));
  YV4_CHECK_LAUNCH("coco_error_need");
  return YV4_OK;
}

extern "C" int yv4_coco_error_match(const float* det, const uint32_t* order, const int64_t* det_off, const double* gt_box,
                                    const double* gt_area, const uint8_t* gt_flag, const int32_t* gt_cat,
                                    const int64_t* gt_img_off, const int32_t* cat_group, int P, int K, int64_t total_det,
                                    int64_t total_gt, int max_det, const double* iou_thrs, int T, double conf_thr,
                                    const double* area_rng, int A, double* work, int64_t work_len, int64_t* state,
                                    uint8_t* flags, int32_t* counts, void* stream) {
  YV4_REQUIRE(P > 0 && K > 0 && P % K == 0 && det_off && gt_img_off && cat_group, "coco_error_match: bad problem table");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "coco_error_match: more than 2^31 detections");
  YV4_REQUIRE(total_gt >= 0 && total_gt < 0x7fffffff, "coco_error_match: more than 2^31 ground truths");
  YV4_REQUIRE(max_det > 0, "coco_error_match: maxDets[-1] must be positive");
  YV4_REQUIRE(iou_thrs && T > 0, "coco_error_match: no IoU thresholds");
  YV4_REQUIRE(area_rng && A > 0 && A <= kCrLanes, "coco_error_match: between 1 and 64 area ranges");
  // yv4_coco_accumulate takes T + 2 thresholds next: K * A * M * (T + 2) waves with M >= 1
  YV4_REQUIRE((int64_t)K * A * ((int64_t)T + 2) < 0x7fffffff, "coco_error_match: too many (k, a, t) combinations");
  YV4_REQUIRE(state && counts, "coco_error_match: null pointer");
  YV4_REQUIRE(total_det == 0 || (det && order && flags), "coco_error_match: null detection pointer");
  YV4_REQUIRE(total_gt == 0 || (gt_box && gt_area && gt_flag && gt_cat), "coco_error_match: null ground-truth pointer");
  YV4_REQUIRE(work_len >= 0 && (work_len == 0 || work), "coco_error_match: bad workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t AW = (size_t)A * ((size_t)T + 2);
  if (hipMemsetAsync(state, 0, 2 * sizeof(int64_t), s) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)K * A, s) != hipSuccess ||
      (total_det > 0 && hipMemsetAsync(flags, 0, (size_t)total_det * AW, s) != hipSuccess)) {
    set_error("coco_error_match: memset failed");
    return YV4_E_LAUNCH;
  }
  if (total_gt > 0)
    hipLaunchKernelGGL(cr_counts_kernel, dim3((unsigned)((total_gt + 255) / 256)), dim3(256), 0, s, gt_area, gt_flag, gt_cat,
                       total_gt, K, area_rng, A, counts);
  if (total_det > 0) {
    const dim3 grid((unsigned)P, (unsigned)((AW + kCrLanes - 1) / kCrLanes));
    hipLaunchKernelGGL(cr_match_kernel<0>, grid, dim3(kCrLanes), 0, s, det, order, det_off, gt_box, gt_area, gt_flag, gt_cat,
                       gt_img_off, cat_group, K, max_det, iou_thrs, T, conf_thr, area_rng, A, work, work_len, state, flags);
    hipLaunchKernelGGL(cr_match_kernel<1>, grid, dim3(kCrLanes), 0, s, det, order, det_off, gt_box, gt_area, gt_flag, gt_cat,
                       gt_img_off, cat_group, K, max_det, iou_thrs, T, conf_thr, area_rng, A, work, work_len, state, flags);
  }
  YV4_CHECK_LAUNCH("coco_error_match");
  return YV4_OK;
}
