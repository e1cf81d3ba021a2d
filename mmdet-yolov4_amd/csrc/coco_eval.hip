// COCO bbox evaluation (COCOeval, iouType='bbox', useCats=1): evaluate and accumulate on the device.
//   pycocotools/cocoeval.py  computeIoU / evaluateImg / accumulate, _mask.pyx iou -> maskApi.c bbIou
// as mmdet/datasets/coco.py:547-551 configures it.  Three entry points (declared in include/yv4.h):
//   yv4_coco_rank        stable sort of the flat detection table by (problem, descending score): the rank of every
//                        detection inside its (image, category) problem, and the problems' offset table
//   yv4_coco_match       one wave per problem: the float64 IoU block once, then the A x T greedy walks on A x T lanes
//   yv4_coco_accumulate  stable sort by (category, descending score) from the (image-major, rank) order, then per
//                        (k, a, m, t) the cumulative tp / fp, precision envelope and the recall-threshold sampling
// Every floating-point value is ONE IEEE float64 operation of the definition, in its order (compiled with
// -ffp-contract=off); sums are integers.  Bit-exact against the definition; two runs give identical bytes.
// The score key, the offsets kernel and the sorts' sizing are eval_common.h's; ce_scan_kernel's one-wave backward walk
// is its own.
#include "eval_common.h"

namespace yv4 {
namespace {

constexpr int kCeLanes = 64;
constexpr int kCeIouLds = 2048;      // a problem's IoU block sits in LDS up to this many doubles
constexpr int kCeGtLds = 512;        // ... when its gts' matched bits do too (one bit per gt and lane)
constexpr int kCeMaxRec = 256;       // recall thresholds held in LDS
constexpr int kCeMaxM = 16;          // maxDets entries (passed by value)

// doubles of workspace a problem needs per (a, t) lane group: the IoU block and 64 lanes' matched bits (0: both in LDS)
__host__ __device__ __forceinline__ int64_t ce_problem_need(int64_t nd, int64_t ng) {
  const int64_t pairs = nd * ng;
  if (nd == 0 || (pairs <= kCeIouLds && ng <= kCeGtLds)) return 0;
  return pairs + ((ng + 31) / 32) * 32;          // words * 64 lanes * 4 bytes = words * 32 doubles
}

// ---- ordering ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_keys1_kernel(const float* __restrict__ det, const int32_t* __restrict__ prob,
                                                       int64_t D, int P, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const int32_t p = prob[d];
  const uint32_t pp = (p < 0 || p >= P) ? (uint32_t)P : (uint32_t)p;       // outside every problem: sorted to the end
  keys[d] = ((uint64_t)pp << 32) | desc_key(det[5 * d + 4]);
  vals[d] = (uint32_t)d;
}

__global__ __launch_bounds__(256) void ce_sprob_kernel(const uint64_t* __restrict__ keys, int64_t D,
                                                       int32_t* __restrict__ sprob) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < D) sprob[s] = (int32_t)(keys[s] >> 32);
}

__global__ __launch_bounds__(256) void ce_need_kernel(const int64_t* __restrict__ det_off,
                                                      const int64_t* __restrict__ gt_off, int P, int max_det, int groups,
                                                      unsigned long long* __restrict__ need) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int64_t nd = det_off[p + 1] - det_off[p];
  if (nd > max_det) nd = max_det;
  const int64_t n = ce_problem_need(nd, gt_off[p + 1] - gt_off[p]);
  if (n) atomicAdd(need, (unsigned long long)(n * groups));
}

// ---- matching: one wave per (problem, group of 64 (a, t) walks) ----------------------------------------------------
__global__ __launch_bounds__(kCeLanes) void ce_match_kernel(
    const float* __restrict__ det, const uint32_t* __restrict__ order, const int64_t* __restrict__ det_off,
    const double* __restrict__ gt_box, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flag,
    const int64_t* __restrict__ gt_off, int K, int max_det, const double* __restrict__ thrs, int T,
    const double* __restrict__ area_rng, int A, double* __restrict__ work, int64_t work_len, int64_t* __restrict__ state,
    uint8_t* __restrict__ flags, int32_t* __restrict__ counts) {
  __shared__ double s_iou[kCeIouLds];
  __shared__ uint32_t s_gtm[(kCeGtLds / 32) * kCeLanes];
  __shared__ int64_t s_base;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t d0 = det_off[p];
  int64_t nd = det_off[p + 1] - d0;
  if (nd > max_det) nd = max_det;                       // only the first maxDets[-1] in rank order take part
  const int64_t g0 = gt_off[p];
  const int64_t G = gt_off[p + 1] - g0;
  if (nd == 0 && G == 0) return;
  const int AT = A * T;

  // gts that count in each area range (integer atomics: the sum does not depend on the arrival order)
  if (blockIdx.y == 0 && lane < A && G > 0) {
    const double lo = area_rng[2 * lane], hi = area_rng[2 * lane + 1];
    int32_t c = 0;
    for (int64_t g = 0; g < G; ++g) {
      const double ar = gt_area[g0 + g];
      if (!((gt_flag[g0 + g] & 2) || ar < lo || ar > hi)) ++c;
    }
    if (c) atomicAdd(&counts[(p % K) * A + lane], c);
  }
  if (nd == 0) return;

  const int64_t pairs = nd * G;
  const int64_t words = (G + 31) / 32;
  const int64_t need = ce_problem_need(nd, G);
  double* iou = s_iou;
  uint32_t* gtm = s_gtm;
  if (need) {
    if (lane == 0) s_base = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(&state[0]), (unsigned long long)need);
    __syncthreads();
    const int64_t base = s_base;
    if (base + need > work_len) {                       // never with a workspace of the size yv4_coco_rank reported
      if (lane == 0) state[1] = 1;
      return;
    }
    iou = work + base;
    gtm = reinterpret_cast<uint32_t*>(iou + pairs);
  }
  for (int64_t i = lane; i < pairs; i += kCeLanes) {
    const int64_t d = i / G, g = i - d * G;
    const float* b = det + 5 * (int64_t)order[d0 + d];
    const double dx = (double)b[0], dy = (double)b[1];
    const double dw = (double)b[2] - dx, dh = (double)b[3] - dy;
    const double* q = gt_box + 4 * (g0 + g);
    const double gx = q[0], gy = q[1], gw = q[2], gh = q[3];
    double v = 0.0;
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    if (w > 0.0) {
      const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
      if (h > 0.0) {
        const double inter = w * h;
        const double da = dw * dh;
        const double uni = (gt_flag[g0 + g] & 1) ? da : (da + gw * gh) - inter;
        v = inter / uni;
      }
    }
    iou[i] = v;
  }
  for (int64_t i = lane; i < words * kCeLanes; i += kCeLanes) gtm[i] = 0u;
  __syncthreads();

  const int at = blockIdx.y * kCeLanes + lane;
  if (at >= AT) return;
  const int a = at / T, t = at - a * T;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(thrs[t], 1 - 1e-10);
  for (int64_t d = 0; d < nd; ++d) {
    const double* row = iou + d * G;
    double best = thr;
    int64_t m = -1;
    bool m_ig = false;
    // gts in the stable order "not ignored first": two passes.  The stop rule (a match to a counted gt is not given up
    // for an ignored one) is exactly "skip the second pass when the first found a match".
    for (int pass = 0; pass < 2 && m < 0; ++pass) {
      for (int64_t g = 0; g < G; ++g) {
        const uint8_t fl = gt_flag[g0 + g];
        const double ar = gt_area[g0 + g];
        const bool ig = (fl & 2) || ar < lo || ar > hi;
        if (ig != (pass == 1)) continue;
        if (((gtm[(g >> 5) * kCeLanes + lane] >> (g & 31)) & 1u) && !(fl & 1)) continue;   // taken, and not a crowd
        const double v = row[g];
        if (v < best) continue;
        best = v;                                          // equality passes: among equal IoUs the later gt wins
        m = g;
        m_ig = ig;
      }
    }
    bool dig;
    if (m >= 0) {
      gtm[(m >> 5) * kCeLanes + lane] |= 1u << (m & 31);
      dig = m_ig;
    } else {
      const float* b = det + 5 * (int64_t)order[d0 + d];
      const double da = ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
      dig = da < lo || da > hi;
    }
    flags[(d0 + d) * AT + at] = (uint8_t)((m >= 0 ? 1 : 0) | (dig ? 2 : 0));
  }
}

// ---- accumulation ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_keys2_kernel(const float* __restrict__ det, const uint32_t* __restrict__ order,
                                                       const int32_t* __restrict__ sprob,
                                                       const int64_t* __restrict__ det_off, int64_t D, int P, int K,
                                                       int max_det, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= D) return;
  const int32_t p = sprob[s];
  uint64_t key = (uint64_t)(uint32_t)K << 32;             // cut by maxDets[-1] or outside every problem: to the end
  if (p < P && s - det_off[p] < max_det)
    key = ((uint64_t)(uint32_t)(p % K) << 32) | desc_key(det[5 * (int64_t)order[s] + 4]);
  keys[s] = key;
  vals[s] = (uint32_t)s;
}

// the category-ordered detections as dense columns: rank, score, and the flags transposed to [at][j]
__global__ __launch_bounds__(256) void ce_gather_kernel(const float* __restrict__ det, const uint32_t* __restrict__ order,
                                                        const int32_t* __restrict__ sprob,
                                                        const int64_t* __restrict__ det_off,
                                                        const uint8_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ vals,
                                                        const int64_t* __restrict__ cat_off, int K, int64_t D, int AT,
                                                        int32_t* __restrict__ rank2, float* __restrict__ score2,
                                                        uint8_t* __restrict__ flags2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cat_off[K]) return;
  const int64_t s = vals[j];
  rank2[j] = (int32_t)(s - det_off[sprob[s]]);
  score2[j] = det[5 * (int64_t)order[s] + 4];
  for (int at = 0; at < AT; ++at) flags2[(int64_t)at * D + j] = flags[s * AT + at];
}

__global__ __launch_bounds__(256) void ce_fill_kernel(double* __restrict__ x, int64_t n, double v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = v;
}

struct CeMaxDets { int32_t v[kCeMaxM]; };

__device__ __forceinline__ int ce_count_le(const double* rec, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per (k, a, m, t).  The category's detections with rank < maxDets[m] form the list; the wave walks it in
// chunks of 64, forwards for the totals and backwards for everything else: the inclusive counts of a lane are the
// chunk's end count minus the set bits above it (ballots: integers), pr's suffix maximum is carried from chunk to chunk,
// and position i is np.searchsorted(rc, recThrs, 'left')'s answer for exactly the thresholds in (rc[i-1], rc[i]]
// ((-inf, rc[0]] for i = 0), which only a true positive or the first position can make non-empty.
__global__ __launch_bounds__(kCeLanes) void ce_scan_kernel(const int32_t* __restrict__ rank2, const float* __restrict__ score2,
                                                           const uint8_t* __restrict__ flags2,
                                                           const int64_t* __restrict__ cat_off,
                                                           const int32_t* __restrict__ counts, CeMaxDets max_dets,
                                                           int64_t D, int K, int A,
                                                           int M, int T, const double* __restrict__ rec_thrs, int R,
                                                           double* __restrict__ precision, double* __restrict__ recall,
                                                           double* __restrict__ scores) {
  __shared__ double s_rec[kCeMaxRec];
  const int lane = threadIdx.x;
  int id = blockIdx.x;
  const int t = id % T; id /= T;
  const int m = id % M; id /= M;
  const int a = id % A;
  const int k = id / A;
  const int32_t npig_i = counts[k * A + a];
  if (npig_i == 0) return;                                // the (k, a, m) entries stay -1
  for (int r = lane; r < R; r += kCeLanes) s_rec[r] = rec_thrs[r];
  const int64_t base = cat_off[k];
  const int64_t n = cat_off[k + 1] - base;
  const int md = max_dets.v[m];
  const int at = a * T + t;
  const uint8_t* fl = flags2 + (int64_t)at * D + base;
  const int32_t* rk = rank2 + base;
  const int64_t out_stride = (int64_t)K * A * M;
  const int64_t out0 = ((int64_t)k * A + a) * M + m;     // + (t * R + r) * out_stride
  for (int r = lane; r < R; r += kCeLanes) {
    precision[((int64_t)t * R + r) * out_stride + out0] = 0.0;
    scores[((int64_t)t * R + r) * out_stride + out0] = 0.0;
  }
  __syncthreads();
  const int64_t nchunks = (n + kCeLanes - 1) / kCeLanes;
  int64_t tp_end = 0, fp_end = 0, in_end = 0;
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t pos = c * kCeLanes + lane;
    const bool incl = pos < n && rk[pos] < md;
    const int f = incl ? (fl[pos] & 3) : 3;
    tp_end += __popcll(__ballot(incl && f == 1));
    fp_end += __popcll(__ballot(incl && f == 0));
    in_end += __popcll(__ballot(incl));
  }
  const double npig = (double)npig_i;
  if (lane == 0) recall[((int64_t)t * K + k) * A * M + a * M + m] = in_end ? (double)tp_end / npig : 0.0;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const unsigned long long le = lt | (1ull << lane);
  double carry = -1.0;                                    // below every precision
  for (int64_t c = nchunks - 1; c >= 0; --c) {
    const int64_t pos = c * kCeLanes + lane;
    const bool incl = pos < n && rk[pos] < md;
    const int f = incl ? (fl[pos] & 3) : 3;
    const bool tp = incl && f == 1, fp = incl && f == 0;
    const unsigned long long bt = __ballot(tp), bf = __ballot(fp), bi = __ballot(incl);
    const int64_t tpc = tp_end - __popcll(bt) + __popcll(bt & le);
    const int64_t fpc = fp_end - __popcll(bf) + __popcll(bf & le);
    const int64_t sub = in_end - __popcll(bi) + __popcll(bi & lt);       // position in the list
    double v = incl ? (double)tpc / (((double)fpc + (double)tpc) + 2.220446049250313e-16) : -1.0;
#pragma unroll
    for (int o = 1; o < kCeLanes; o <<= 1) {
      const double u = __shfl_down(v, o);
      if (lane + o < kCeLanes) v = fmax(v, u);
    }
    v = fmax(v, carry);
    carry = __shfl(v, 0);
    if (incl && (tp || sub == 0)) {
      const int hi = ce_count_le(s_rec, R, (double)tpc / npig);
      const int lo = sub == 0 ? 0 : ce_count_le(s_rec, R, (double)(tpc - 1) / npig);
      const double sc = (double)score2[base + pos];
      for (int r = lo; r < hi; ++r) {
        precision[((int64_t)t * R + r) * out_stride + out0] = v;
        scores[((int64_t)t * R + r) * out_stride + out0] = sc;
      }
    }
    tp_end -= __popcll(bt);
    fp_end -= __popcll(bf);
    in_end -= __popcll(bi);
  }
}

// the two workspaces, each read by its *_work function and its entry point
struct CeRankLayout {       // keys x2 | values | histogram
  size_t kx, ky, vy, hist;
  Carve carve;
  explicit CeRankLayout(int64_t D) {
    const size_t n = (size_t)D;
    kx = carve.take(8 * n), ky = carve.take(8 * n);
    vy = carve.take(4 * n);
    hist = carve.take(sort_hist_bytes(D));
  }
};

struct CeAccumLayout {      // keys x2 | values x2 | histogram | cat_off | rank2 | score2 | flags2
  size_t kx, ky, vx, vy, hist, cat_off, rank2, score2, flags2;
  Carve carve;
  CeAccumLayout(int64_t D, int K, int num_at) {
    const size_t n = (size_t)(D > 0 ? D : 1);
    kx = carve.take(8 * n), ky = carve.take(8 * n);
    vx = carve.take(4 * n), vy = carve.take(4 * n);
    hist = carve.take(sort_hist_bytes((int64_t)n));
    cat_off = carve.take(8 * ((size_t)K + 1));
    rank2 = carve.take(4 * n), score2 = carve.take(4 * n);
    flags2 = carve.take(n * (size_t)num_at);
  }
};

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" size_t yv4_coco_rank_work(int64_t total_det) {
  if (total_det <= 0) return 256;
  return CeRankLayout(total_det).carve.off;
}

extern "C" int yv4_coco_rank(const float* det, const int32_t* prob, int64_t total_det, int P, int max_det, int num_at,
                             const int64_t* gt_off, void* work, uint32_t* order, int32_t* sprob, int64_t* det_off,
                             int64_t* match_need, void* stream) {
  YV4_REQUIRE(P > 0 && gt_off && det_off && match_need, "coco_rank: bad problem table");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "coco_rank: more than 2^31 detections");
  YV4_REQUIRE(max_det > 0 && num_at > 0, "coco_rank: maxDets[-1] and the number of (area, threshold) walks must be positive");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(match_need, 0, sizeof(int64_t), s) != hipSuccess ||
      (total_det == 0 && hipMemsetAsync(det_off, 0, sizeof(int64_t) * ((size_t)P + 1), s) != hipSuccess)) {
    set_error("coco_rank: memset failed");
    return YV4_E_LAUNCH;
  }
  if (total_det == 0) return YV4_OK;
  YV4_REQUIRE(det && prob && work && order && sprob, "coco_rank: null pointer");
  YV4_REQUIRE(((uintptr_t)work & 7) == 0, "coco_rank: work must be 8-byte aligned");
  const int64_t D = total_det;
  const CeRankLayout L(D);
  char* w = reinterpret_cast<char*>(work);
  uint64_t* kx = reinterpret_cast<uint64_t*>(w + L.kx);
  uint64_t* ky = reinterpret_cast<uint64_t*>(w + L.ky);
  uint32_t* vy = reinterpret_cast<uint32_t*>(w + L.vy);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + L.hist);
  const unsigned blocks = (unsigned)((D + 255) / 256);
  hipLaunchKernelGGL(ce_keys1_kernel, dim3(blocks), dim3(256), 0, s, det, prob, D, P, kx, order);
  // the first pass only reads its input, so the keys / values are sorted "in place": the result lands in (kx, order)
  const int rc = rs_sort<uint64_t, uint32_t, true>(kx, kx, ky, order, order, vy, D, key_bits_hi32(P), hist, s, "coco_rank: radix sort");
  if (rc != YV4_OK) return rc;
  hipLaunchKernelGGL((offsets_kernel<uint64_t, 32>), dim3((unsigned)(P / 256 + 1)), dim3(256), 0, s, kx, D, P, det_off);
  hipLaunchKernelGGL(ce_sprob_kernel, dim3(blocks), dim3(256), 0, s, kx, D, sprob);
  hipLaunchKernelGGL(ce_need_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, det_off, gt_off, P, max_det,
                     (num_at + kCeLanes - 1) / kCeLanes, reinterpret_cast<unsigned long long*>(match_need));
  YV4_CHECK_LAUNCH("coco_rank");
  return YV4_OK;
}

extern "C" int yv4_coco_match(const float* det, const uint32_t* order, const int64_t* det_off, const double* gt_box,
                              const double* gt_area, const uint8_t* gt_flag, const int64_t* gt_off, int P, int K,
                              int64_t total_det, int max_det, const double* iou_thrs, int T, const double* area_rng, int A,
                              double* work, int64_t work_len, int64_t* state, uint8_t* flags, int32_t* counts,
                              void* stream) {
  YV4_REQUIRE(P > 0 && K > 0 && P % K == 0 && det_off && gt_off, "coco_match: bad problem table");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "coco_match: more than 2^31 detections");
  YV4_REQUIRE(max_det > 0, "coco_match: maxDets[-1] must be positive");
  YV4_REQUIRE(iou_thrs && T > 0, "coco_match: no IoU thresholds");
  YV4_REQUIRE(area_rng && A > 0 && A <= kCeLanes, "coco_match: between 1 and 64 area ranges");
  YV4_REQUIRE(state && counts, "coco_match: null pointer");
  YV4_REQUIRE(total_det == 0 || (det && order && flags), "coco_match: null detection pointer");
  YV4_REQUIRE(work_len >= 0 && (work_len == 0 || work), "coco_match: bad workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t AT = (size_t)A * (size_t)T;
  if (hipMemsetAsync(state, 0, 2 * sizeof(int64_t), s) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)K * A, s) != hipSuccess ||
      (total_det > 0 && hipMemsetAsync(flags, 0, (size_t)total_det * AT, s) != hipSuccess)) {
    set_error("coco_match: memset failed");
    return YV4_E_LAUNCH;
  }
  hipLaunchKernelGGL(ce_match_kernel, dim3((unsigned)P, (unsigned)((AT + kCeLanes - 1) / kCeLanes)), dim3(kCeLanes), 0, s,
                     det, order, det_off, gt_box, gt_area, gt_flag, gt_off, K, max_det, iou_thrs, T, area_rng, A, work,
                     work_len, state, flags, counts);
  YV4_CHECK_LAUNCH("coco_match");
  return YV4_OK;
}

extern "C" size_t yv4_coco_accumulate_work(int64_t total_det, int K, int num_at) {
  if (total_det < 0 || K <= 0 || num_at <= 0) return 0;
  return CeAccumLayout(total_det, K, num_at).carve.off;
}

extern "C" int yv4_coco_accumulate(const float* det, const uint32_t* order, const int32_t* sprob, const int64_t* det_off,
                                   const uint8_t* flags, const int32_t* counts, int P, int K, int64_t total_det,
                                   const int32_t* max_dets, int M, int T, int A, const double* rec_thrs, int R, void* work,
                                   double* precision, double* recall, double* scores, void* stream) {
  YV4_REQUIRE(P > 0 && K > 0 && P % K == 0 && K < 65535 && det_off && counts, "coco_accumulate: bad problem table");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7fffffff, "coco_accumulate: more than 2^31 detections");
  YV4_REQUIRE(max_dets && M > 0 && M <= kCeMaxM && T > 0 && A > 0, "coco_accumulate: between 1 and 16 maxDets; thresholds and area ranges must not be empty");
  CeMaxDets md;
  for (int i = 0; i < kCeMaxM; ++i) md.v[i] = i < M ? max_dets[i] : 0;
  const int max_last = md.v[M - 1];                       // maxDets[-1] cuts every list
  YV4_REQUIRE(max_last > 0, "coco_accumulate: maxDets[-1] must be positive");
  YV4_REQUIRE(rec_thrs && R > 0 && R <= kCeMaxRec, "coco_accumulate: between 1 and 256 recall thresholds");
  YV4_REQUIRE((int64_t)K * A * M * T < 0x7fffffff, "coco_accumulate: too many (k, a, m, t) combinations");
  YV4_REQUIRE(work && precision && recall && scores, "coco_accumulate: null pointer");
  YV4_REQUIRE(total_det == 0 || (det && order && sprob && flags), "coco_accumulate: null detection pointer");
  YV4_REQUIRE(((uintptr_t)work & 7) == 0, "coco_accumulate: work must be 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t D = total_det;
  const int64_t Dn = D > 0 ? D : 1;
  const int AT = A * T;
  const CeAccumLayout L(D, K, AT);
  char* w = reinterpret_cast<char*>(work);
  uint64_t* kx = reinterpret_cast<uint64_t*>(w + L.kx);
  uint64_t* ky = reinterpret_cast<uint64_t*>(w + L.ky);
  uint32_t* vx = reinterpret_cast<uint32_t*>(w + L.vx);
  uint32_t* vy = reinterpret_cast<uint32_t*>(w + L.vy);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + L.hist);
  int64_t* cat_off = reinterpret_cast<int64_t*>(w + L.cat_off);
  int32_t* rank2 = reinterpret_cast<int32_t*>(w + L.rank2);
  float* score2 = reinterpret_cast<float*>(w + L.score2);
  uint8_t* flags2 = reinterpret_cast<uint8_t*>(w + L.flags2);
  const int64_t n_pr = (int64_t)T * R * K * A * M, n_rc = (int64_t)T * K * A * M;
  hipLaunchKernelGGL(ce_fill_kernel, dim3((unsigned)((n_pr + 255) / 256 < 4096 ? (n_pr + 255) / 256 : 4096)), dim3(256), 0, s,
                     precision, n_pr, -1.0);
  hipLaunchKernelGGL(ce_fill_kernel, dim3((unsigned)((n_pr + 255) / 256 < 4096 ? (n_pr + 255) / 256 : 4096)), dim3(256), 0, s,
                     scores, n_pr, -1.0);
  hipLaunchKernelGGL(ce_fill_kernel, dim3((unsigned)((n_rc + 255) / 256 < 4096 ? (n_rc + 255) / 256 : 4096)), dim3(256), 0, s,
                     recall, n_rc, -1.0);
  if (D > 0) {
    const unsigned blocks = (unsigned)((D + 255) / 256);
    hipLaunchKernelGGL(ce_keys2_kernel, dim3(blocks), dim3(256), 0, s, det, order, sprob, det_off, D, P, K, max_last, kx, vx);
    const int rc = rs_sort<uint64_t, uint32_t, true>(kx, kx, ky, vx, vx, vy, D, 48, hist, s, "coco_accumulate: radix sort");
    if (rc != YV4_OK) return rc;
    hipLaunchKernelGGL((offsets_kernel<uint64_t, 32>), dim3((unsigned)(K / 256 + 1)), dim3(256), 0, s, kx, D, K, cat_off);
    hipLaunchKernelGGL(ce_gather_kernel, dim3(blocks), dim3(256), 0, s, det, order, sprob, det_off, flags, vx, cat_off, K, D,
                       AT, rank2, score2, flags2);
  } else if (hipMemsetAsync(cat_off, 0, sizeof(int64_t) * ((size_t)K + 1), s) != hipSuccess) {
    set_error("coco_accumulate: memset failed");
    return YV4_E_LAUNCH;
  }
  hipLaunchKernelGGL(ce_scan_kernel, dim3((unsigned)((int64_t)K * A * M * T)), dim3(kCeLanes), 0, s, rank2, score2, flags2,
                     cat_off, counts, md, Dn, K, A, M, T, rec_thrs, R, precision, recall, scores);
  YV4_CHECK_LAUNCH("coco_accumulate");
  return YV4_OK;
}
