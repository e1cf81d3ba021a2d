// Per-image mAP (include/yv4.h, "per-image mAP"): tools/analysis_tools/analyze_results.py's bbox_map_eval for every
// image of a dataset at once, behind yv4_map_rank, yv4_bbox_overlaps_batched and yv4_tpfp_batched.
//   yv4_map_image_ap    per problem p = class * N + image and threshold: the 'area' AP of yv4_map_accumulate over the
//                       problem's own detections, and the problem's regular gts
//   yv4_map_image_mean  per image and threshold numpy's float32 mean over the classes that have gts, then the float64
//                       average over the thresholds
// Thread map of the AP: two kernels share the problems by length, each in a grid-stride loop, the thresholds walked in
// turn.  A problem's list is short (about six detections on COCO, at most max_per_img), so
//   mi_ap_wave_kernel  takes the problems of up to 64 detections, ONE WAVE a problem, lane = position: the counts are
//                      ballots, the suffix maximum shuffles, the ordered sum a walk over the ballot of the steps -- no
//                      LDS, no barrier, no workspace; it also counts every problem's regular gts;
//   mi_ap_kernel       takes the longer ones, one workgroup of four waves a problem, thread = position inside a chunk
//                      of 256: the walk of map_flat.hip's accumulation on the three chunk primitives of eval_common.h.
//                      Walking the thresholds in turn lets one float per detection (the precision, then its suffix
//                      maximum) serve all of them: the workspace is 4 * Dv bytes.
// Both state the same rule (yv4.h) and write disjoint entries of ap.
// Every floating-point value is ONE IEEE operation of the definition (compiled with -ffp-contract=off); counts are
// integers; no float atomics: two runs give identical bytes.
#include <cfloat>

#include "eval_common.h"

namespace yv4 {
namespace {

constexpr int kMiMaxBlocks = 1 << 18;      // the grid of an AP kernel: its lanes stay far below 2^32
constexpr int kMiWaveMax = kEvalLanes;     // the longest problem the wave kernel takes
constexpr int kMiStack = 32;               // frames of the pairwise sum: 128 * 2^24 values and more never occur

// a problem's slice of an offset table of `total` elements, clamped to it (never needed with the tables yv4_map_rank
// and MapGt wrote)
__device__ __forceinline__ void mi_slice(const int64_t* __restrict__ off, int64_t p, int64_t total, int64_t& lo, int64_t& n) {
  lo = off[p];
  n = off[p + 1] - lo;
  if (lo < 0 || lo > total) { lo = 0; n = 0; }
  if (n > total - lo) n = total - lo;
  if (n < 0) n = 0;
}

// ---- problems of up to 64 detections: one wave a problem, lane = position; and every problem's regular gts ------------
__global__ __launch_bounds__(kEvalThreads) void mi_ap_wave_kernel(
    const uint8_t* __restrict__ tp, const uint8_t* __restrict__ fp, const int64_t* __restrict__ det_off,
    const int64_t* __restrict__ gt_off, const uint8_t* __restrict__ gt_ignore, int64_t D, int64_t G, int64_t P, int T,
    float* __restrict__ ap, int32_t* __restrict__ ngt) {
  const int lane = threadIdx.x & (kEvalLanes - 1);
  const unsigned long long le = ~0ull >> (63 - lane);     // lanes <= mine
  const int64_t waves = (int64_t)gridDim.x * kEvalWaves;
  // p, and with it every branch below that holds a ballot or a shuffle, is uniform over the wave
  for (int64_t p = (int64_t)blockIdx.x * kEvalWaves + (threadIdx.x >> 6); p < P; p += waves) {
    int64_t g0, gn;
    mi_slice(gt_off, p, G, g0, gn);
    int64_t ng = 0;
    for (int64_t lo = 0; lo < gn; lo += kEvalLanes) {
      const int64_t pos = lo + lane;
      ng += __popcll(__ballot(pos < gn && gt_ignore[g0 + pos] == 0));
    }
    if (lane == 0) ngt[p] = (int32_t)ng;
    int64_t base, n;
    mi_slice(det_off, p, D, base, n);
    if (n > kMiWaveMax) continue;                           // mi_ap_kernel's
    if (n == 0) {                                           // no curve: the AP is 0
      for (int t = lane; t < T; t += kEvalLanes) ap[(int64_t)t * P + p] = 0.f;
      continue;
    }
    const double den = ng >= 1 ? (double)ng : (double)FLT_EPSILON;        // np.maximum(int64 num_gts, float32 eps)
    const bool in = lane < n;
    for (int t = 0; t < T; ++t) {
      const int64_t col = (int64_t)t * D + base + lane;
      const bool ftp = in && tp[col] != 0, ffp = in && fp[col] != 0;
      const unsigned long long btp = __ballot(ftp), bfp = __ballot(ffp);
      const int ictp = __popcll(btp & le);
      const float ctp = (float)ictp, cfp = (float)__popcll(bfp & le);
      const float both = ctp + cfp;
      float sm = in ? ctp / (both >= FLT_EPSILON ? both : FLT_EPSILON) : 0.f;
#pragma unroll
      for (int o = 1; o < kEvalLanes; o <<= 1) {            // precision's suffix maximum (the pad mpre[n + 1] = 0 beyond n)
        const float u = __shfl_down(sm, o);
        if (lane + o < kEvalLanes) sm = fmaxf(sm, u);
      }
      const double r = (double)ctp / den;
      const double r_prev = lane == 0 ? 0.0 : (double)(float)(ictp - (ftp ? 1 : 0)) / den;     // mrec[0] = 0
      const bool step = in && r != r_prev;
      const double term = step ? (r - r_prev) * (double)sm : 0.0;
      double acc = 0.0;                                     // the single accumulator, identical in every lane
      for (unsigned long long m = __ballot(step); m; m &= m - 1) acc += __shfl(term, __ffsll(m) - 1);
      if (lane == 0) {
        const double r_last = (double)(float)__popcll(btp) / den;
        if (1.0 != r_last) acc += (1.0 - r_last) * 0.0;     // the closing step to mrec[n + 1] = 1 meets mpre[n + 1] = 0
        ap[(int64_t)t * P + p] = (float)acc;
      }
    }
  }
}

// ---- longer problems: one workgroup a problem on the chunk primitives --------------------------------------------------
__global__ __launch_bounds__(kEvalThreads) void mi_ap_kernel(
    const uint8_t* __restrict__ tp, const uint8_t* __restrict__ fp, const int64_t* __restrict__ det_off,
    const int64_t* __restrict__ gt_off, const uint8_t* __restrict__ gt_ignore, int64_t D, int64_t G, int64_t P, int T,
    float* __restrict__ scratch, float* __restrict__ ap) {
  __shared__ int s_ct[kEvalWaves], s_cf[kEvalWaves];
  __shared__ float s_wmax[kEvalWaves];
  __shared__ unsigned long long s_mask[kEvalWaves];
  __shared__ double s_term[kEvalThreads];
  const int tid = threadIdx.x;
  for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
    int64_t base, n;
    mi_slice(det_off, p, D, base, n);
    if (n <= kMiWaveMax) continue;                          // mi_ap_wave_kernel's (uniform over the workgroup)
    // ---- the problem's regular gts
    int64_t g0, gn;
    mi_slice(gt_off, p, G, g0, gn);
    int64_t ng = 0;
    for (int64_t lo = 0; lo < gn; lo += kEvalThreads) {
      const int64_t pos = lo + tid;
      const ChunkCount c = chunk_count(pos < gn && gt_ignore[g0 + pos] == 0, s_ct);
      ng += c.total;
      __syncthreads();
    }
    const double den = ng >= 1 ? (double)ng : (double)FLT_EPSILON;        // np.maximum(int64 num_gts, float32 eps)
    const int64_t nchunks = (n + kEvalThreads - 1) / kEvalThreads;
    float* mine = scratch + base;
    for (int t = 0; t < T; ++t) {
      const uint8_t* rtp = tp + (int64_t)t * D + base;
      const uint8_t* rfp = fp + (int64_t)t * D + base;
      // ---- A  forwards: inclusive integer counts -> precision
      int64_t run_tp = 0, run_fp = 0;
      for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int64_t pos = ch * kEvalThreads + tid;
        const bool in = pos < n;
        const bool ftp = in && rtp[pos] != 0, ffp = in && rfp[pos] != 0;
        ChunkCount ct, cf;
        chunk_count2(ftp, ffp, s_ct, s_cf, ct, cf);
        if (in) {
          const float ctp = (float)(run_tp + ct.incl);      // exact: below 2^24 (the host checks the classes' counts)
          const float cfp = (float)(run_fp + cf.incl);
          const float both = ctp + cfp;
          mine[pos] = ctp / (both >= FLT_EPSILON ? both : FLT_EPSILON);
        }
        run_tp += ct.total;
        run_fp += cf.total;
        __syncthreads();
      }
      const int64_t total_tp = run_tp;
      // ---- B  backwards: precision's suffix maximum (the pad mpre[n + 1] = 0 starts it); a thread reads and writes
      // only the positions it wrote in A
      float carry = 0.f;
      for (int64_t ch = nchunks - 1; ch >= 0; --ch) {
        const int64_t pos = ch * kEvalThreads + tid;
        const bool in = pos < n;
        const float v = chunk_suffix_max(in ? mine[pos] : 0.f, carry, s_wmax);
        if (in) mine[pos] = v;
        __syncthreads();
      }
      // ---- C  forwards: a term at every position where recall changes, in position order into one accumulator
      run_tp = 0;
      double acc = 0.0;
      for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int64_t pos = ch * kEvalThreads + tid;
        const bool in = pos < n;
        const bool ftp = in && rtp[pos] != 0;
        const ChunkCount ct = chunk_count(ftp, s_ct);
        const int64_t ctp = run_tp + ct.incl;
        const double r = (double)(float)ctp / den;
        const double r_prev = pos == 0 ? 0.0 : (double)(float)(ctp - (ftp ? 1 : 0)) / den;     // mrec[0] = 0
        const float sm = in ? mine[pos] : 0.f;
        const bool step = in && r != r_prev;
        chunk_ordered_sum(step ? (r - r_prev) * (double)sm : 0.0, step, acc, s_term, s_mask);
        run_tp += ct.total;
      }
      __syncthreads();
      if (tid == 0) {
        const double r_last = (double)(float)total_tp / den;
        if (1.0 != r_last) acc += (1.0 - r_last) * 0.0;     // the closing step to mrec[n + 1] = 1 meets mpre[n + 1] = 0
        ap[(int64_t)t * P + p] = (float)acc;
      }
    }
  }
}

// the APs of image i at one threshold, over the classes that have gts, in ascending class
struct MiValues {
  const float* ap;          // the threshold's row, at the image's column
  const int32_t* ngt;       // at the image's column
  int64_t N;
  int C, c;
  __device__ __forceinline__ float next() {
    while (c < C && ngt[(int64_t)c * N] <= 0) ++c;
    const float v = c < C ? ap[(int64_t)c * N] : 0.f;
    ++c;
    return v;
  }
};

// numpy's pairwise sum of n <= 128 values
__device__ float mi_leaf(MiValues& it, int n) {
  if (n < 8) {
    float res = 0.f;
    for (int k = 0; k < n; ++k) res += it.next();
    return res;
  }
  float r0 = it.next(), r1 = it.next(), r2 = it.next(), r3 = it.next();
  float r4 = it.next(), r5 = it.next(), r6 = it.next(), r7 = it.next();
  int k = 8;
  for (; k < n - n % 8; k += 8) {
    r0 += it.next(); r1 += it.next(); r2 += it.next(); r3 += it.next();
    r4 += it.next(); r5 += it.next(); r6 += it.next(); r7 += it.next();
  }
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; k < n; ++k) res += it.next();
  return res;
}

// numpy's pairwise sum of any n: the recursion on an explicit stack; the leaves take their values in order
__device__ float mi_pairwise(MiValues& it, int n) {
  if (n <= 128) return mi_leaf(it, n);
  int fn[kMiStack], stage[kMiStack];
  float left[kMiStack];
  int sp = 0;
  fn[0] = n; stage[0] = 0;
  float ret = 0.f;
  while (sp >= 0) {
    const int m = fn[sp];
    int n2 = m / 2;
    n2 -= n2 % 8;
    if (m <= 128) {
      ret = mi_leaf(it, m);
      --sp;
    } else if (stage[sp] == 0) {
      stage[sp] = 1;
      if (sp + 1 >= kMiStack) return ret;       // (unreachable: see kMiStack)
      ++sp; fn[sp] = n2; stage[sp] = 0;
    } else if (stage[sp] == 1) {
      left[sp] = ret;
      stage[sp] = 2;
      ++sp; fn[sp] = m - n2; stage[sp] = 0;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

// one lane per (threshold, image)
__global__ __launch_bounds__(256) void mi_mean_kernel(const float* __restrict__ ap, const int32_t* __restrict__ ngt, int N,
                                                      int C, int T, float* __restrict__ thr_mean) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)T * N) return;
  const int t = (int)(id / N), i = (int)(id % N);
  const int32_t* g = ngt + i;
  int n = 0;
  for (int c = 0; c < C; ++c) n += g[(int64_t)c * N] > 0 ? 1 : 0;
  float out = 0.f;
  if (n > 0) {
    MiValues it{ap + (int64_t)t * C * N + i, g, N, C, 0};
    out = mi_pairwise(it, n) / (float)n;
  }
  thr_mean[id] = out;
}

// one lane per image: sum(mean_aps) / len(mean_aps) on Python floats
__global__ __launch_bounds__(256) void mi_image_kernel(const float* __restrict__ thr_mean, int N, int T,
                                                       double* __restrict__ image_map) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double acc = 0.0;
  for (int t = 0; t < T; ++t) acc += (double)thr_mean[(int64_t)t * N + i];
  image_map[i] = acc / (double)T;
}

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" size_t yv4_map_image_ap_work(int64_t total_det) {
  if (total_det < 0) return 0;
  return 4 * (size_t)(total_det > 0 ? total_det : 1);
}

extern "C" int yv4_map_image_ap(const uint8_t* tp, const uint8_t* fp, int64_t tpfp_elems, const int64_t* det_off,
                                const int64_t* gt_off, int64_t off_elems, const uint8_t* gt_ignore, int64_t total_gt,
                                int64_t total_det, int N, int C, int num_thrs, void* work, size_t work_bytes, float* ap,
                                int64_t ap_elems, int32_t* ngt, int64_t ngt_elems, void* stream) {
  YV4_REQUIRE(N > 0 && C > 0 && (int64_t)N * C < 0x7fffffff, "map_image_ap: N x C problems must be positive and fit 31 bits");
  YV4_REQUIRE(num_thrs > 0 && (int64_t)num_thrs * N * C < ((int64_t)1 << 40), "map_image_ap: bad number of thresholds");
  YV4_REQUIRE(total_det >= 0 && total_det < 0x7f7f7f7f, "map_image_ap: more than 2^31 detections");
  YV4_REQUIRE(total_gt >= 0 && total_gt < 0x7f7f7f7f, "map_image_ap: more than 2^31 gts");
  const int64_t P = (int64_t)N * C;
  YV4_REQUIRE(det_off && gt_off && ap && ngt && work, "map_image_ap: null pointer");
  YV4_REQUIRE(total_det == 0 || (tp && fp), "map_image_ap: null tp / fp");
  YV4_REQUIRE(total_gt == 0 || gt_ignore, "map_image_ap: null gt_ignore");
  YV4_REQUIRE(tpfp_elems >= (int64_t)num_thrs * total_det, "map_image_ap: tp / fp hold %lld bytes, %d thresholds x %lld detections need %lld",
              (long long)tpfp_elems, num_thrs, (long long)total_det, (long long)((int64_t)num_thrs * total_det));
  YV4_REQUIRE(off_elems >= P + 1, "map_image_ap: det_off / gt_off hold %lld entries, %lld problems need %lld", (long long)off_elems,
              (long long)P, (long long)(P + 1));
  YV4_REQUIRE(ap_elems >= (int64_t)num_thrs * P, "map_image_ap: ap holds %lld values, %d thresholds x %lld problems need %lld",
              (long long)ap_elems, num_thrs, (long long)P, (long long)((int64_t)num_thrs * P));
  YV4_REQUIRE(ngt_elems >= P, "map_image_ap: ngt holds %lld values, %lld problems", (long long)ngt_elems, (long long)P);
  YV4_REQUIRE(work_bytes >= yv4_map_image_ap_work(total_det), "map_image_ap: work holds %zu bytes, %zu needed", work_bytes,
              yv4_map_image_ap_work(total_det));
  YV4_REQUIRE(((uintptr_t)work & 3) == 0, "map_image_ap: work must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t wave_blocks = (P + kEvalWaves - 1) / kEvalWaves;
  hipLaunchKernelGGL(mi_ap_wave_kernel, dim3((unsigned)(wave_blocks < kMiMaxBlocks ? wave_blocks : kMiMaxBlocks)),
                     dim3(kEvalThreads), 0, s, tp, fp, det_off, gt_off, gt_ignore, total_det, total_gt, P, num_thrs, ap, ngt);
  if (total_det > kMiWaveMax)                               // else no problem is longer than a wave
    hipLaunchKernelGGL(mi_ap_kernel, dim3((unsigned)(P < kMiMaxBlocks ? P : kMiMaxBlocks)), dim3(kEvalThreads), 0, s, tp, fp,
                       det_off, gt_off, gt_ignore, total_det, total_gt, P, num_thrs, reinterpret_cast<float*>(work), ap);
  YV4_CHECK_LAUNCH("map_image_ap");
  return YV4_OK;
}

extern "C" int yv4_map_image_mean(const float* ap, int64_t ap_elems, const int32_t* ngt, int64_t ngt_elems, int N, int C,
                                  int num_thrs, double* image_map, int64_t map_elems, float* image_map_thr,
                                  int64_t thr_elems, void* stream) {
  YV4_REQUIRE(N > 0 && C > 0 && (int64_t)N * C < 0x7fffffff, "map_image_mean: N x C problems must be positive and fit 31 bits");
  YV4_REQUIRE(num_thrs > 0 && (int64_t)num_thrs * N < ((int64_t)1 << 31), "map_image_mean: thresholds x images must be positive and fit 31 bits");
  YV4_REQUIRE(ap && ngt && image_map && image_map_thr, "map_image_mean: null pointer");
  const int64_t P = (int64_t)N * C;
  YV4_REQUIRE(ap_elems >= (int64_t)num_thrs * P, "map_image_mean: ap holds %lld values, %d thresholds x %lld problems need %lld",
              (long long)ap_elems, num_thrs, (long long)P, (long long)((int64_t)num_thrs * P));
  YV4_REQUIRE(ngt_elems >= P, "map_image_mean: ngt holds %lld values, %lld problems", (long long)ngt_elems, (long long)P);
  YV4_REQUIRE(map_elems >= N, "map_image_mean: image_map holds %lld values, %d images", (long long)map_elems, N);
  YV4_REQUIRE(thr_elems >= (int64_t)num_thrs * N, "map_image_mean: image_map_thr holds %lld values, %d thresholds x %d images",
              (long long)thr_elems, num_thrs, N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t lanes = (int64_t)num_thrs * N;
  hipLaunchKernelGGL(mi_mean_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, ap, ngt, N, C, num_thrs,
                     image_map_thr);
  hipLaunchKernelGGL(mi_image_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, image_map_thr, N, num_thrs, image_map);
  YV4_CHECK_LAUNCH("map_image_mean");
  return YV4_OK;
}
