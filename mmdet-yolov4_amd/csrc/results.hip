// The flat result table of a test loop, built on the device: one call appends one batch's post-processing output
// (Plan.postprocess: dets (N, max_per_img, 5), labels (N, max_per_img), count (N)) in the order the reference's
// _det2json walks a result list (mmdet/datasets/coco.py:179-199): image, then class, then the row order NMS left --
// what flatten_results([bbox2result(dets[n, :k], labels[n, :k], C) for n]) yields on the host.
//
// One 256-thread workgroup per image.  The image's first row lands at base + (the counts of the kept images before it);
// inside the image a row's place is (rows with a smaller label) + (earlier rows with the same label): a stable counting
// sort by label without a sort -- k <= max_per_img labels sit in LDS and every thread walks them (a broadcast read, no
// bank conflict), k * k compares per image.  The place is a permutation of [0, k) whatever the label values are, so no
// write leaves the image's own range; every write is checked against `capacity` on top of that.
#include "yv4_common.h"

namespace yv4 {

constexpr int kResultsBlock = 256;

__global__ __launch_bounds__(kResultsBlock) void results_append_kernel(
    const float* __restrict__ dets, const int32_t* __restrict__ labels, const int32_t* __restrict__ count,
    const int64_t* __restrict__ img_index, int max_per_img, int64_t base, int64_t capacity, float* __restrict__ out_dets,
    int64_t* __restrict__ out_labels, int64_t* __restrict__ out_img) {
  __shared__ int32_t s_lab[YV4_RESULTS_MAX_PER_IMG];
  __shared__ long long s_sum[kResultsBlock];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t image = img_index[n];
  if (image < 0) return;                     // (uniform over the workgroup)
  // rows of the kept images before this one
  long long before = 0;
  for (int m = tid; m < n; m += kResultsBlock)
    if (img_index[m] >= 0) before += min(max(count[m], 0), max_per_img);
  s_sum[tid] = before;
  const int k = min(max(count[n], 0), max_per_img);
  const int32_t* lab = labels + (size_t)n * max_per_img;
  for (int i = tid; i < k; i += kResultsBlock) s_lab[i] = lab[i];
  __syncthreads();
  for (int step = kResultsBlock / 2; step > 0; step >>= 1) {
    if (tid < step) s_sum[tid] += s_sum[tid + step];
    __syncthreads();
  }
  const int64_t start = base + s_sum[0];
  const float* src = dets + (size_t)n * max_per_img * 5;
  for (int i = tid; i < k; i += kResultsBlock) {
    const int32_t li = s_lab[i];
    int place = 0;
    for (int j = 0; j < k; ++j) {
      const int32_t lj = s_lab[j];
      place += (lj < li || (lj == li && j < i)) ? 1 : 0;
    }
    const int64_t row = start + place;
    if (row >= capacity) continue;
#pragma unroll
    for (int c = 0; c < 5; ++c) out_dets[row * 5 + c] = src[i * 5 + c];
    out_labels[row] = li;
    out_img[row] = image;
  }
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_results_append(const float* dets, const int32_t* labels, const int32_t* count, const int64_t* img_index,
                                  int N, int max_per_img, int num_classes, int64_t base, int64_t capacity,
                                  float* out_dets, int64_t* out_labels, int64_t* out_img, void* stream) {
  YV4_REQUIRE(N >= 0, "results_append: negative batch size %d", N);
  YV4_REQUIRE(max_per_img > 0 && num_classes > 0, "results_append: max_per_img and num_classes must be positive");
  if (max_per_img > YV4_RESULTS_MAX_PER_IMG) {
    set_error("results_append: max_per_img %d exceeds YV4_RESULTS_MAX_PER_IMG (%d labels per image in LDS)", max_per_img,
              YV4_RESULTS_MAX_PER_IMG);
    return YV4_E_UNSUPPORTED;
  }
  YV4_REQUIRE(base >= 0 && capacity >= base, "results_append: need 0 <= base <= capacity");
  if (N == 0) return YV4_OK;
  YV4_REQUIRE(dets && labels && count && img_index && out_dets && out_labels && out_img, "results_append: null pointer");
  hipLaunchKernelGGL(results_append_kernel, dim3(N), dim3(kResultsBlock), 0, reinterpret_cast<hipStream_t>(stream), dets,
                     labels, count, img_index, max_per_img, base, capacity, out_dets, out_labels, out_img);
  YV4_CHECK_LAUNCH("results_append");
  return YV4_OK;
}
