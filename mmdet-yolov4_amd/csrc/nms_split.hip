// mmcv batched_nms, n >= split_thr branch, for ONE image on gfx950:
//   for id in unique(idxs): keep |= nms(boxes_for_nms[idxs == id], scores[idxs == id])
//   keep = keep.nonzero();  keep = keep[scores[keep].argsort(descending=True)]
// (mmcv-full 1.3.x, third party; call site mmdet/core/post_processing/bbox_nms.py:84).
// Ties in the final argsort are broken by ascending candidate index (mmcv leaves them
// unspecified), the same rule as everywhere else in this library.
//
// Pipeline (all on the caller's stream, n is a host value):
//   1. radix sort of the 64-bit candidate keys (score desc, index asc)           [rs_* kernels below]
//   2. stable radix sort of those by class label -> class-major, order kept      [rs_* kernels below]
//   3. one workgroup per class: greedy NMS over its segment in chunks of 256, survivors
//      of earlier chunks kept as class-offset boxes in a global scratch list
//   4. survivors' keys (others = ~0) sorted again, the first max_out become detections
// Candidate decode, the class-offset box, the chunk mask and the bodies of the label / segment / emit kernels are
// nms_common.h's, the workspace layout's common part radix_sort.h's (soft_nms.hip's split path shares them).
// Built with -ffp-contract=off (see nms_common.h).
#include "nms_common.h"
#include "radix_sort.h"

namespace yv4 {

constexpr int kSplitThreads = 1024;

__global__ __launch_bounds__(256) void split_labels_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                           const int32_t* __restrict__ labels, int fused,
                                                           int32_t* __restrict__ out_labels) {
  key_labels_body(keys, n, labels, fused, out_labels);
}

// seg[c] = first sorted position with label >= c  (seg has num_classes + 1 entries)
__global__ __launch_bounds__(256) void split_segments_kernel(const int32_t* __restrict__ sorted_labels, int64_t n,
                                                             int num_classes, int64_t* __restrict__ seg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > num_classes) return;
  seg[c] = label_lower_bound(sorted_labels, n, c);
}

struct SplitArgs {
  const uint64_t* keys;      // class-major sorted candidate keys
  const int64_t* seg;        // num_classes + 1 segment bounds
  const float* boxes;
  int fused;
  float off_unit;            // max_coord + 1
  float iou_thr;
  int iou_form;
  float4* kept_box;          // scratch, n entries (class segment c uses [seg[c], ...))
  float* kept_area;          // scratch, n entries
  uint64_t* out_keys;        // n entries: key if kept else ~0
};

__global__ __launch_bounds__(kSplitThreads) void split_class_nms_kernel(SplitArgs p) {
  __shared__ float4 cbox[kNmsChunk];
  __shared__ float carea[kNmsChunk];
  __shared__ uint64_t cmask[kNmsChunk * 4];
  __shared__ uint64_t calive[4];
  __shared__ int kcount;
  const int cls = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t lo = p.seg[cls], hi = p.seg[cls + 1];
  const int64_t n = hi - lo;
  if (n <= 0) return;
  const uint64_t* keys = p.keys + lo;
  float4* kbox = p.kept_box + lo;
  float* karea = p.kept_area + lo;
  uint64_t* okeys = p.out_keys + lo;
  const float off = (float)cls * p.off_unit;
  if (tid == 0) kcount = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += kNmsChunk) {
    const int cn = (int)min((int64_t)kNmsChunk, n - c0);
    const int kept = kcount;
    if (tid < kNmsChunk) {
      float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
      float ar = 0.f;
      if (tid < cn) {
        // (the label is the segment's: only the box row is decoded)
        bb = offset_box(candidate_box(p.boxes, decode_candidate((uint32_t)keys[c0 + tid], p.fused, nullptr)), off);
        ar = (bb.z - bb.x) * (bb.w - bb.y);
      }
      cbox[tid] = bb;
      carea[tid] = ar;
    }
    __syncthreads();
    {  // (a) chunk vs survivors of earlier chunks (global scratch, written by this workgroup)
      const int i = tid & (kNmsChunk - 1);
      const int q = tid >> 8;
      bool dead = i >= cn;
      if (!dead) {
        const float4 bj = cbox[i];
        const float aj = carea[i];
        const volatile float4* vb = kbox;
        const volatile float* va = karea;
        for (int k = q; k < kept && !dead; k += 4) {
          float4 bk;
          bk.x = vb[k].x; bk.y = vb[k].y; bk.z = vb[k].z; bk.w = vb[k].w;
          dead = iou_gt(bk, va[k], bj, aj, p.iou_thr, p.iou_form);
        }
      }
      // combine the four quarters (as in nms_images_kernel; see nms_common.h for why it is not a shared function)
      const unsigned long long live = __ballot(!dead);
      if (q == 0 && (tid & 63) == 0) calive[tid >> 6] = live;
      __syncthreads();
      if (q != 0 && (tid & 63) == 0) atomicAnd(reinterpret_cast<unsigned long long*>(&calive[(tid & 255) >> 6]), live);
    }
    chunk_mask_row(cbox, carea, cn, tid, p.iou_thr, p.iou_form, 0, cmask);   // (b) chunk x chunk bitmask
    __syncthreads();
    if (tid == 0) {  // (c) greedy resolve
      uint64_t removed[4] = {0, 0, 0, 0};
      uint64_t keepbits[4] = {0, 0, 0, 0};
      int k = kept;
      for (int w = 0; w < 4; ++w) {
        uint64_t cur = calive[w] & ~removed[w];
        while (cur) {
          const int b = __builtin_ctzll(cur);
          const int i = w * 64 + b;
          kbox[k] = cbox[i];
          karea[k] = carea[i];
          ++k;
          keepbits[w] |= 1ull << b;
          removed[0] |= cmask[i * 4 + 0];
          removed[1] |= cmask[i * 4 + 1];
          removed[2] |= cmask[i * 4 + 2];
          removed[3] |= cmask[i * 4 + 3];
          const uint64_t above = b == 63 ? 0ull : (~0ull << (b + 1));
          cur = calive[w] & ~removed[w] & above;
        }
      }
      kcount = k;
      calive[0] = keepbits[0]; calive[1] = keepbits[1]; calive[2] = keepbits[2]; calive[3] = keepbits[3];
    }
    __threadfence_block();
    __syncthreads();
    if (tid < cn) okeys[c0 + tid] = ((calive[tid >> 6] >> (tid & 63)) & 1ull) ? keys[c0 + tid] : ~0ull;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void split_emit_kernel(const uint64_t* __restrict__ sorted_keys, int64_t n,
                                                         const float* __restrict__ boxes,
                                                         const int32_t* __restrict__ labels, int fused, int max_out,
                                                         float* out_dets, int32_t* out_labels, int64_t* out_index,
                                                         int32_t* out_count) {
  emit_body(sorted_keys, n, boxes, labels, fused, max_out, out_dets, out_labels, out_index, out_count);
}

// the common pieces, then the survivors of earlier chunks: class-offset box and area per candidate
struct SplitLayout : SplitSortLayout {
  size_t kbox, karea, total;
  explicit SplitLayout(int64_t n) : SplitSortLayout(n) {
    kbox = carve.take((size_t)n * 16);
    karea = carve.take((size_t)n * 4);
    total = carve.off;
  }
};

}  // namespace yv4

using namespace yv4;

extern "C" size_t yv4_nms_split_work(int64_t n) {
  if (n <= 0 || n >= (1LL << 31)) return 0;
  return SplitLayout(n).total;
}

extern "C" int yv4_nms_split(const uint64_t* keys, int64_t n, float max_coord, const float* boxes,
                             const int32_t* labels, int fused_classes, float iou_thr, int max_out, void* work,
                             float* out_dets, int32_t* out_labels, int64_t* out_index, int32_t* out_count,
                             void* stream) {
  YV4_REQUIRE(keys && boxes && work && out_dets && out_labels && out_index && out_count, "nms_split: null pointer");
  YV4_REQUIRE(n > 0 && n < (1LL << 31), "nms_split: n out of range");
  YV4_REQUIRE(max_out > 0 && fused_classes >= 0 && fused_classes <= kSplitMaxClasses, "nms_split: bad max_out / classes");
  YV4_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)work & 255) == 0, "nms_split: boxes must be 16-byte and work 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // labels are < 65536 (16 radix bits); with fused classes the class count is known, otherwise
  // the caller's labels are bounded by the same limit
  const int num_classes = fused_classes > 0 ? fused_classes : kSplitMaxClasses;
  const SplitLayout L(n);
  char* w = reinterpret_cast<char*>(work);
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(w + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(w + L.keys_b);
  int32_t* lab_a = reinterpret_cast<int32_t*>(w + L.lab_a);
  int32_t* lab_b = reinterpret_cast<int32_t*>(w + L.lab_b);
  int64_t* seg = reinterpret_cast<int64_t*>(w + L.seg);
  uint64_t* keys_t = reinterpret_cast<uint64_t*>(w + L.keys_t);
  uint32_t* lab_t = reinterpret_cast<uint32_t*>(w + L.lab_t);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + L.hist);
  const unsigned g = (unsigned)((n + 255) / 256);
  // 1. by (score desc, index asc)
  if (int rc = rs_sort<uint64_t, int, false>(keys, keys_a, keys_t, nullptr, nullptr, nullptr, n, 64, hist, s)) return rc;
  // 2. stable by label (labels are < 65536: two passes)
  hipLaunchKernelGGL(split_labels_kernel, dim3(g), dim3(256), 0, s, keys_a, n, labels, fused_classes, lab_a);
  if (int rc = rs_sort<uint32_t, uint64_t, true>(reinterpret_cast<const uint32_t*>(lab_a), reinterpret_cast<uint32_t*>(lab_b),
                                                 lab_t, keys_a, keys_b, keys_t, n, 16, hist, s))
    return rc;
  hipLaunchKernelGGL(split_segments_kernel, dim3((num_classes + 1 + 255) / 256), dim3(256), 0, s, lab_b, n, num_classes, seg);
  // 3. per-class NMS; survivors' keys into keys_a (others ~0)
  SplitArgs a;
  a.keys = keys_b; a.seg = seg; a.boxes = boxes; a.fused = fused_classes; a.off_unit = max_coord + 1.f;
  a.iou_thr = iou_thr; a.iou_form = nms_iou_form(); a.kept_box = reinterpret_cast<float4*>(w + L.kbox); a.kept_area = reinterpret_cast<float*>(w + L.karea);
  a.out_keys = keys_a;
  hipLaunchKernelGGL(split_class_nms_kernel, dim3(num_classes), dim3(kSplitThreads), 0, s, a);
  // 4. survivors by (score desc, index asc), first max_out
  if (int rc = rs_sort<uint64_t, int, false>(keys_a, keys_b, keys_t, nullptr, nullptr, nullptr, n, 64, hist, s)) return rc;
  const int lim = (int)(n < max_out ? n : max_out);
  hipLaunchKernelGGL(split_emit_kernel, dim3((lim + 255) / 256), dim3(256), 0, s, keys_b, n, boxes, labels, fused_classes,
                     max_out, out_dets, out_labels, out_index, out_count);
  YV4_CHECK_LAUNCH("nms_split");
  return YV4_OK;
}
