// Device helpers shared by the post-processing kernels (postproc.hip, nms_split.hip, soft_nms.hip, tta.hip,
// conf_topk.hip): the score keys, the suppression predicate, candidate key -> box row and label, the class-offset box,
// the chunk x chunk mask stage of the two hard-NMS kernels and the bodies of the split paths' label / segment / emit
// kernels (the __global__ wrappers stay in their translation units).
// Translation units including this header must be built with -ffp-contract=off.
#pragma once
#include "yv4_common.h"

namespace yv4 {

// ---- order-preserving float <-> uint32 (descending score = ascending key) ---------
__device__ __forceinline__ uint32_t score_to_key(float s) {
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending order of floats
  return ~u;                                       // descending
}
__device__ __forceinline__ float key_to_score(uint32_t k) {
  uint32_t u = ~k;
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

// The suppression predicate, in the two forms mmcv-full 1.3.x ships (the reference's call site is
// core/post_processing/bbox_nms.py:84; mmcv itself is third party and absent):
//   form 0 (YV4_NMS_IOU_DIV, default)  inter / (Sa + Sb - inter) > thr     mmcv's CPU kernel (nms_cpu)
//   form 1 (YV4_NMS_IOU_MUL)           inter > thr * (Sa + Sb - inter)     mmcv's CUDA kernel (devIoU)
// They differ only where the fp32 rounding of the quotient / the product crosses thr (tests/golden/nms_boundary.npz
// holds such pairs).  `form` is uniform over the launch.
__device__ __forceinline__ bool iou_gt(const float4 bi, const float ai, const float4 bj, const float aj, const float thr,
                                       const int form) {
  const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
  const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  // disjoint boxes (most pairs), division form: 0 / uni is +-0 or NaN, none of which is > thr >= 0 -- the same answer
  // without the division.  (The product form keeps its expression: thr * uni is negative for a malformed box.)
  if (!form && !(inter > 0.f) && thr >= 0.f) return false;
  const float uni = ai + aj - inter;
  if (form) return inter > thr * uni;
  const float ovr = inter / uni;
  return ovr > thr;
}

int nms_iou_form();   // api.hip: the process-wide form set by yv4_nms_set_iou_form

__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
  // valid for any mix of signs when *addr starts at -inf
  if (v >= 0.f)
    atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else
    atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// ---- candidate keys: (score key << 32) | flat ----------------------------------------------------------------------
// flat = box row * fused + label when the caller fuses `fused` classes into the index (the heads' score matrix), else
// flat is the box row itself and its label comes from `labels` (NULL: one class, label 0).
struct Candidate {
  uint32_t row;
  int label;
};
__device__ __forceinline__ Candidate decode_candidate(const uint32_t flat, const int fused, const int32_t* labels) {
  Candidate c;
  if (fused > 0) {
    c.row = flat / (uint32_t)fused;
    c.label = (int)(flat - c.row * (uint32_t)fused);
  } else {
    c.row = flat;
    c.label = labels ? labels[flat] : 0;
  }
  return c;
}
__device__ __forceinline__ float4 candidate_box(const float* boxes, const Candidate c) {
  return reinterpret_cast<const float4*>(boxes)[c.row];
}
// mmcv batched_nms' boxes_for_nms: boxes + idxs.to(boxes) * (max_coordinate + 1); off = label * (max + 1)
__device__ __forceinline__ float4 offset_box(const float4 ob, const float off) {
  return make_float4(ob.x + off, ob.y + off, ob.z + off, ob.w + off);
}

// ---- nms_images_kernel and split_class_nms_kernel: 1024 threads walk the sorted candidates in chunks of kNmsChunk -----
// (The four-quarter ballot / atomicAnd combine of their stage (a) is spelled out in both kernels: as a function of this
// header the address of its ds_and_b64 is computed ahead of the branch, and neither kernel keeps its instructions.)
constexpr int kNmsChunk = 256;

// chunk x chunk suppression bitmask: thread -> (row i = tid >> 2, word w = tid & 3); bit jj of the word: candidate i
// suppresses the later candidate j = 64 w + jj.  `ablate`: the measurement build's YV4_NMS_ABLATE word (bit 4: no mask).
__device__ __forceinline__ void chunk_mask_row(const float4* cbox, const float* carea, const int cn, const int tid,
                                               const float iou_thr, const int iou_form, const int ablate,
                                               uint64_t* cmask) {
  const int i = tid >> 2;
  const int w = tid & 3;
  uint64_t bits = 0;
  if (i < cn) {
    const float4 bi = cbox[i];
    const float ai = carea[i];
    const int j0 = w * 64;
    for (int jj = 0; jj < 64 && !YV4_ABLATE(ablate, 4); ++jj) {
      const int j = j0 + jj;
      if (j > i && j < cn && iou_gt(bi, ai, cbox[j], carea[j], iou_thr, iou_form)) bits |= 1ull << jj;
    }
  }
  cmask[i * 4 + w] = bits;
}

// ---- bodies of the split paths' small kernels (nms_split.hip, soft_nms.hip) ------------------------------------------
// out_labels[i] = label of keys[i], one thread per key
__device__ __forceinline__ void key_labels_body(const uint64_t* __restrict__ keys, const int64_t n,
                                                const int32_t* __restrict__ labels, const int fused,
                                                int32_t* __restrict__ out_labels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out_labels[i] = decode_candidate((uint32_t)keys[i], fused, labels).label;
}

// first sorted position with label >= c
__device__ __forceinline__ int64_t label_lower_bound(const int32_t* __restrict__ sorted_labels, const int64_t n, const int c) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_labels[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// thread k < min(max_out, n): the detection row (box, score of the key's high word), label and candidate index of
// sorted_keys[k] unless it is ~0; thread 0: *out_count = number of valid keys among the first min(max_out, n) (valid
// keys sort first), by bisection
__device__ __forceinline__ void emit_body(const uint64_t* __restrict__ sorted_keys, const int64_t n,
                                          const float* __restrict__ boxes, const int32_t* __restrict__ labels,
                                          const int fused, const int max_out, float* out_dets, int32_t* out_labels,
                                          int64_t* out_index, int32_t* out_count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lim = (int)min((int64_t)max_out, n);
  if (k < lim) {
    const uint64_t key = sorted_keys[k];
    if (key != ~0ull) {
      const uint32_t flat = (uint32_t)key;
      const Candidate c = decode_candidate(flat, fused, labels);
      const float4 ob = candidate_box(boxes, c);
      out_dets[k * 5 + 0] = ob.x; out_dets[k * 5 + 1] = ob.y; out_dets[k * 5 + 2] = ob.z; out_dets[k * 5 + 3] = ob.w;
      out_dets[k * 5 + 4] = key_to_score((uint32_t)(key >> 32));
      out_labels[k] = c.label;
      out_index[k] = (int64_t)flat;
    }
  }
  if (k == 0) {
    int64_t lo = 0, hi = lim;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted_keys[mid] != ~0ull) lo = mid + 1; else hi = mid;
    }
    *out_count = (int32_t)lo;
  }
}

}  // namespace yv4
