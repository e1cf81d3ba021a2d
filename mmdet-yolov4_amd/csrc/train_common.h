// What the training-side translation units (conv_wgrad.hip, pack_weights.hip, elementwise_bwd.hip, bn_train.hip)
// share: element access for the three operand types, the dtype dispatch of the host entries and the grid of the
// element-wise kernels.
#pragma once
#include "yv4_common.h"

namespace yv4 {

// ---- element access for the three operand types (fp32, fp16, bf16): 4 consecutive channels ----
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
template <typename T> struct El;
template <> struct El<float> {
  static __device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
};
template <> struct El<_Float16> {
  static __device__ __forceinline__ float4 ld4(const _Float16* p) {
    const f16x4_t v = *reinterpret_cast<const f16x4_t*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
  static __device__ __forceinline__ void st4(_Float16* p, float4 v) {
    f16x4_t o;
    o[0] = (_Float16)v.x; o[1] = (_Float16)v.y; o[2] = (_Float16)v.z; o[3] = (_Float16)v.w;
    *reinterpret_cast<f16x4_t*>(p) = o;
  }
};
template <> struct El<__bf16> {
  static __device__ __forceinline__ float4 ld4(const __bf16* p) {
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
  static __device__ __forceinline__ void st4(__bf16* p, float4 v) {
    bf16x4_t o;
    o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4_t*>(p) = o;
  }
};

static inline unsigned ew_grid_t(size_t work_items) {
  size_t g = (work_items + 255) / 256;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (unsigned)g;
}

}  // namespace yv4

// dtype-dispatching bodies shared by the fp32 entries and their _h16 forms ------------------------
#define YV4_DISPATCH_T(dtype, CALL)                    \
  switch (dtype) {                                     \
    case YV4_F32: { typedef float T; CALL; } break;    \
    case YV4_F16: { typedef _Float16 T; CALL; } break; \
    default: { typedef __bf16 T; CALL; } break;        \
  }
