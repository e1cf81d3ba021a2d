// The LDS-DMA load and its buffer descriptor, shared by every kernel family that stages through LDS-DMA (the fp32 and
// 16-bit convolutions, the weight gradients).
#pragma once
#include "yv4_common.h"

namespace yv4 {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// One LDS-DMA wave-instruction: lane l's 16 bytes at (descriptor base + voff + soff) land at
// LDS byte address lds_addr + 16*l.  Issued through inline asm on purpose: hipcc would
// otherwise wait vmcnt(0) before the next ds_read of ANY LDS address (it cannot tell the two
// halves of the double buffer apart), exposing the whole memory latency every K step.  The
// kernel counts these loads itself: s_waitcnt vmcnt(0) + s_barrier before the slice is read.
__device__ __forceinline__ void lds_dma16(u32x4_t rsrc, unsigned lds_addr, unsigned voff, unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :
               : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");
}

__device__ __forceinline__ u32x4_t make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  u32x4_t v;
  v.x = __builtin_amdgcn_readfirstlane((unsigned)a);
  v.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
  v.z = __builtin_amdgcn_readfirstlane(bytes);
  v.w = 0x00020000u;
  return v;
}

// A buffer descriptor reaches a tensor through 32-bit byte offsets, the last 16 of which are the kernels' out-of-range
// offset (0xFFFFFFF0: reads deliver zeros): tensors below that many bytes.
static inline bool desc_addressable(long long bytes) { return bytes < 0xFFFFFFF0LL; }

}  // namespace yv4
