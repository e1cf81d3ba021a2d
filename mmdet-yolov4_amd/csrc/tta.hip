// Test-time augmentation of YOLOV3Head on gfx950: the part of BBoxTestMixin.aug_test_bboxes between the per-augmentation
// decode and the merged NMS.
//
// Reference code restated here:
//   slots    mmdet/models/dense_heads/yolo_head.py:254-311 with with_nms=False: per level conf.topk(nms_pre) (sorted,
//            descending objectness; ties to the lower anchor index, the rule of yv4_conf_topk_levels) when the level
//            has more than nms_pre boxes, else the level in anchor order; the levels concatenated
//   merge    mmdet/models/dense_heads/dense_test_mixins.py:10-36,84-100 (merge_aug_bboxes + multiclass_nms inputs),
//            mmdet/core/bbox/transforms.py:5-55 (bbox_flip, bbox_mapping_back),
//            mmdet/core/post_processing/bbox_nms.py:52-62 (cls > score_thr, then * score_factors)
// The NMS that follows is yv4_nms_images / yv4_nms_split, unchanged.
//
// Built with -ffp-contract=off: the flip subtraction, the division by scale_factor and cls * conf are separate fp32
// IEEE operations, as in the reference.
#include "nms_common.h"
#include "radix_sort.h"

namespace yv4 {

constexpr int kSlotThreads = 1024;
constexpr int kSlotCap = 8192;     // keys sorted in LDS (64 KB); larger top-k levels take the radix sort
constexpr int kMaxSlotLevels = 8;

struct SlotArgs {
  const float* conf;
  int64_t total;
  int num_levels;
  int n_l[kMaxSlotLevels];          // boxes of the level
  int k_l[kMaxSlotLevels];          // slots of the level
  int abase[kMaxSlotLevels];        // first anchor of the level inside an image
  int sbase[kMaxSlotLevels];        // first slot of the level inside an image
  const uint64_t* topk;             // (N * num_levels) admission keys
  int32_t* slots;
  int64_t S;
};

__device__ __forceinline__ uint64_t conf_key(float cf, int j) {
  return ((uint64_t)score_to_key(cf) << 32) | (uint32_t)j;
}

// one workgroup per (level, image)
__global__ __launch_bounds__(kSlotThreads) void topk_slots_kernel(SlotArgs p) {
  extern __shared__ uint64_t skeys[];
  __shared__ int scount;
  const int l = blockIdx.x, n = blockIdx.y;
  const int nl = p.n_l[l], k = p.k_l[l];
  int32_t* out = p.slots + (size_t)n * p.S + p.sbase[l];
  const int ab = p.abase[l];
  if (k == nl) {                                           // no top-k on this level: anchor order
    for (int i = threadIdx.x; i < nl; i += kSlotThreads) out[i] = ab + i;
    return;
  }
  if (k > kSlotCap) return;                                // the radix path (host side) owns this level
  const float* cf = p.conf + (size_t)n * p.total + ab;
  const uint64_t thr = p.topk[n * p.num_levels + l];
  if (threadIdx.x == 0) scount = 0;
  __syncthreads();
  // the admitted keys (exactly k of them: keys are distinct), in any order
  for (int i = threadIdx.x; i < nl; i += kSlotThreads) {
    const uint64_t key = conf_key(cf[i], ab + i);
    if (key <= thr) {
      const int pos = atomicAdd(&scount, 1);
      if (pos < kSlotCap) skeys[pos] = key;
    }
  }
  __syncthreads();
  const int cnt = min(scount, kSlotCap);
  int P = 1;
  while (P < cnt) P <<= 1;
  for (int i = cnt + threadIdx.x; i < P; i += kSlotThreads) skeys[i] = ~0ull;
  __syncthreads();
  // bitonic sort, ascending key = descending objectness, then ascending anchor index
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < P; i += kSlotThreads) {
        const int j = i ^ stride;
        if (j > i) {
          const uint64_t a = skeys[i], b = skeys[j];
          const bool up = (i & size) == 0;
          if ((a > b) == up) { skeys[i] = b; skeys[j] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < k; i += kSlotThreads) out[i] = i < cnt ? (int32_t)(uint32_t)skeys[i] : ab;
}

// radix path: every key of one (image, level), sorted whole; the first k are the slots
__global__ __launch_bounds__(256) void level_keys_kernel(const float* __restrict__ cf, int ab, int nl,
                                                         uint64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nl) keys[i] = conf_key(cf[i], ab + i);
}

__global__ __launch_bounds__(256) void level_slots_kernel(const uint64_t* __restrict__ sorted, int k,
                                                          int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < k) out[i] = (int32_t)(uint32_t)sorted[i];
}

// ---------------------------------------------------------------------------------
// merge: a workgroup owns 64 consecutive merged slots of one image; thread t works on slot t/4 and classes t%4,
// t%4+4, ... (the decode kernel's split).  Candidates leave with one reservation on the image's counter per workgroup.
// ---------------------------------------------------------------------------------
constexpr int kMergeSlots = 64;

struct MergeArgs {
  yv4_tta_aug aug[YV4_TTA_MAX_AUGS];
  int64_t mbase[YV4_TTA_MAX_AUGS + 1];   // first merged slot of each augmentation
  int num_augs, N, C;
  float score_thr;
  const float* meta;
  float* boxes_out;
  uint64_t* keys;
  int64_t key_cap;
  int32_t* counts;
  float* max_coord;
};

__global__ __launch_bounds__(256) void tta_merge_kernel(MergeArgs p) {
  __shared__ int wg_count, wg_base;
  __shared__ float wg_max[4];
  const int n = blockIdx.y;
  const int64_t S_total = p.mbase[p.num_augs];
  const int part = threadIdx.x & 3;
  const int64_t m = (int64_t)blockIdx.x * kMergeSlots + (threadIdx.x >> 2);
  const bool live = m < S_total;
  if (threadIdx.x == 0) wg_count = 0;
  __syncthreads();
  int a = 0;
  while (a + 1 < p.num_augs && m >= p.mbase[a + 1]) ++a;
  const yv4_tta_aug& g = p.aug[a];
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, cf = 0.f;
  const float* cls = nullptr;
  if (live) {
    const int s = (int)(m - p.mbase[a]);
    const int j = g.slots[(size_t)n * g.S + s];
    const size_t gj = (size_t)n * g.total + j;
    const float4 b = reinterpret_cast<const float4*>(g.boxes)[gj];
    cf = g.conf[gj];
    cls = g.cls + gj * p.C;
    const float* mt = p.meta + ((size_t)a * p.N + n) * 6;
    const float h = mt[0], w = mt[1];
    // bbox_flip (transforms.py:20-32)
    x1 = b.x; y1 = b.y; x2 = b.z; y2 = b.w;
    if (g.flip & 1) { x1 = w - b.z; x2 = w - b.x; }
    if (g.flip & 2) { y1 = h - b.w; y2 = h - b.y; }
    // / scale_factor (transforms.py:52-54)
    x1 /= mt[2]; y1 /= mt[3]; x2 /= mt[4]; y2 /= mt[5];
    if (part == 0) reinterpret_cast<float4*>(p.boxes_out)[(size_t)n * S_total + m] = make_float4(x1, y1, x2, y2);
  }
  int mine = 0;
  if (live)
    for (int c = part; c < p.C; c += 4) mine += cls[c] > p.score_thr ? 1 : 0;
  int slot = mine ? atomicAdd(&wg_count, mine) : 0;
  __syncthreads();
  if (threadIdx.x == 0 && wg_count > 0) wg_base = atomicAdd(&p.counts[n], wg_count);
  __syncthreads();
  float mx = -__builtin_huge_valf();
  if (mine) {
    uint64_t* ikeys = p.keys + (size_t)n * p.key_cap;
    slot += wg_base;
    for (int c = part; c < p.C; c += 4) {
      const float sc = cls[c];
      if (sc > p.score_thr) {
        const float score = sc * cf;
        const uint32_t flat = (uint32_t)m * (uint32_t)p.C + (uint32_t)c;
        if (slot < p.key_cap) ikeys[slot] = ((uint64_t)score_to_key(score) << 32) | flat;
        ++slot;
      }
    }
    mx = fmaxf(fmaxf(x1, y1), fmaxf(x2, y2));
  }
  // boxes.max() over the passing candidates (mmcv batched_nms): one atomic per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) wg_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = fmaxf(fmaxf(wg_max[0], wg_max[1]), fmaxf(wg_max[2], wg_max[3]));
    if (mx > -__builtin_huge_valf()) atomic_max_float(&p.max_coord[n], mx);
  }
}

// level geometry of yv4_topk_slots: k_l per level, total slots
static int64_t slot_layout(int num_levels, const int32_t* level_anchors, int nms_pre, int* k_l) {
  int64_t S = 0;
  for (int l = 0; l < num_levels; ++l) {
    const int nl = level_anchors[l];
    k_l[l] = (nms_pre > 0 && nl > nms_pre) ? nms_pre : nl;
    S += k_l[l];
  }
  return S;
}

// the radix path's workspace: the keys of one (image, level), the sort's two sides and its counters
struct RadixWork {
  size_t keys, kx, ky, hist, total;
  explicit RadixWork(int64_t n) {
    Carve c;
    keys = c.take((size_t)n * 8);
    kx = c.take((size_t)n * 8);
    ky = c.take((size_t)n * 8);
    hist = c.take(rs_hist_bytes(n));
    total = c.off;
  }
};

}  // namespace yv4

using namespace yv4;

extern "C" size_t yv4_topk_slots_work(int num_levels, const int32_t* level_anchors, int nms_pre) {
  if (!level_anchors || num_levels <= 0 || num_levels > kMaxSlotLevels) return 0;
  int k_l[kMaxSlotLevels];
  slot_layout(num_levels, level_anchors, nms_pre, k_l);
  int64_t biggest = 0;
  for (int l = 0; l < num_levels; ++l)
    if (k_l[l] < level_anchors[l] && k_l[l] > kSlotCap && level_anchors[l] > biggest) biggest = level_anchors[l];
  return biggest ? RadixWork(biggest).total : 0;
}

extern "C" int yv4_topk_slots(const float* conf, int N, int64_t total_anchors, int num_levels,
                              const int32_t* level_anchors, int nms_pre, const uint64_t* topk_keys, void* work,
                              int32_t* slots, int64_t S, void* stream) {
  YV4_REQUIRE(conf && slots && level_anchors, "topk_slots: null pointer");
  YV4_REQUIRE(N > 0 && N <= 65535 && num_levels > 0 && num_levels <= kMaxSlotLevels, "topk_slots: bad N / num_levels");
  int64_t sum = 0;
  for (int l = 0; l < num_levels; ++l) {
    YV4_REQUIRE(level_anchors[l] > 0, "topk_slots: level %d has no boxes", l);
    sum += level_anchors[l];
  }
  YV4_REQUIRE(sum == total_anchors && total_anchors < (1LL << 31), "topk_slots: level sizes do not add up to total_anchors");
  SlotArgs p;
  const int64_t S_want = slot_layout(num_levels, level_anchors, nms_pre, p.k_l);
  YV4_REQUIRE(S == S_want, "topk_slots: S = %lld, the levels give %lld", (long long)S, (long long)S_want);
  bool cut = false, radix = false;
  int ab = 0, sb = 0;
  for (int l = 0; l < num_levels; ++l) {
    p.n_l[l] = level_anchors[l];
    p.abase[l] = ab; p.sbase[l] = sb;
    ab += p.n_l[l]; sb += p.k_l[l];
    if (p.k_l[l] < p.n_l[l]) {
      cut = true;
      if (p.k_l[l] > kSlotCap) radix = true;
    }
  }
  YV4_REQUIRE(!cut || topk_keys, "topk_slots: a level is cut to nms_pre: topk_keys are required");
  YV4_REQUIRE(!radix || work, "topk_slots: a level's top-k exceeds %d: work (yv4_topk_slots_work bytes) is required",
              kSlotCap);
  p.conf = conf; p.total = total_anchors; p.num_levels = num_levels; p.topk = topk_keys; p.slots = slots; p.S = S;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(topk_slots_kernel, dim3((unsigned)num_levels, (unsigned)N), dim3(kSlotThreads),
                     (size_t)kSlotCap * sizeof(uint64_t), s, p);
  YV4_CHECK_LAUNCH("topk_slots");
  if (radix) {
    for (int l = 0; l < num_levels; ++l) {
      const int nl = p.n_l[l], k = p.k_l[l];
      if (!(k < nl && k > kSlotCap)) continue;
      const RadixWork L(nl);
      char* w = reinterpret_cast<char*>(work);
      uint64_t* keys = reinterpret_cast<uint64_t*>(w + L.keys);
      uint64_t* kx = reinterpret_cast<uint64_t*>(w + L.kx);
      uint64_t* ky = reinterpret_cast<uint64_t*>(w + L.ky);
      uint32_t* hist = reinterpret_cast<uint32_t*>(w + L.hist);
      for (int n = 0; n < N; ++n) {
        hipLaunchKernelGGL(level_keys_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s,
                           conf + (size_t)n * total_anchors + p.abase[l], p.abase[l], nl, keys);
        if (int rc = rs_sort<uint64_t, int, false>(keys, kx, ky, nullptr, nullptr, nullptr, nl, 64, hist, s)) return rc;
        hipLaunchKernelGGL(level_slots_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, kx, k,
                           slots + (size_t)n * S + p.sbase[l]);
      }
    }
    YV4_CHECK_LAUNCH("topk_slots: radix path");
  }
  return YV4_OK;
}

extern "C" int yv4_tta_merge(const yv4_tta_aug* augs, int num_augs, int N, int num_classes, float score_thr,
                             const float* meta, float* boxes_out, uint64_t* keys, int64_t key_cap, int32_t* counts,
                             float* max_coord, void* stream) {
  YV4_REQUIRE(augs && meta && boxes_out && keys && counts && max_coord, "tta_merge: null pointer");
  YV4_REQUIRE(num_augs > 0 && num_augs <= YV4_TTA_MAX_AUGS, "tta_merge: num_augs = %d outside [1, %d]", num_augs,
              YV4_TTA_MAX_AUGS);
  YV4_REQUIRE(N > 0 && N <= 65535 && num_classes > 0 && key_cap > 0, "tta_merge: bad N / num_classes / key_cap");
  YV4_REQUIRE(((uintptr_t)boxes_out & 15) == 0, "tta_merge: boxes_out must be 16-byte aligned");
  MergeArgs p;
  p.mbase[0] = 0;
  for (int a = 0; a < num_augs; ++a) {
    const yv4_tta_aug& g = augs[a];
    YV4_REQUIRE(g.boxes && g.conf && g.cls && g.slots, "tta_merge: null pointer in augmentation %d", a);
    YV4_REQUIRE(((uintptr_t)g.boxes & 15) == 0, "tta_merge: boxes of augmentation %d must be 16-byte aligned", a);
    YV4_REQUIRE(g.S > 0 && g.total > 0 && (int64_t)g.S <= g.total && g.total < (1LL << 31),
                "tta_merge: S / total out of range in augmentation %d", a);
    YV4_REQUIRE(g.flip >= YV4_FLIP_NONE && g.flip <= YV4_FLIP_DIAGONAL, "tta_merge: bad flip direction %d", g.flip);
    p.aug[a] = g;
    p.mbase[a + 1] = p.mbase[a] + g.S;
  }
  const int64_t S_total = p.mbase[num_augs];
  YV4_REQUIRE(S_total * (int64_t)num_classes <= (int64_t)UINT32_MAX,
              "tta_merge: %lld merged slots x %d classes exceed the 32-bit candidate index", (long long)S_total,
              num_classes);
  p.num_augs = num_augs; p.N = N; p.C = num_classes; p.score_thr = score_thr; p.meta = meta; p.boxes_out = boxes_out;
  p.keys = keys; p.key_cap = key_cap; p.counts = counts; p.max_coord = max_coord;
  hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((S_total + kMergeSlots - 1) / kMergeSlots), (unsigned)N),
                     dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  YV4_CHECK_LAUNCH("tta_merge");
  return YV4_OK;
}
