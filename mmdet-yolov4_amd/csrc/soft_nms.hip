// Soft-NMS (mmcv-full 1.3.x softnms_cpu, restated in include/yv4.h and DESIGN 12) on gfx950.
//
// The loop is sequential: one step selects the first position of [i, nb) with the largest current score, swaps it to i,
// emits it, decays every other entry once and discards (end-swap compaction) the entries that fall below min_score.
// One workgroup runs one problem.  Entries never move in memory: each keeps its CURRENT ARRAY POSITION in a register
// (or in the global-memory form, a word of its own), and a step is
//   (1) a workgroup argmax over (score desc, position asc) keys -> the winner at position m;
//   (2) the winner's owner publishes its box; the entry at position i takes position m (the swap);
//   (3) every live entry decays; entries below min_score set their position's bit in an LDS bitmask;
//   (4)-(6) only when something was discarded: a prefix count over the bitmask words ranks the discarded positions from
//       the left and the surviving positions >= the new end from the right; the k-th survivor from the right takes the
//       k-th discarded position below the new end -- the literal loop's end swaps (tests/_soft_nms_ref.py checks the
//       rule against the loop).
// Images (yv4_soft_nms_images): candidates sorted into flat-index order in LDS, up to 20 per thread in registers.
// Split problems and large n (yv4_soft_nms_split): the same loop over entries in global memory (L2-resident scratch).
// The split path's label / segment / emit kernels wrap nms_common.h's bodies (nms_split.hip's grouping and output
// format); its workspace starts with radix_sort.h's SplitSortLayout.
// Built with -ffp-contract=off (see nms_common.h).
#include "nms_common.h"
#include "radix_sort.h"

namespace yv4 {
namespace {

constexpr int kSoftThreads = 1024;                           // split kernel (global-memory entries)
constexpr int kSoftWaves = kSoftThreads / 64;
constexpr int kImgThreads = 512;                             // images kernel: 2 waves per SIMD (217 VGPRs, no scratch)
constexpr int kSoftRegSlots = 20;                            // register entries per thread (images kernel)
constexpr int kSoftRegCap = kImgThreads * kSoftRegSlots;     // 10240 candidates of one image (>= mmcv split_thr 10000)
constexpr int kSoftPerThread = 8;                            // the images kernel sizes its active waves for 8 per thread
constexpr int kSoftMoveBatch = 8192;                         // hole positions per LDS batch of the compaction
constexpr int kSoftGlobalCap = 1 << 19;                      // largest problem (one label) of the global-memory form
constexpr int kDead = -1;                                    // position word of an emitted or discarded entry
constexpr int kFlag = 0x40000000;                            // position word of an entry discarded in this step

struct SoftParams {
  int method;
  float thr, sigma, min_score;
};

struct SoftShared {
  uint64_t red[kSoftWaves];
  float4 wbox;
  float wscore;
  int wslot;
  int dcount;
};

// mmcv softnms_cpu's weight (offset 0): IoU with the IEEE division, `>=` against the threshold, expf for gaussian
__device__ __forceinline__ float soft_decay(const float s, const float4 bi, const float ai, const float4 bj,
                                            const SoftParams& q) {
  const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
  const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float aj = (bj.z - bj.x) * (bj.w - bj.y);
  const float ovr = inter / (ai + aj - inter);
  float weight = 1.f;
  if (q.method == YV4_SOFT_NMS_NAIVE) {
    if (ovr >= q.thr) weight = 0.f;
  } else if (q.method == YV4_SOFT_NMS_LINEAR) {
    if (ovr >= q.thr) weight = 1.f - ovr;
  } else {
    weight = expf(-(ovr * ovr) / q.sigma);
  }
  return s * weight;
}

__device__ __forceinline__ uint64_t sel_key(float s, int pos) {
  return ((uint64_t)score_to_key(s) << 32) | (uint32_t)pos;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    v = u < v ? u : v;
  }
  return v;
}

// number of discarded positions below p (bits of positions < i are never set)
__device__ __forceinline__ int hole_rank(const uint64_t* bits, const int* wpre, int p) {
  const int w = p >> 6;
  return wpre[w] + __popcll(bits[w] & ((1ull << (p & 63)) - 1ull));
}

__device__ __forceinline__ void mark_hole(uint64_t* bits, int p) {
  atomicOr(reinterpret_cast<unsigned long long*>(&bits[p >> 6]), 1ull << (p & 63));
}

// ---- entries in registers: thread t holds slots t + k*Tn, k < kSoftRegSlots -----------------------------------------
struct RegStore {
  float4 b[kSoftRegSlots];
  float s[kSoftRegSlots];
  int pos[kSoftRegSlots];
  int tn;     // threads holding entries

  __device__ __forceinline__ uint64_t argmax() {
    uint64_t best = ~0ull;
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k)
      if ((unsigned)pos[k] < (unsigned)kFlag) {
        const uint64_t key = sel_key(s[k], pos[k]);
        best = key < best ? key : best;
      }
    return best;
  }
  __device__ __forceinline__ void take_winner(int m, SoftShared& sh) {
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k)
      if (pos[k] == m) {
        sh.wbox = b[k];
        sh.wscore = s[k];
        sh.wslot = (int)threadIdx.x + k * tn;
        pos[k] = kDead;
      }
  }
  __device__ __forceinline__ int decay(int i, int m, float4 wb, float wa, const SoftParams& q, uint64_t* bits) {
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k) {
      int p = pos[k];
      if (p < 0) continue;
      if (p == i) p = m;
      const float ns = soft_decay(s[k], wb, wa, b[k], q);
      s[k] = ns;
      if (ns < q.min_score) {
        mark_hole(bits, p);
        p |= kFlag;
        ++cnt;
      }
      pos[k] = p;
    }
    return cnt;
  }
  __device__ __forceinline__ void publish(int base, int nb2, const uint64_t* bits, const int* wpre, int* posA) {
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k) {
      const int p = pos[k];
      if (p >= kFlag) {
        const int q = p & (kFlag - 1);
        if (q < nb2) {
          const int a = hole_rank(bits, wpre, q) - base;
          if ((unsigned)a < (unsigned)kSoftMoveBatch) posA[a] = q;
        }
      }
    }
  }
  __device__ __forceinline__ void fill(int base, int nb, int nb2, int d, const uint64_t* bits, const int* wpre,
                                       const int* posA, bool last) {
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k) {
      const int p = pos[k];
      if (p >= kFlag) {
        if (last) pos[k] = kDead;
      } else if (p >= nb2) {
        const int bk = (nb - 1 - p) - (d - hole_rank(bits, wpre, p)) - base;
        if ((unsigned)bk < (unsigned)kSoftMoveBatch) pos[k] = posA[bk];
      }
    }
  }
};

// ---- entries in global memory (one problem of yv4_soft_nms_split): thread t owns slots lo + t + k*Tn ---------------
struct GlobalStore {
  float4* b;
  float* s;
  int* pos;
  int lo, n, tn;
  int kbest;  // the slot of this thread's argmax candidate

  __device__ __forceinline__ uint64_t argmax() {
    uint64_t best = ~0ull;
    kbest = -1;
    for (int j = (int)threadIdx.x; j < n; j += tn) {
      const int p = pos[lo + j];
      if ((unsigned)p < (unsigned)kFlag) {
        const uint64_t key = sel_key(s[lo + j], p);
        if (key < best) { best = key; kbest = j; }
      }
    }
    return best;
  }
  __device__ __forceinline__ void take_winner(int m, SoftShared& sh) {
    if (kbest >= 0 && pos[lo + kbest] == m) {
      sh.wbox = b[lo + kbest];
      sh.wscore = s[lo + kbest];
      sh.wslot = lo + kbest;
      pos[lo + kbest] = kDead;
    }
  }
  __device__ __forceinline__ int decay(int i, int m, float4 wb, float wa, const SoftParams& q, uint64_t* bits) {
    int cnt = 0;
    for (int j = (int)threadIdx.x; j < n; j += tn) {
      int p = pos[lo + j];
      if (p < 0) continue;
      if (p == i) p = m;
      const float ns = soft_decay(s[lo + j], wb, wa, b[lo + j], q);
      s[lo + j] = ns;
      if (ns < q.min_score) {
        mark_hole(bits, p);
        p |= kFlag;
        ++cnt;
      }
      pos[lo + j] = p;
    }
    return cnt;
  }
  __device__ __forceinline__ void publish(int base, int nb2, const uint64_t* bits, const int* wpre, int* posA) {
    for (int j = (int)threadIdx.x; j < n; j += tn) {
      const int p = pos[lo + j];
      if (p >= kFlag) {
        const int q = p & (kFlag - 1);
        if (q < nb2) {
          const int a = hole_rank(bits, wpre, q) - base;
          if ((unsigned)a < (unsigned)kSoftMoveBatch) posA[a] = q;
        }
      }
    }
  }
  __device__ __forceinline__ void fill(int base, int nb, int nb2, int d, const uint64_t* bits, const int* wpre,
                                       const int* posA, bool last) {
    for (int j = (int)threadIdx.x; j < n; j += tn) {
      const int p = pos[lo + j];
      if (p >= kFlag) {
        if (last) pos[lo + j] = kDead;
      } else if (p >= nb2) {
        const int bk = (nb - 1 - p) - (d - hole_rank(bits, wpre, p)) - base;
        if ((unsigned)bk < (unsigned)kSoftMoveBatch) pos[lo + j] = posA[bk];
      }
    }
  }
};

// The loop of one problem of n entries at positions 0 .. n-1.  Every thread of the workgroup calls it (barriers);
// threads >= st.tn hold no entries.  emit(r, slot, score) runs on thread 0 for the r-th selection.  Stops after max_out
// selections; with tie_ext it goes on while the winner's score equals the max_out-th one (the split path's re-sort breaks
// ties by index).  bits / wpre: nwords LDS words each; posA: kSoftMoveBatch LDS ints.  Returns the selection count.
template <class St, class Emit>
__device__ __forceinline__ int soft_loop(St& st, const int n, const int max_out, const bool tie_ext, const SoftParams q, SoftShared& sh,
                         uint64_t* bits, int* wpre, int* posA, const int nwords, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwa = (st.tn + 63) >> 6;
  for (int w = tid; w < nwords; w += blockDim.x) bits[w] = 0ull;
  int i = 0, nb = n, r = 0, clr0 = 0, clr1 = -1;
  float cut = 0.f;
  __syncthreads();
  while (i < nb && (tie_ext || r < max_out)) {
    // (1) argmax over (score desc, position asc)
    uint64_t best = wave_min_u64(st.argmax());
    if (lane == 0 && wave < nwa) sh.red[wave] = best;
    __syncthreads();
    uint64_t g = sh.red[0];
    for (int w = 1; w < nwa; ++w) {
      const uint64_t v = sh.red[w];
      g = v < g ? v : g;
    }
    const int m = (int)(uint32_t)g;
    const float gs = key_to_score((uint32_t)(g >> 32));
    if (r >= max_out && !(gs == cut)) break;                       // (tie_ext only: uniform)
    // (2) the winner leaves; the previous step's bitmask words are cleared
    for (int w = clr0 + tid; w <= clr1; w += blockDim.x) bits[w] = 0ull;
    if (tid == 0) sh.dcount = 0;
    st.take_winner(m, sh);
    __syncthreads();
    const float4 wb = sh.wbox;
    const float wa = (wb.z - wb.x) * (wb.w - wb.y);
    if (tid == 0) emit(r, sh.wslot, sh.wscore);
    if (r == max_out - 1) cut = gs;
    ++r;
    // (3) decay; the entry at position i takes the winner's position m
    const int mine = st.decay(i, m, wb, wa, q, bits);
    if (mine) atomicAdd(&sh.dcount, mine);
    __syncthreads();
    const int d = sh.dcount;
    const int i_old = i;
    ++i;
    clr0 = 0;
    clr1 = -1;
    if (d == 0) continue;
    // (4) prefix counts of the discarded positions, words [w0, w1]
    const int w0 = (i_old + 1) >> 6, w1 = (nb - 1) >> 6;
    if (wave == 0) {
      const int c = (w1 - w0 + 64) >> 6;
      const int a0 = min(w0 + lane * c, w1 + 1), a1 = min(a0 + c, w1 + 1);
      int sum = 0;
      for (int w = a0; w < a1; ++w) sum += __popcll(bits[w]);
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
      }
      int run = incl - sum;
      for (int w = a0; w < a1; ++w) {
        wpre[w] = run;
        run += __popcll(bits[w]);
      }
    }
    __syncthreads();
    // (5)-(6) the k-th survivor from the right at or above the new end takes the k-th hole from the left below it
    const int nb2 = nb - d;
    const int holes = hole_rank(bits, wpre, nb2);
    for (int base = 0;; base += kSoftMoveBatch) {
      st.publish(base, nb2, bits, wpre, posA);
      __syncthreads();
      const bool last = base + kSoftMoveBatch >= holes;
      st.fill(base, nb, nb2, d, bits, wpre, posA, last);
      __syncthreads();
      if (last) break;
    }
    nb = nb2;
    clr0 = w0;
    clr1 = w1;
  }
  return r;
}

// ---- images ---------------------------------------------------------------------------------------------------------
struct SoftImagesArgs {
  uint64_t* keys;
  int64_t key_cap;
  const int32_t* counts;
  const float* max_coord;
  const float* boxes;
  int64_t boxes_per_image;
  const int32_t* labels;
  int64_t label_stride;
  int fused_classes;
  SoftParams q;
  int max_out;
  int split_thr;
  float* out_dets;
  int32_t* out_labels;
  int64_t* out_index;
  int32_t* out_count;
};

static_assert(kSoftRegCap <= 16384, "the images kernel sorts at most 16384 keys in LDS");
constexpr int kImgWords = kSoftRegCap / 64 + 1;
constexpr int kImgSortCap = 16384;                           // the bitonic sort's power of two >= kSoftRegCap
constexpr size_t kImgLdsSort = (size_t)kImgSortCap * sizeof(uint64_t);
constexpr size_t kImgLdsLoop = (size_t)kImgWords * (8 + 4) + (size_t)kSoftMoveBatch * 4 + 16;
constexpr size_t kImgLds = kImgLdsSort > kImgLdsLoop ? kImgLdsSort : kImgLdsLoop;

__global__ __launch_bounds__(kImgThreads) void soft_nms_images_kernel(SoftImagesArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ SoftShared sh;
  const int img = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = p.counts[img];
  if (n <= 0) {
    if (tid == 0) p.out_count[img] = 0;
    return;
  }
  if (n >= p.split_thr || n > p.key_cap || n > kSoftRegCap) {
    if (tid == 0) p.out_count[img] = -1;  // caller must use yv4_soft_nms_split
    return;
  }
  uint64_t* gkeys = p.keys + (size_t)img * p.key_cap;
  // ---- 1. candidates into flat-index order: bitonic sort of the keys by their low word, written back in place ----------
  {
    uint64_t* sk = reinterpret_cast<uint64_t*>(lds_raw);
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += kImgThreads) {
      const uint64_t k = i < n ? gkeys[i] : ~0ull;
      sk[i] = (k << 32) | (k >> 32);                    // flat in the high word
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += kImgThreads) {
          const int i = ((t / j) * 2 * j) + (t % j);
          const int ixj = i + j;
          const bool up = (i & k) == 0;
          const uint64_t a = sk[i], b = sk[ixj];
          if ((a > b) == up) {
            sk[i] = b;
            sk[ixj] = a;
          }
        }
        __syncthreads();
      }
    }
    for (int i = tid; i < n; i += kImgThreads) {
      const uint64_t k = sk[i];
      gkeys[i] = (k << 32) | (k >> 32);
    }
  }
  // ---- 2. entries into registers: slot s = t + k*tn holds the s-th candidate at position s -------------------------------
  RegStore st;
  {
    // as many waves as give about kSoftPerThread entries per thread: fewer waves, a cheaper workgroup argmax
    const int tn = min(kImgThreads, ((n + kSoftPerThread - 1) / kSoftPerThread + 63) & ~63);
    st.tn = tn;
    const uint64_t* sk = reinterpret_cast<const uint64_t*>(lds_raw);
    const float off_unit = p.max_coord[img] + 1.f;
    const float* ibox = p.boxes + (size_t)img * p.boxes_per_image * 4;
    const int32_t* ilab = p.labels ? p.labels + (size_t)img * p.label_stride : nullptr;
#pragma unroll
    for (int k = 0; k < kSoftRegSlots; ++k) {
      const int s = tid + k * tn;
      st.pos[k] = kDead;
      st.s[k] = 0.f;
      st.b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (tid < tn && s < n) {
        const uint64_t key = sk[s];
        const uint32_t flat = (uint32_t)(key >> 32);
        const Candidate c = decode_candidate(flat, p.fused_classes, ilab);
        st.b[k] = offset_box(candidate_box(ibox, c), (float)c.label * off_unit);   // idxs.to(boxes) * (max + 1)
        st.s[k] = key_to_score((uint32_t)key);
        st.pos[k] = s;
      }
    }
  }
  __threadfence_block();
  __syncthreads();   // the sort buffer becomes the loop's bitmask / prefix / hole tables
  uint64_t* bits = reinterpret_cast<uint64_t*>(lds_raw);
  int* wpre = reinterpret_cast<int*>(bits + kImgWords);
  int* posA = wpre + kImgWords;
  float* odet = p.out_dets + (size_t)img * p.max_out * 5;
  int32_t* olab = p.out_labels + (size_t)img * p.max_out;
  int64_t* oidx = p.out_index + (size_t)img * p.max_out;
  const int r = soft_loop(st, n, p.max_out, false, p.q, sh, bits, wpre, posA, kImgWords,
                          [&](int rr, int slot, float score) {
                            odet[rr * 5 + 4] = score;
                            oidx[rr] = slot;        // slot for now: the candidate is resolved below
                          });
  __threadfence_block();
  __syncthreads();
  // ---- 3. the selections' candidates: slot -> flat index -> original box and label ------------------------------------
  {
    const float* ibox = p.boxes + (size_t)img * p.boxes_per_image * 4;
    const int32_t* ilab = p.labels ? p.labels + (size_t)img * p.label_stride : nullptr;
    const volatile int64_t* vidx = oidx;
    const volatile uint64_t* vkeys = gkeys;
    for (int q = tid; q < r; q += kImgThreads) {
      const int slot = (int)vidx[q];
      const uint32_t flat = (uint32_t)vkeys[slot];
      const Candidate c = decode_candidate(flat, p.fused_classes, ilab);
      const float4 ob = candidate_box(ibox, c);
      odet[q * 5 + 0] = ob.x;
      odet[q * 5 + 1] = ob.y;
      odet[q * 5 + 2] = ob.z;
      odet[q * 5 + 3] = ob.w;
      olab[q] = c.label;
      oidx[q] = (int64_t)flat;
    }
  }
  if (tid == 0) p.out_count[img] = r;
}

// ---- split: one workgroup per label segment over entries in global memory ---------------------------------------------
struct SoftSplitArgs {
  const uint64_t* keys;      // segment-major candidate keys, flat order inside a segment
  const int64_t* seg;        // num_segments + 1 bounds
  const float* boxes;
  const int32_t* labels;
  int fused;
  float off_unit;
  SoftParams q;
  int max_out;
  int tie_ext;
  float4* gbox;
  float* gscore;
  int* gpos;
  uint64_t* sel;             // per slot: the segment's selections (decayed score key << 32 | flat) in order, then ~0
  int nwords;
  int seg_cap;               // the largest segment the LDS tables were sized for
  int32_t* overflow;         // set when a segment is larger than the LDS tables were sized for
};

__global__ __launch_bounds__(kSoftThreads) void soft_nms_split_kernel(SoftSplitArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ SoftShared sh;
  const int tid = threadIdx.x;
  const int64_t lo = p.seg[blockIdx.x], hi = p.seg[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  if (n > p.seg_cap) {            // (only a problem above kSoftGlobalCap; the call then reports -2)
    if (tid == 0) *p.overflow = 1;
    return;
  }
  GlobalStore st;
  st.b = p.gbox;
  st.s = p.gscore;
  st.pos = p.gpos;
  st.lo = (int)lo;
  st.n = n;
  st.tn = min(kSoftThreads, (n + 63) & ~63);
  st.kbest = -1;
  for (int j = tid; j < n; j += st.tn) {
    const uint64_t key = p.keys[lo + j];
    const Candidate c = decode_candidate((uint32_t)key, p.fused, p.labels);
    p.gbox[lo + j] = offset_box(candidate_box(p.boxes, c), (float)c.label * p.off_unit);
    p.gscore[lo + j] = key_to_score((uint32_t)(key >> 32));
    p.gpos[lo + j] = j;
  }
  uint64_t* bits = reinterpret_cast<uint64_t*>(lds_raw);
  int* wpre = reinterpret_cast<int*>(bits + p.nwords);
  int* posA = wpre + p.nwords;
  uint64_t* sel = p.sel + lo;
  const int r = soft_loop(st, n, p.max_out, p.tie_ext != 0, p.q, sh, bits, wpre, posA, p.nwords,
                          [&](int rr, int slot, float score) {
                            sel[rr] = ((uint64_t)score_to_key(score) << 32) | (uint32_t)slot;
                          });
  __threadfence_block();
  __syncthreads();
  const volatile uint64_t* vsel = sel;
  for (int q = tid; q < n; q += kSoftThreads) {
    if (q < r) {
      const uint64_t v = vsel[q];
      const uint32_t flat = (uint32_t)p.keys[(uint32_t)v];
      sel[q] = (v & 0xffffffff00000000ull) | flat;
    } else {
      sel[q] = ~0ull;
    }
  }
}

__global__ __launch_bounds__(256) void soft_labels_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                          const int32_t* __restrict__ labels, int fused,
                                                          int32_t* __restrict__ out_labels) {
  key_labels_body(keys, n, labels, fused, out_labels);
}

// seg[c] = first position with label >= c (num_classes + 1 entries); one segment [0, n) when per_label == 0
__global__ __launch_bounds__(256) void soft_segments_kernel(const int32_t* __restrict__ sorted_labels, int64_t n,
                                                            int num_classes, int per_label, int64_t* __restrict__ seg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > num_classes) return;
  if (!per_label) {
    seg[c] = c == 0 ? 0 : n;
    return;
  }
  seg[c] = label_lower_bound(sorted_labels, n, c);
}

__global__ __launch_bounds__(256) void soft_emit_kernel(const uint64_t* __restrict__ sel, int64_t n,
                                                        const float* __restrict__ boxes,
                                                        const int32_t* __restrict__ labels, int fused, int max_out,
                                                        float* out_dets, int32_t* out_labels, int64_t* out_index,
                                                        int32_t* out_count, const int32_t* overflow) {
  if (*overflow) {
    if (blockIdx.x * blockDim.x + threadIdx.x == 0) *out_count = -2;
    return;
  }
  emit_body(sel, n, boxes, labels, fused, max_out, out_dets, out_labels, out_index, out_count);
}

// the common pieces, then the entries in global memory (class-offset box, current score, position word), the
// selections per slot and the overflow flag
struct SoftSplitLayout : SplitSortLayout {
  size_t gbox, gscore, gpos, sel, flag, total;
  explicit SoftSplitLayout(int64_t n) : SplitSortLayout(n) {
    gbox = carve.take((size_t)n * 16);
    gscore = carve.take((size_t)n * 4);
    gpos = carve.take((size_t)n * 4);
    sel = carve.take((size_t)n * 8);
    flag = carve.take(4);
    total = carve.off;
  }
};

int soft_words(int64_t n) { return (int)(n / 64) + 2; }
size_t soft_split_lds(int64_t n) { return (size_t)soft_words(n) * (8 + 4) + (size_t)kSoftMoveBatch * 4 + 16; }

const char* check_params(int method, float sigma) {
  if (method != YV4_SOFT_NMS_NAIVE && method != YV4_SOFT_NMS_LINEAR && method != YV4_SOFT_NMS_GAUSSIAN)
    return "unknown method (YV4_SOFT_NMS_NAIVE / _LINEAR / _GAUSSIAN)";
  if (method == YV4_SOFT_NMS_GAUSSIAN && !(sigma > 0.f)) return "sigma must be > 0 for the gaussian method";
  return nullptr;
}

}  // namespace
}  // namespace yv4

using namespace yv4;

extern "C" int yv4_soft_nms_images(uint64_t* keys, int64_t key_cap, const int32_t* counts, const float* max_coord,
                                   const float* boxes, int64_t boxes_per_image, const int32_t* labels,
                                   int64_t label_stride, int fused_classes, int N, int method, float iou_thr,
                                   float sigma, float min_score, int max_out, int split_thr, float* out_dets,
                                   int32_t* out_labels, int64_t* out_index, int32_t* out_count, void* stream) {
  const char* bad = check_params(method, sigma);
  YV4_REQUIRE(!bad, "soft_nms_images: %s", bad ? bad : "");
  YV4_REQUIRE(keys && counts && max_coord && boxes && out_dets && out_labels && out_index && out_count,
              "soft_nms_images: null pointer");
  YV4_REQUIRE(N > 0 && N <= 65535 && max_out > 0 && key_cap > 0 && boxes_per_image > 0,
              "soft_nms_images: bad sizes");
  YV4_REQUIRE(fused_classes >= 0, "soft_nms_images: fused_classes must be >= 0");
  YV4_REQUIRE(((uintptr_t)boxes & 15) == 0, "soft_nms_images: boxes must be 16-byte aligned");
  if (split_thr <= 0 || split_thr > kSoftRegCap) split_thr = kSoftRegCap + 1;
  SoftImagesArgs a;
  a.keys = keys; a.key_cap = key_cap; a.counts = counts; a.max_coord = max_coord; a.boxes = boxes;
  a.boxes_per_image = boxes_per_image; a.labels = labels; a.label_stride = label_stride;
  a.fused_classes = fused_classes; a.q.method = method; a.q.thr = iou_thr; a.q.sigma = sigma; a.q.min_score = min_score;
  a.max_out = max_out; a.split_thr = split_thr;
  a.out_dets = out_dets; a.out_labels = out_labels; a.out_index = out_index; a.out_count = out_count;
  static LdsAttrOnce once;
  if (int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(soft_nms_images_kernel), kImgLds, "soft_nms_images"))
    return rc;
  hipLaunchKernelGGL(soft_nms_images_kernel, dim3(N), dim3(kImgThreads), kImgLds, reinterpret_cast<hipStream_t>(stream),
                     a);
  YV4_CHECK_LAUNCH("soft_nms_images");
  return YV4_OK;
}

extern "C" size_t yv4_soft_nms_split_work(int64_t n) {
  if (n <= 0 || n >= (1LL << 31)) return 0;
  return SoftSplitLayout(n).total;
}

extern "C" int yv4_soft_nms_split(const uint64_t* keys, int64_t n, float max_coord, const float* boxes,
                                  const int32_t* labels, int fused_classes, int per_label, int method, float iou_thr,
                                  float sigma, float min_score, int max_out, void* work, float* out_dets,
                                  int32_t* out_labels, int64_t* out_index, int32_t* out_count, void* stream) {
  const char* bad = check_params(method, sigma);
  YV4_REQUIRE(!bad, "soft_nms_split: %s", bad ? bad : "");
  YV4_REQUIRE(keys && boxes && work && out_dets && out_labels && out_index && out_count, "soft_nms_split: null pointer");
  YV4_REQUIRE(n > 0 && n < (1LL << 31), "soft_nms_split: n out of range");
  YV4_REQUIRE(per_label == 1 || n <= kSoftGlobalCap, "soft_nms_split: one problem of at most %d candidates", kSoftGlobalCap);
  YV4_REQUIRE(max_out > 0 && fused_classes >= 0 && fused_classes <= kSplitMaxClasses,
              "soft_nms_split: bad max_out / classes");
  YV4_REQUIRE(per_label == 0 || per_label == 1, "soft_nms_split: per_label must be 0 or 1");
  YV4_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)work & 255) == 0,
              "soft_nms_split: boxes must be 16-byte and work 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int num_classes = per_label ? (fused_classes > 0 ? fused_classes : kSplitMaxClasses) : 1;
  const SoftSplitLayout L(n);
  char* w = reinterpret_cast<char*>(work);
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(w + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(w + L.keys_b);
  uint64_t* keys_t = reinterpret_cast<uint64_t*>(w + L.keys_t);
  int32_t* lab_a = reinterpret_cast<int32_t*>(w + L.lab_a);
  int32_t* lab_b = reinterpret_cast<int32_t*>(w + L.lab_b);
  uint32_t* lab_t = reinterpret_cast<uint32_t*>(w + L.lab_t);
  int64_t* seg = reinterpret_cast<int64_t*>(w + L.seg);
  uint64_t* sel = reinterpret_cast<uint64_t*>(w + L.sel);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + L.hist);
  int32_t* overflow = reinterpret_cast<int32_t*>(w + L.flag);
  const unsigned g = (unsigned)((n + 255) / 256);
  if (hipMemsetAsync(overflow, 0, sizeof(int32_t), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("soft_nms_split: hipMemsetAsync failed");
    return YV4_E_LAUNCH;
  }
  // 1. flat-index order (the low word of the keys)
  if (int rc = rs_sort<uint64_t, int, false>(keys, keys_a, keys_t, nullptr, nullptr, nullptr, n, 32, hist, s)) return rc;
  const uint64_t* seg_keys = keys_a;
  // 2. stable by label: label-major, flat order kept (nms_split.hip's grouping)
  if (per_label) {
    hipLaunchKernelGGL(soft_labels_kernel, dim3(g), dim3(256), 0, s, keys_a, n, labels, fused_classes, lab_a);
    if (int rc = rs_sort<uint32_t, uint64_t, true>(reinterpret_cast<const uint32_t*>(lab_a),
                                                   reinterpret_cast<uint32_t*>(lab_b), lab_t, keys_a, keys_b, keys_t, n,
                                                   16, hist, s))
      return rc;
    seg_keys = keys_b;
  }
  hipLaunchKernelGGL(soft_segments_kernel, dim3((num_classes + 1 + 255) / 256), dim3(256), 0, s, lab_b, n, num_classes,
                     per_label, seg);
  // 3. soft-NMS per segment
  SoftSplitArgs a;
  a.keys = seg_keys; a.seg = seg; a.boxes = boxes; a.labels = labels; a.fused = fused_classes;
  a.off_unit = max_coord + 1.f;
  a.q.method = method; a.q.thr = iou_thr; a.q.sigma = sigma; a.q.min_score = min_score;
  a.max_out = max_out; a.tie_ext = per_label;
  a.gbox = reinterpret_cast<float4*>(w + L.gbox); a.gscore = reinterpret_cast<float*>(w + L.gscore);
  const int64_t lds_n = n < kSoftGlobalCap ? n : kSoftGlobalCap;    // a label's problem is at most kSoftGlobalCap
  a.gpos = reinterpret_cast<int*>(w + L.gpos); a.sel = sel; a.nwords = soft_words(lds_n); a.seg_cap = (int)lds_n;
  a.overflow = overflow;
  static LdsAttrOnce once;
  if (int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(soft_nms_split_kernel), soft_split_lds(kSoftGlobalCap),
                              "soft_nms_split"))
    return rc;
  hipLaunchKernelGGL(soft_nms_split_kernel, dim3(num_classes), dim3(kSoftThreads), soft_split_lds(lds_n), s, a);
  // 4. per label: survivors by (decayed score desc, flat index asc); one problem: selection order
  const uint64_t* out_sel = sel;
  if (per_label) {
    if (int rc = rs_sort<uint64_t, int, false>(sel, keys_a, keys_t, nullptr, nullptr, nullptr, n, 64, hist, s)) return rc;
    out_sel = keys_a;
  }
  const int lim = (int)(n < max_out ? n : max_out);
  hipLaunchKernelGGL(soft_emit_kernel, dim3((lim + 255) / 256), dim3(256), 0, s, out_sel, n, boxes, labels, fused_classes,
                     max_out, out_dets, out_labels, out_index, out_count, overflow);
  YV4_CHECK_LAUNCH("soft_nms_split");
  return YV4_OK;
}
