// YOLOV3Head training loss, forward and backward, without a host round trip:
//   mmdet/core/bbox/assigners/grid_assigner.py:73-156     GridAssigner.assign
//   mmdet/core/anchor/anchor_generator.py:667-727          responsible_flags (+ grid_anchors)
//   mmdet/core/bbox/iou_calculators/iou2d_calculator.py    BboxOverlaps2D (gts as bboxes1)
//   mmdet/core/bbox/coder/yolo_bbox_coder.py:26-60         encode
//   mmdet/models/dense_heads/yolo_head.py:396-586          loss / loss_single / get_targets / _get_targets_single
// The reference runs one Python pass per image with a per-ground-truth loop that reads a device value on the host,
// builds a dense fp32 (N, anchors, 5+C) target map and reduces it with ~30 small launches per level.  Here:
//
//   prep     per-image ground-truth ranges (gt_img is non-decreasing), per-gt max / argmax words initialised.
//   cand     one thread per candidate (ground truth g, level l, base anchor a): g's centre cell at level l holds a
//            responsible anchor; its IoUs against every ground truth of the image go into that ground truth's max
//            (an integer atomicMax on the bit pattern: IoUs are non-negative floats).  With gt_max_assign_all = 0 a
//            second launch takes, per ground truth, the smallest anchor index that attains the max (torch's argmax).
//   dense    one thread per anchor box: its final id (a pure function of the anchor and the per-gt tables), then --
//            forward -- the four loss sums of the row, or -- backward -- the whole gradient row, written once.
//
// IoUs are evaluated in BboxOverlaps2D's expression order, fp32, compiled with -ffp-contract=off: the equality test of
// the per-gt claims needs them bit-identical to the reference's.  Sums run in double, or -- yv4_set_deterministic(1)
// -- in fixed-point words (order-independent).  The backward writes every element once and has no sums.
#include "yv4_common.h"

#include <climits>

namespace yv4 {

constexpr int kV3Levels = YV4_V3_LOSS_MAX_LEVELS;

struct V3Lv {
  const float* pred; float* dpred;
  long long sn, sc, sh, sw;
  int H, W, stride, a_inner;  // a_inner: rows enumerate (n, y, x, a) -- channels-last maps; else (n, a, y, x)
  int rows;                   // N * H * W * A
  float base[8][4];
  long long anchor_off;       // first anchor box of the level inside an image
  long long block0;           // first workgroup of the level in the dense launches
};

struct V3Args {
  V3Lv lv[kV3Levels];
  int L, N, A, C, attr, G, all;
  long long TA;               // anchor boxes per image, all levels
  const float* gt; const int64_t* gt_label; const int64_t* gt_img;
  float pos_thr, neg_lo, neg_hi, min_pos, eps, eps_hi, iou_eps, smooth;
  float w[4]; int mean[4];
  int32_t* img_off; int32_t* gt_cell; int32_t* gt_max; int32_t* gt_arg; int32_t* assigned;
  double* sums; float* losses; const float* gout;
  int det;
};

// BboxOverlaps2D(gt, anchor): union = area_gt + area_anchor - overlap, clamped to eps, then overlap / union
__device__ __forceinline__ float iou_gt_box(const float* g, float ax1, float ay1, float ax2, float ay2, float eps) {
  const float area1 = (g[2] - g[0]) * (g[3] - g[1]);
  const float area2 = (ax2 - ax1) * (ay2 - ay1);
  const float lx = fmaxf(g[0], ax1), ly = fmaxf(g[1], ay1);
  const float rx = fminf(g[2], ax2), ry = fminf(g[3], ay2);
  const float w = fmaxf(rx - lx, 0.f), h = fmaxf(ry - ly, 0.f);
  const float ov = w * h;
  const float u = fmaxf(area1 + area2 - ov, eps);
  return ov / u;
}

// ordered integer key of a non-negative float (a -0 IoU counts as 0)
__device__ __forceinline__ int iou_key(float v) { return __float_as_int(v) & 0x7fffffff; }

__device__ __forceinline__ float bce_logits_v3(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

__device__ __forceinline__ void anchor_box(const V3Lv& lv, int a, int x, int y, float b[4]) {
  const float sx = (float)(x * lv.stride), sy = (float)(y * lv.stride);   // grid_anchors: base + shift, fp32
  b[0] = lv.base[a][0] + sx; b[1] = lv.base[a][1] + sy; b[2] = lv.base[a][2] + sx; b[3] = lv.base[a][3] + sy;
}

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void v3_prep_kernel(V3Args p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= p.N) {                       // img_off[n] = number of ground truths of images < n
    int lo = 0, hi = p.G;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.gt_img[mid] < i) lo = mid + 1; else hi = mid;
    }
    p.img_off[i] = lo;
  }
  if (i < p.G) {
    p.gt_max[i] = __float_as_int(-1.f);  // below every IoU key: "no responsible anchor"
    p.gt_arg[i] = INT_MAX;
  }
}

template <bool ARGMIN>
__global__ __launch_bounds__(256) void v3_cand_kernel(V3Args p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.G * p.L * p.A) return;
  const int g = i / (p.L * p.A);
  const int r = i - g * p.L * p.A;
  const int l = r / p.A, a = r - l * p.A;
  const V3Lv& lv = p.lv[l];
  const float* b = p.gt + 4 * (size_t)g;
  const float cx = (b[0] + b[2]) * 0.5f, cy = (b[1] + b[3]) * 0.5f;
  const float fx = floorf(cx / (float)lv.stride), fy = floorf(cy / (float)lv.stride);
  const long long img = p.gt_img[g];
  // a centre cell off the map (the reference raises or wraps there) holds no responsible anchor
  const bool in = fx >= 0.f && fx < (float)lv.W && fy >= 0.f && fy < (float)lv.H && img >= 0 && img < p.N;
  const int gx = in ? (int)fx : 0, gy = in ? (int)fy : 0;
  if (!ARGMIN && a == 0) p.gt_cell[l * p.G + g] = in ? gy * lv.W + gx : -1;
  if (!in) return;
  float box[4];
  anchor_box(lv, a, gx, gy, box);
  const int aidx = (int)(lv.anchor_off + (long long)(gy * lv.W + gx) * p.A + a);
  const int g0 = p.img_off[img], g1 = p.img_off[img + 1];
  for (int j = g0; j < g1; ++j) {
    const float v = iou_gt_box(p.gt + 4 * (size_t)j, box[0], box[1], box[2], box[3], p.iou_eps);
    if (!ARGMIN) atomicMax(&p.gt_max[j], iou_key(v));
    else if (iou_key(v) == p.gt_max[j]) atomicMin(&p.gt_arg[j], aidx);
  }
}

// ---------------------------------------------------------------------------------------------------------
struct RowPos { int n, a, x, y, cell; long long aidx; };

__device__ __forceinline__ RowPos row_pos(const V3Args& p, const V3Lv& lv, int r) {
  RowPos q;
  const int HW = lv.H * lv.W, HWA = HW * p.A;
  q.n = r / HWA;
  const int rem = r - q.n * HWA;
  if (lv.a_inner) { q.cell = rem / p.A; q.a = rem - q.cell * p.A; }
  else { q.a = rem / HW; q.cell = rem - q.a * HW; }
  q.y = q.cell / lv.W; q.x = q.cell - q.y * lv.W;
  q.aidx = lv.anchor_off + (long long)q.cell * p.A + q.a;
  return q;
}

// assigned_gt_inds of one anchor box: -1 ignore, 0 negative, k > 0 the image's ground truth k-1
__device__ int resolve_id(const V3Args& p, int l, const RowPos& q, const float box[4]) {
  const int g0 = p.img_off[q.n], g1 = p.img_off[q.n + 1];
  if (g1 == g0) return 0;                                   // no ground truth: everything is negative
  float best = -INFINITY;
  int arg = 0;
  bool resp = false;
  for (int j = g0; j < g1; ++j) {
    const float v = iou_gt_box(p.gt + 4 * (size_t)j, box[0], box[1], box[2], box[3], p.iou_eps);
    if (v > best) { best = v; arg = j - g0; }               // first maximum, like torch.max(dim=0)
    resp = resp || p.gt_cell[l * p.G + j] == q.cell;
  }
  int id = (best > p.neg_lo && best <= p.neg_hi) ? 0 : -1;
  if (!resp) return id;
  if (best > p.pos_thr) id = arg + 1;
  for (int j = g0; j < g1; ++j) {                          // per-gt claims in gt order: a later one overwrites
    const int key = p.gt_max[j];
    if (key < 0) continue;                                  // no responsible anchor for this ground truth
    const float m = __int_as_float(key);
    if (!(m > p.min_pos)) continue;
    if (p.all) {
      if (iou_key(iou_gt_box(p.gt + 4 * (size_t)j, box[0], box[1], box[2], box[3], p.iou_eps)) == key) id = j - g0 + 1;
    } else if ((long long)p.gt_arg[j] == q.aidx) {
      id = j - g0 + 1;
    }
  }
  return id;
}

// YOLOBBoxCoder.encode of a positive, in the coder's order
__device__ __forceinline__ void encode_v3(const float* g, const float b[4], float stride, float eps, float eps_hi,
                                          float t[4]) {
  const float xg = (g[0] + g[2]) * 0.5f, yg = (g[1] + g[3]) * 0.5f;
  const float wg = g[2] - g[0], hg = g[3] - g[1];
  const float xc = (b[0] + b[2]) * 0.5f, yc = (b[1] + b[3]) * 0.5f;
  const float w = b[2] - b[0], h = b[3] - b[1];
  t[2] = logf(fmaxf(wg / w, eps));
  t[3] = logf(fmaxf(hg / h, eps));
  t[0] = fminf(fmaxf((xg - xc) / stride + 0.5f, eps), eps_hi);
  t[1] = fminf(fmaxf((yg - yc) / stride + 0.5f, eps), eps_hi);
}

__device__ __forceinline__ double count_of(const V3Args& p, const V3Lv& lv, int term) {
  const double rows = (double)lv.rows;
  return term == 0 ? rows * p.C : (term == 1 ? rows : rows * 2.0);
}

template <bool BWD>
__global__ __launch_bounds__(256) void v3_dense_kernel(V3Args p) {
  int l = 0;
  while (l + 1 < p.L && (long long)blockIdx.x >= p.lv[l + 1].block0) ++l;
  const V3Lv& lv = p.lv[l];
  const int r = (int)(((long long)blockIdx.x - lv.block0) * 256 + threadIdx.x);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < lv.rows) {
    const RowPos q = row_pos(p, lv, r);
    float box[4];
    anchor_box(lv, q.a, q.x, q.y, box);
    int32_t* asg = p.assigned + (long long)q.n * p.TA + q.aidx;
    const int id = BWD ? *asg : resolve_id(p, l, q, box);
    if (!BWD) *asg = id;
    const long long base = (long long)q.n * lv.sn + (long long)q.a * p.attr * lv.sc + (long long)q.y * lv.sh +
                           (long long)q.x * lv.sw;
    const float* row = lv.pred + base;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    int label = -1;
    if (id > 0) {
      const int gj = p.img_off[q.n] + id - 1;
      encode_v3(p.gt + 4 * (size_t)gj, box, (float)lv.stride, p.eps, p.eps_hi, t);
      label = (int)p.gt_label[gj];
    }
    const float t_on = p.smooth != 0.f ? (1.f - p.smooth) + p.smooth / (float)p.C : 1.f;
    const float t_off = p.smooth != 0.f ? p.smooth / (float)p.C : 0.f;
    if (!BWD) {
      if (id > 0) {
        double c = 0.0;
        for (int k = 0; k < p.C; ++k) c += (double)bce_logits_v3(row[(long long)(5 + k) * lv.sc], k == label ? t_on : t_off);
        s[0] = c;
        s[1] = (double)bce_logits_v3(row[4 * lv.sc], 1.f);
        s[2] = (double)bce_logits_v3(row[0], t[0]) + (double)bce_logits_v3(row[lv.sc], t[1]);
        const float d2 = row[2 * lv.sc] - t[2], d3 = row[3 * lv.sc] - t[3];
        s[3] = (double)(d2 * d2) + (double)(d3 * d3);
      } else if (id == 0) {
        s[1] = (double)bce_logits_v3(row[4 * lv.sc], 0.f);
      }
    } else {
      float k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        k[u] = p.gout[l * 4 + u] * p.w[u];
        if (p.mean[u]) k[u] = k[u] / (float)count_of(p, lv, u);
      }
      float* drow = lv.dpred + base;
      const bool pos = id > 0;
      for (int j = 0; j < p.attr; ++j) {
        float v = 0.f;
        if (j == 4) {
          if (id >= 0) v = (sigmoid_f32(row[4 * lv.sc]) - (pos ? 1.f : 0.f)) * k[1];
        } else if (pos) {
          const float x = row[(long long)j * lv.sc];
          if (j < 2) v = (sigmoid_f32(x) - t[j]) * k[2];
          else if (j < 4) v = 2.f * (x - t[j]) * k[3];
          else v = (sigmoid_f32(x) - (j - 5 == label ? t_on : t_off)) * k[0];
        }
        drow[(long long)j * lv.sc] = v;
      }
    }
  }
  if (BWD) return;
  // workgroup reduction of the four sums, then one atomic (or fixed-point add) per term
  __shared__ double red[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    double v = s[u];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][u] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int u = threadIdx.x;
    const double v = ((red[0][u] + red[1][u]) + red[2][u]) + red[3][u];
    if (v != 0.0) {
      const int i = l * 4 + u;
      if (p.det) fx_add<kFxStat>(reinterpret_cast<u64_t*>(p.sums) + i, reinterpret_cast<u64_t*>(p.sums) + 4 * p.L + i, v);
      else atomicAdd(&p.sums[i], v);
    }
  }
}

// sums -> the (L, 4) losses [cls | conf | xy | wh]: loss_weight * sum (/ element count for reduction='mean')
__global__ void v3_finish_kernel(V3Args p) {
  const int i = threadIdx.x;
  if (i >= 4 * p.L) return;
  const int l = i / 4, u = i - l * 4;
  const u64_t* wds = reinterpret_cast<const u64_t*>(p.sums);
  double v = p.det ? fx_value<kFxStat>(wds[i], wds[4 * p.L + i]) : p.sums[i];
  v *= (double)p.w[u];
  if (p.mean[u]) v /= count_of(p, p.lv[l], u);
  p.losses[i] = (float)v;
}

static int fill_v3_args(const yv4_v3_loss_desc* d, V3Args& a, const char* who) {
  YV4_REQUIRE(d, "%s: null descriptor", who);
  YV4_REQUIRE(d->num_levels >= 1 && d->num_levels <= kV3Levels, "%s: 1..%d levels", who, kV3Levels);
  YV4_REQUIRE(d->N > 0 && d->A >= 1 && d->A <= 8 && d->num_classes >= 1 && d->G >= 0, "%s: bad sizes", who);
  YV4_REQUIRE(d->img_off && d->gt_cell && d->gt_max && d->gt_arg && d->assigned && d->sums,
              "%s: work buffers missing", who);
  YV4_REQUIRE(d->G == 0 || (d->gt && d->gt_label && d->gt_img), "%s: ground-truth tables missing", who);
  a = V3Args{};
  a.L = d->num_levels; a.N = d->N; a.A = d->A; a.C = d->num_classes; a.attr = 5 + d->num_classes; a.G = d->G;
  a.all = d->gt_max_assign_all ? 1 : 0;
  long long off = 0, blocks = 0;
  for (int l = 0; l < a.L; ++l) {
    const yv4_v3_loss_level& s = d->levels[l];
    YV4_REQUIRE(s.pred && s.H > 0 && s.W > 0 && s.stride > 0, "%s: level %d incomplete", who, l);
    YV4_REQUIRE(s.sn > 0 && s.sc > 0 && s.sh > 0 && s.sw > 0, "%s: level %d: strides must be positive", who, l);
    V3Lv& t = a.lv[l];
    t.pred = s.pred; t.dpred = s.dpred;
    t.sn = s.sn; t.sc = s.sc; t.sh = s.sh; t.sw = s.sw;
    t.H = s.H; t.W = s.W; t.stride = s.stride;
    t.a_inner = s.sc == 1 ? 1 : 0;
    const long long rows = (long long)d->N * s.H * s.W * d->A;
    YV4_REQUIRE(rows < (1LL << 31) - 256, "%s: level %d: map too large", who, l);
    YV4_REQUIRE((long long)(s.W - 1) * s.stride < (1LL << 24) && (long long)(s.H - 1) * s.stride < (1LL << 24),
                "%s: level %d: grid shifts must be exact in fp32", who, l);
    t.rows = (int)rows;
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < 4; ++c) t.base[k][c] = s.base_anchors[k][c];
    t.anchor_off = off;
    off += (long long)s.H * s.W * d->A;
    t.block0 = blocks;
    blocks += (rows + 255) / 256;
  }
  a.TA = off;
  YV4_REQUIRE(a.TA < (1LL << 31) && blocks < (1LL << 31) && (long long)a.G * a.L * a.A < (1LL << 31),
              "%s: index space exceeds 31 bits", who);
  a.gt = d->gt; a.gt_label = d->gt_label; a.gt_img = d->gt_img;
  a.pos_thr = d->pos_iou_thr; a.neg_lo = d->neg_lo; a.neg_hi = d->neg_hi; a.min_pos = d->min_pos_iou;
  a.eps = d->eps; a.eps_hi = d->eps_hi; a.iou_eps = d->iou_eps; a.smooth = d->smoother;
  for (int u = 0; u < 4; ++u) { a.w[u] = d->loss_weight[u]; a.mean[u] = d->reduce_mean[u] ? 1 : 0; }
  a.img_off = d->img_off; a.gt_cell = d->gt_cell; a.gt_max = d->gt_max; a.gt_arg = d->gt_arg; a.assigned = d->assigned;
  a.sums = d->sums; a.losses = d->losses;
  a.det = deterministic() ? 1 : 0;
  return YV4_OK;
}

static unsigned dense_blocks(const V3Args& a) {
  return (unsigned)(a.lv[a.L - 1].block0 + ((long long)a.lv[a.L - 1].rows + 255) / 256);
}

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_yolov3_loss_fwd(const yv4_v3_loss_desc* d, void* stream) {
  V3Args a;
  if (int rc = fill_v3_args(d, a, "yolov3_loss_fwd")) return rc;
  YV4_REQUIRE(a.losses, "yolov3_loss_fwd: losses missing");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(a.sums, 0, sizeof(double) * 2 * 4 * a.L, s) != hipSuccess) {
    set_error("yolov3_loss_fwd: memset failed");
    return YV4_E_LAUNCH;
  }
  const int prep = (a.G > a.N + 1 ? a.G : a.N + 1);
  hipLaunchKernelGGL(v3_prep_kernel, dim3((unsigned)((prep + 255) / 256)), dim3(256), 0, s, a);
  const int cand = a.G * a.L * a.A;
  if (cand > 0) {
    hipLaunchKernelGGL(v3_cand_kernel<false>, dim3((unsigned)((cand + 255) / 256)), dim3(256), 0, s, a);
    if (!a.all) hipLaunchKernelGGL(v3_cand_kernel<true>, dim3((unsigned)((cand + 255) / 256)), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(v3_dense_kernel<false>, dim3(dense_blocks(a)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(v3_finish_kernel, dim3(1), dim3(64), 0, s, a);
  YV4_CHECK_LAUNCH("yolov3_loss_fwd");
  return YV4_OK;
}

extern "C" int yv4_yolov3_loss_bwd(const yv4_v3_loss_desc* d, const float* grad_out, void* stream) {
  V3Args a;
  if (int rc = fill_v3_args(d, a, "yolov3_loss_bwd")) return rc;
  YV4_REQUIRE(grad_out, "yolov3_loss_bwd: grad_out missing");
  for (int l = 0; l < a.L; ++l) YV4_REQUIRE(a.lv[l].dpred, "yolov3_loss_bwd: level %d: dpred missing", l);
  a.gout = grad_out;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(v3_dense_kernel<true>, dim3(dense_blocks(a)), dim3(256), 0, s, a);
  YV4_CHECK_LAUNCH("yolov3_loss_bwd");
  return YV4_OK;
}
