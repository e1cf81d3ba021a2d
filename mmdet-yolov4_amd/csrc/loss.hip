// YOLOCSPHead training loss, forward and backward, in three kernels each way and without a host round trip:
//   mmdet/core/anchor/yolov4_anchor_generator.py:12-134   responsible_indices (neighbor = 2)
//   mmdet/models/dense_heads/yolocsp_head.py:384-575       loss / loss_single_no_assigner / get_targets_no_assigner
//   mmdet/core/bbox/coder/yolov4_bbox_coder.py:39-67       decode
//   mmdet/core/bbox/iou_calculators/iou2d_calculator.py    aligned GIoU (eps on union and on the enclosing area)
//   mmdet/models/losses/cross_entropy_loss.py:58-91        sigmoid BCE, mean
//   mmdet/models/losses/iou_loss.py:14-36,105-219          IoU (linear / log), DIoU, CIoU: box_terms<KIND> below
//   mmdet/models/dense_heads/yolocsp_head.py:21-50         SoftFocalLoss around the BCE, objectness and / or class term
// The reference builds the positives with ~150 small tensor ops and two nonzero() host syncs per level, gathers
// them out of a dense fp32 (N, H*W*A, 5+C) copy of the prediction map and scatters the objectness targets with
// an index_put whose result for duplicate positives depends on the execution order.  Here:
//
//   assign   one thread per candidate slot (level, neighbour kind k, base anchor a, ground truth g): shape test,
//            neighbour-cell test, anchor index.  The slot number (k*A + a)*G + g is the position the positive has
//            in the reference's index lists (mask indexing is row-major), so "the last write wins" -- what the
//            reference's index_put does when it runs sequentially -- is an atomicMax of the slot number per
//            anchor box: deterministic, no compaction, no count needed on the host.
//   pos      one wavefront per valid slot: the 5+C logits of its anchor box straight from the head conv's raw
//            NHWC output (+ bias), decode, box loss (GIoU or another member of the family), class BCE; forward writes the objectness target of the slot and
//            adds to the loss sums (double); backward accumulates the row gradient into the winner slot's row.
//   dense    forward: objectness BCE over every anchor box, target = the winner slot's (or 0); backward: writes
//            the WHOLE gradient tensor of the conv output once (zeros, objectness gradients, the positive rows),
//            in the conv's own dtype and layout, and reduces the bias gradient on the way.
//
// Arithmetic is fp32 in the reference's expression order where a value is rounded (decode, GIoU); sums run in
// double.  Compiled with -ffp-contract=off.
#include "yv4_common.h"

namespace yv4 {

constexpr int kLossLevels = YV4_LOSS_MAX_LEVELS;

struct LossLv {
  const void* raw; void* draw; const float* bias; double* dbias;
  int H, W, Cp, stride;
  float base[8][4];
  long long anchor_off;   // first anchor box of the level inside an image
  long long block0;       // first workgroup of the level in the dense backward launch
  FastDiv fd_hw, fd_cpr;  // row / (H*W), chunk index / (Cp / chunk): the dense backward runs one divide per 16 bytes
};

struct LossArgs {
  LossLv lv[kLossLevels];
  int L, N, A, attr, C, G;
  long long TA;           // anchor boxes per image, all levels
  long long S;            // candidate slots per level = 5 * A * G
  FastDiv fd_TA, fd_A;
  const float* gt; const int64_t* gt_label; const int64_t* gt_img;
  float shape_thr, smooth, ratio, eps, w_cls, w_conf, w_bbox;
  int32_t* slot_anchor; int32_t* winner; int32_t* npos; float* conf_t; float* gpos; double* sums;
  const float* gout;
  float* losses;          // optional: (L, 3) float [cls | conf | bbox] written by the forward's last kernel
  int box_kind;           // YV4_BOX_*: selects the yolo_pos_kernel instantiation on the host
  float conf_gamma, conf_alpha, cls_gamma, cls_alpha;     // SoftFocalLoss on the objectness / class term (where selected)
  int det;                // yv4_set_deterministic: sums / dbias / gpos are fixed-point words, [hi (n) | lo (n)] each
  long long gpos_n;       // L * S * attr
};

// loss sums (3 per level): doubles, or fixed-point words with the lo words 3*L entries further on
__device__ __forceinline__ void loss_sum_add(const LossArgs& p, int i, double v) {
  if (p.det) fx_add<kFxStat>(reinterpret_cast<u64_t*>(p.sums) + i, reinterpret_cast<u64_t*>(p.sums) + 3 * p.L + i, v);
  else atomicAdd(&p.sums[i], v);
}
// sums (doubles by now) + npos -> the (L, 3) losses: one thread per level
__global__ void loss_finish_kernel(LossArgs p) {
  const int l = threadIdx.x;
  if (l >= p.L) return;
  const double n = (double)p.npos[l];
  const double per_pos = n > 0.0 ? 1.0 / n : 0.0;
  const double boxes = (double)p.N * p.lv[l].H * p.lv[l].W * p.A;
  p.losses[l * 3 + 0] = (float)(p.sums[l * 3 + 0] * per_pos / (double)(p.C > 0 ? p.C : 1) * (double)p.w_cls);
  p.losses[l * 3 + 1] = (float)(p.sums[l * 3 + 1] / boxes * (double)p.w_conf);
  p.losses[l * 3 + 2] = (float)(p.sums[l * 3 + 2] * per_pos * (double)p.w_bbox);
}

template <int SHIFT>
__global__ void loss_fx_decode_kernel(double* __restrict__ buf, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64_t* w = reinterpret_cast<const u64_t*>(buf);
  buf[i] = fx_value<SHIFT>(w[i], w[n + i]);
}

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }

__device__ __forceinline__ float rem1(float v) {      // torch's `v % 1.` (remainder: sign of the divisor)
  float r = fmodf(v, 1.f);
  if (r < 0.f) r += 1.f;
  return r;
}

__device__ __forceinline__ float bce_logits(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// SoftFocalLoss (yolocsp_head.py:21-50) around the sigmoid BCE, soft target t:
//   loss = bce * (t*alpha + (1-t)*(1-alpha)) * (1 - p_t)**gamma,   p_t = t*p + (1-t)*(1-p),   p = sigmoid(x)
// in the reference's expression order.  gamma >= 1 (host): the derivative's (1 - p_t)**(gamma-1) is then finite at
// p_t = 1.
// m**g for the base m = 1 - p_t in [0, 1]: exp2(g * log2(m)) on the hardware's v_log_f32 / v_exp_f32 (a dozen
// instructions) instead of libm's powf (a few hundred: with it the dense backward, memory-bound without focal, took
// twice its time).  Its error is g * |log2 m| * 2^-23 RELATIVE to m**g, i.e. at most 0.53 * 2^-23 of the largest
// value the factor takes (m**g * g * |log2 m| <= 1 / (e ln 2) on [0, 1]): below the 8 * 2^-24 floor of the tests'
// bound before it is multiplied by a BCE term and averaged.  m == 0 is torch's pow: 1 for g == 0, else 0; a negative
// base (which the convex combination above does not produce) gives nan as powf does for a fractional exponent.
__device__ __forceinline__ float focal_pow(float m, float g) {
  if (m == 0.f) return g == 0.f ? 1.f : 0.f;
  return exp2f(g * log2f(m));
}
__device__ __forceinline__ float focal_logits(float x, float t, float gamma, float alpha) {
  const float p = sigmoid_f32(x);
  const float p_t = t * p + (1.f - t) * (1.f - p);
  return bce_logits(x, t) * (t * alpha + (1.f - t) * (1.f - alpha)) * focal_pow(1.f - p_t, gamma);
}
// d focal / dx: through the BCE (p - t), and through p_t in the modulating factor (d p_t / dx = (2t - 1) p (1 - p))
__device__ __forceinline__ float focal_logits_grad(float x, float t, float gamma, float alpha) {
  const float p = sigmoid_f32(x);
  const float p_t = t * p + (1.f - t) * (1.f - p);
  const float m = 1.f - p_t;
  const float af = t * alpha + (1.f - t) * (1.f - alpha);
  const float d_m = -((t - (1.f - t)) * (p * (1.f - p)));
  return af * ((p - t) * focal_pow(m, gamma) + bce_logits(x, t) * (gamma * focal_pow(m, gamma - 1.f)) * d_m);
}

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void yolo_assign_kernel(LossArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.S * p.L) return;            // (tail lanes leave; __ballot() below only sees the lanes still here)
  const int ii = (int)i, S = (int)p.S;   // S * L < 2^31 (host)
  const int l = ii / S;
  const int s = ii - l * S;
  const int ag = s / p.G;
  const int g = s - ag * p.G;
  const int k = ag / p.A;
  const int a = ag - k * p.A;
  const LossLv& lv = p.lv[l];
  const float* b = p.gt + 4 * (size_t)g;
  const float cx = 0.5f * (b[2] + b[0]), cy = 0.5f * (b[3] + b[1]);
  const float gw = b[2] - b[0], gh = b[3] - b[1];
  const float bw = lv.base[a][2] - lv.base[a][0], bh = lv.base[a][3] - lv.base[a][1];
  float dw = gw / bw, dh = gh / bh;
  dw = fmaxf(dw, 1.f / dw);
  dh = fmaxf(dh, 1.f / dh);
  bool ok = fmaxf(dw, dh) < p.shape_thr;
  const float st = (float)lv.stride;
  const float x = cx / st, y = cy / st;
  const float ix = (float)lv.W - x, iy = (float)lv.H - y;
  float ox = 0.f, oy = 0.f;
  switch (k) {
    case 1: ok = ok && rem1(x) < 0.5f && x > 1.f; ox = -1.f; break;     // left
    case 2: ok = ok && rem1(y) < 0.5f && y > 1.f; oy = -1.f; break;     // up
    case 3: ok = ok && rem1(ix) < 0.5f && ix > 1.f; ox = 1.f; break;    // right
    case 4: ok = ok && rem1(iy) < 0.5f && iy > 1.f; oy = 1.f; break;    // down
    default: break;
  }
  const long long px = (long long)(x + ox), py = (long long)(y + oy);   // .long(): truncation
  const long long img = p.gt_img[g];
  ok = ok && px >= 0 && px < lv.W && py >= 0 && py < lv.H && img >= 0 && img < p.N;
  int anchor = -1;
  if (ok) {
    anchor = (int)((py * lv.W + px) * p.A + a);
    atomicMax(&p.winner[img * p.TA + lv.anchor_off + anchor], (int)s);
  }
  p.slot_anchor[i] = anchor;
  // positives per level: one atomic per wavefront (all of a level's positives hit the same counter)
  const int l0 = __builtin_amdgcn_readfirstlane(l);
  const unsigned long long same = __ballot(l == l0), live = __ballot(true);
  if (same == live) {
    const unsigned long long votes = __ballot(ok);
    if (votes && (int)(threadIdx.x & 63) == __ffsll((long long)live) - 1) atomicAdd(&p.npos[l0], __popcll(votes));
  } else if (ok) {
    atomicAdd(&p.npos[l], 1);
  }
}

// ---------------------------------------------------------------------------------------------------------
struct BoxTerms { float giou; float dt[4]; };      // giou: the GIoU for YV4_BOX_GIOU, the LOSS VALUE for every other kind

// decode + GIoU of one positive; with_grad: d(1 - giou)/d(box logits)
__device__ __forceinline__ BoxTerms box_terms_giou(const float t[4], const LossLv& lv, int a, int gx, int gy, const float* tg,
                                                   float eps, bool with_grad) {
  BoxTerms r;
  const float stride = (float)lv.stride;
  const float sx = (float)(gx * lv.stride), sy = (float)(gy * lv.stride);
  const float ax1 = lv.base[a][0] + sx, ay1 = lv.base[a][1] + sy, ax2 = lv.base[a][2] + sx, ay2 = lv.base[a][3] + sy;
  const float axc = (ax1 + ax2) * 0.5f, ayc = (ay1 + ay2) * 0.5f, aw = ax2 - ax1, ah = ay2 - ay1;
  float sg[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sg[j] = sigmoid_f32(t[j]);
  const float px = sg[0] * 2.f - 1.f, py = sg[1] * 2.f - 1.f;
  const float tw = sg[2] * 2.f, th = sg[3] * 2.f;
  const float xc = px * stride + axc, yc = py * stride + ayc;
  const float w = tw * tw * aw, h = th * th * ah;
  const float x1 = xc - w / 2.f, y1 = yc - h / 2.f, x2 = xc + w / 2.f, y2 = yc + h / 2.f;
  const float tx1 = tg[0], ty1 = tg[1], tx2 = tg[2], ty2 = tg[3];
  const float w1 = x2 - x1, h1 = y2 - y1;
  const float area1 = w1 * h1, area2 = (tx2 - tx1) * (ty2 - ty1);
  const float dwr = fminf(x2, tx2) - fmaxf(x1, tx1), dhr = fminf(y2, ty2) - fmaxf(y1, ty1);
  const float iw = fmaxf(dwr, 0.f), ih = fmaxf(dhr, 0.f);
  const float ov = iw * ih;
  const float Uraw = area1 + area2 - ov;
  const float U = fmaxf(Uraw, eps);
  const float ewr = fmaxf(x2, tx2) - fminf(x1, tx1), ehr = fmaxf(y2, ty2) - fminf(y1, ty1);
  const float ew = fmaxf(ewr, 0.f), eh = fmaxf(ehr, 0.f);
  const float Eraw = ew * eh;
  const float E = fmaxf(Eraw, eps);
  r.giou = ov / U - (E - U) / E;
  if (!with_grad) return r;
  // L = 1 - giou
  const float d_iou = -1.f, d_frac = 1.f;
  float d_ov = d_iou / U;
  float d_U = -d_iou * ov / (U * U) - d_frac / E;
  const float d_E = d_frac * U / (E * E);
  const float d_Uraw = d_U * (Uraw > eps ? 1.f : (Uraw == eps ? 0.5f : 0.f));
  d_ov -= d_Uraw;
  const float d_area1 = d_Uraw;
  const float d_Eraw = d_E * (Eraw > eps ? 1.f : (Eraw == eps ? 0.5f : 0.f));
  const float d_ewr = ewr >= 0.f ? d_Eraw * eh : 0.f, d_ehr = ehr >= 0.f ? d_Eraw * ew : 0.f;
  const float d_dwr = dwr >= 0.f ? d_ov * ih : 0.f, d_dhr = dhr >= 0.f ? d_ov * iw : 0.f;
  // max / min against the (constant) target: the gradient goes to the prediction where it is selected, half on a tie
  auto sel_gt = [](float a_, float b_) { return a_ > b_ ? 1.f : (a_ == b_ ? 0.5f : 0.f); };
  auto sel_lt = [](float a_, float b_) { return a_ < b_ ? 1.f : (a_ == b_ ? 0.5f : 0.f); };
  float d_x1 = -d_area1 * h1 - d_ewr * sel_lt(x1, tx1) - d_dwr * sel_gt(x1, tx1);
  float d_x2 = d_area1 * h1 + d_ewr * sel_gt(x2, tx2) + d_dwr * sel_lt(x2, tx2);
  float d_y1 = -d_area1 * w1 - d_ehr * sel_lt(y1, ty1) - d_dhr * sel_gt(y1, ty1);
  float d_y2 = d_area1 * w1 + d_ehr * sel_gt(y2, ty2) + d_dhr * sel_lt(y2, ty2);
  const float d_xc = d_x1 + d_x2, d_yc = d_y1 + d_y2;
  const float d_w = (d_x2 - d_x1) * 0.5f, d_h = (d_y2 - d_y1) * 0.5f;
  const float d_s0 = d_xc * stride * 2.f, d_s1 = d_yc * stride * 2.f;
  const float d_s2 = d_w * aw * 2.f * tw * 2.f, d_s3 = d_h * ah * 2.f * th * 2.f;
  r.dt[0] = d_s0 * sg[0] * (1.f - sg[0]);
  r.dt[1] = d_s1 * sg[1] * (1.f - sg[1]);
  r.dt[2] = d_s2 * sg[2] * (1.f - sg[2]);
  r.dt[3] = d_s3 * sg[3] * (1.f - sg[3]);
  return r;
}

// The other box losses of mmdet/models/losses/iou_loss.py:14-36,105-219, in the reference's expression order (fp32):
//   IoU     iou = ov / max(area1 + area2 - ov, 1e-6)  (the calculator's own bound), clamped below at eps;
//           loss = 1 - iou (linear) or -log(iou)
//   DIoU    iou = ov / (area1 + area2 - ov + eps);  c2 = cw^2 + ch^2 + eps  (eps ADDED, no clamp);
//           rho2 = ((tx1 + tx2) - (x1 + x2))^2 / 4 + (same in y);  loss = 1 - (iou - rho2 / c2)
//   CIoU    DIoU's terms, v = (4 / pi^2) (atan(w2 / (h2 + eps)) - atan(w1 / (h1 + eps)))^2,
//           loss = 1 - (iou - (rho2 / c2 + v^2 / (1 - iou + v))),  differentiated through v, iou AND the denominator.
//           Where the reference's expression is 0 / 0 (iou == 1 and v == 0) this one is too: nan, in the value and in
//           the gradient, exactly as there.  It is NOT special-cased.
// Subgradients are torch's: max / min against the constant target give one half on a tie, clamp(min=c) passes the
// gradient where x >= c (so also AT c), torch.max(union, 1e-6) gives one half on a tie.
template <int KIND>
__device__ __forceinline__ BoxTerms box_terms_iou(const float t[4], const LossLv& lv, int a, int gx, int gy, const float* tg,
                                                  float eps, bool with_grad) {
  BoxTerms r;
  const float stride = (float)lv.stride;
  const float sx = (float)(gx * lv.stride), sy = (float)(gy * lv.stride);
  const float ax1 = lv.base[a][0] + sx, ay1 = lv.base[a][1] + sy, ax2 = lv.base[a][2] + sx, ay2 = lv.base[a][3] + sy;
  const float axc = (ax1 + ax2) * 0.5f, ayc = (ay1 + ay2) * 0.5f, aw = ax2 - ax1, ah = ay2 - ay1;
  float sg[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sg[j] = sigmoid_f32(t[j]);
  const float px = sg[0] * 2.f - 1.f, py = sg[1] * 2.f - 1.f;
  const float tw = sg[2] * 2.f, th = sg[3] * 2.f;
  const float xc = px * stride + axc, yc = py * stride + ayc;
  const float w = tw * tw * aw, h = th * th * ah;
  const float x1 = xc - w / 2.f, y1 = yc - h / 2.f, x2 = xc + w / 2.f, y2 = yc + h / 2.f;
  const float tx1 = tg[0], ty1 = tg[1], tx2 = tg[2], ty2 = tg[3];
  const float w1 = x2 - x1, h1 = y2 - y1;
  const float area1 = w1 * h1, area2 = (tx2 - tx1) * (ty2 - ty1);
  const float dwr = fminf(x2, tx2) - fmaxf(x1, tx1), dhr = fminf(y2, ty2) - fmaxf(y1, ty1);
  const float iw = fmaxf(dwr, 0.f), ih = fmaxf(dhr, 0.f);
  const float ov = iw * ih;
  auto sel_gt = [](float a_, float b_) { return a_ > b_ ? 1.f : (a_ == b_ ? 0.5f : 0.f); };
  auto sel_lt = [](float a_, float b_) { return a_ < b_ ? 1.f : (a_ == b_ ? 0.5f : 0.f); };
  float d_x1 = 0.f, d_x2 = 0.f, d_y1 = 0.f, d_y2 = 0.f;     // what does not go through ov / area1
  float d_ov, d_area1;
  if constexpr (KIND == YV4_BOX_IOU_LINEAR || KIND == YV4_BOX_IOU_LOG) {
    const float ueps = 1e-6f;                                 // bbox_overlaps' default, not the loss's eps
    const float Uraw = area1 + area2 - ov;
    const float U = fmaxf(Uraw, ueps);
    const float iou = ov / U;
    const float ic = fmaxf(iou, eps);
    r.giou = KIND == YV4_BOX_IOU_LINEAR ? 1.f - ic : -logf(ic);
    if (!with_grad) return r;
    const float d_ic = KIND == YV4_BOX_IOU_LINEAR ? -1.f : -1.f / ic;
    const float d_iou = iou >= eps ? d_ic : 0.f;
    d_ov = d_iou / U;
    const float d_U = -d_iou * ov / (U * U);
    const float d_Uraw = d_U * (Uraw > ueps ? 1.f : (Uraw == ueps ? 0.5f : 0.f));
    d_ov -= d_Uraw;
    d_area1 = d_Uraw;
  } else {
    const float U = area1 + area2 - ov + eps;
    const float iou = ov / U;
    const float ewr = fmaxf(x2, tx2) - fminf(x1, tx1), ehr = fmaxf(y2, ty2) - fminf(y1, ty1);
    const float cw = fmaxf(ewr, 0.f), ch = fmaxf(ehr, 0.f);
    const float c2 = cw * cw + ch * ch + eps;
    const float ddx = (tx1 + tx2) - (x1 + x2), ddy = (ty1 + ty2) - (y1 + y2);
    const float rho2 = ddx * ddx / 4.f + ddy * ddy / 4.f;
    float d_iou = -1.f;
    if constexpr (KIND == YV4_BOX_DIOU) {
      r.giou = 1.f - (iou - rho2 / c2);
      if (!with_grad) return r;
    } else {
      const float h1e = h1 + eps, h2e = (ty2 - ty1) + eps;
      const float ratio = w1 / h1e;
      const float factor = 0.40528473456935109f;             // 4 / pi^2
      const float dv = atanf((tx2 - tx1) / h2e) - atanf(ratio);
      const float v = factor * (dv * dv);
      const float D = 1.f - iou + v;
      r.giou = 1.f - (iou - (rho2 / c2 + v * v / D));
      if (!with_grad) return r;
      const float q = v * v / (D * D);                        // d(v^2 / D) / dD = -q;  dD / d iou = -1
      d_iou = -1.f + q;
      const float d_v = 2.f * v / D - q;
      const float d_ratio = -(d_v * factor * 2.f * dv) / (1.f + ratio * ratio);
      const float d_w1 = d_ratio / h1e, d_h1 = -d_ratio * ratio / h1e;
      d_x2 += d_w1; d_x1 -= d_w1; d_y2 += d_h1; d_y1 -= d_h1;
    }
    d_ov = d_iou / U;
    const float d_U = -d_iou * ov / (U * U);
    d_ov -= d_U;
    d_area1 = d_U;
    const float d_c2 = -rho2 / (c2 * c2);
    const float d_ewr = ewr >= 0.f ? d_c2 * 2.f * cw : 0.f, d_ehr = ehr >= 0.f ? d_c2 * 2.f * ch : 0.f;
    const float d_ddx = ddx * 0.5f / c2, d_ddy = ddy * 0.5f / c2;
    d_x1 += -d_ewr * sel_lt(x1, tx1) - d_ddx;
    d_x2 += d_ewr * sel_gt(x2, tx2) - d_ddx;
    d_y1 += -d_ehr * sel_lt(y1, ty1) - d_ddy;
    d_y2 += d_ehr * sel_gt(y2, ty2) - d_ddy;
  }
  const float d_dwr = dwr >= 0.f ? d_ov * ih : 0.f, d_dhr = dhr >= 0.f ? d_ov * iw : 0.f;
  d_x1 += -d_area1 * h1 - d_dwr * sel_gt(x1, tx1);
  d_x2 += d_area1 * h1 + d_dwr * sel_lt(x2, tx2);
  d_y1 += -d_area1 * w1 - d_dhr * sel_gt(y1, ty1);
  d_y2 += d_area1 * w1 + d_dhr * sel_lt(y2, ty2);
  const float d_xc = d_x1 + d_x2, d_yc = d_y1 + d_y2;
  const float d_w = (d_x2 - d_x1) * 0.5f, d_h = (d_y2 - d_y1) * 0.5f;
  const float d_s0 = d_xc * stride * 2.f, d_s1 = d_yc * stride * 2.f;
  const float d_s2 = d_w * aw * 2.f * tw * 2.f, d_s3 = d_h * ah * 2.f * th * 2.f;
  r.dt[0] = d_s0 * sg[0] * (1.f - sg[0]);
  r.dt[1] = d_s1 * sg[1] * (1.f - sg[1]);
  r.dt[2] = d_s2 * sg[2] * (1.f - sg[2]);
  r.dt[3] = d_s3 * sg[3] * (1.f - sg[3]);
  return r;
}

// The family, selected at compile time: the GIoU member is the function above, untouched.
template <int KIND>
__device__ __forceinline__ BoxTerms box_terms(const float t[4], const LossLv& lv, int a, int gx, int gy, const float* tg,
                                              float eps, bool with_grad) {
  if constexpr (KIND == YV4_BOX_GIOU) return box_terms_giou(t, lv, a, gx, gy, tg, eps, with_grad);
  else return box_terms_iou<KIND>(t, lv, a, gx, gy, tg, eps, with_grad);
}

constexpr int kSlotsPerWave = 8;

// KIND: the box loss (YV4_BOX_*); CF: SoftFocalLoss on the class term
template <typename T, bool BWD, int KIND, bool CF>
__global__ __launch_bounds__(256) void yolo_pos_kernel(LossArgs p) {
  const int lane = threadIdx.x & 63;
  const int S = (int)p.S, total = S * p.L;
  const int ws0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kSlotsPerWave;
  float part_cls = 0.f, part_box = 0.f;     // forward: this wave's sums for level part_l (lane 0)
  int part_l = -1;
  for (int ws = ws0; ws < ws0 + kSlotsPerWave && ws < total; ++ws) {
  const int anchor = p.slot_anchor[ws];
  if (anchor < 0) continue;                                 // wave-uniform
  const int l = ws / S;
  const int s = ws - l * S;
  const int g = s % p.G;
  const LossLv& lv = p.lv[l];
  const int a = anchor % p.A;
  const int cell = anchor / p.A;
  const int gx = cell % lv.W, gy = cell / lv.W;
  const long long img = p.gt_img[g];
  const T* row = reinterpret_cast<const T*>(lv.raw) + ((size_t)(img * lv.H + gy) * lv.W + gx) * lv.Cp + (size_t)a * p.attr;
  const float* bias = lv.bias + a * p.attr;
  float t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = ldf(row + j) + bias[j];
  const BoxTerms bt = box_terms<KIND>(t, lv, a, gx, gy, p.gt + 4 * (size_t)g, p.eps, BWD);
  const int label = p.C > 0 ? (int)p.gt_label[g] : -1;
  const float t_on = p.smooth != 0.f ? (1.f - p.smooth) + p.smooth / (float)p.C : 1.f;
  const float t_off = p.smooth != 0.f ? p.smooth / (float)p.C : 0.f;
  if (!BWD) {
    float acc = 0.f;
    for (int c = lane; c < p.C; c += 64) {
      const float x = ldf(row + 5 + c) + bias[5 + c], tc = c == label ? t_on : t_off;
      if constexpr (CF) acc += focal_logits(x, tc, p.cls_gamma, p.cls_alpha);
      else acc += bce_logits(x, tc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
      if (l != part_l) {          // a wave's slots rarely straddle two levels: flush, then start the new level
        if (part_l >= 0) {
          if (p.C > 0) loss_sum_add(p, part_l * 3 + 0, (double)part_cls);
          loss_sum_add(p, part_l * 3 + 2, (double)part_box);
        }
        part_l = l; part_cls = 0.f; part_box = 0.f;
      }
      part_cls += acc;
      const float gl = KIND == YV4_BOX_GIOU ? 1.f - bt.giou : bt.giou;     // the box loss of the positive
      part_box += gl;
      const float q = fminf(fmaxf(1.f - gl, 0.f), 1.f);      // (1 - box_loss).clamp(0, 1)
      p.conf_t[ws] = (1.f - p.ratio) + p.ratio * q;
    }
  } else {
    const int np = p.npos[l];
    const float k_box = p.gout[l * 3 + 2] * p.w_bbox / (float)np;
    const int wslot = p.winner[img * p.TA + lv.anchor_off + anchor];
    const size_t grow0 = ((size_t)l * S + wslot) * p.attr;
    float* grow = p.gpos + grow0;
    // several positives of one anchor box add into the winner's row: float atomics in arrival order, or -- deterministic
    // mode -- integer atomics on fixed-point words (gpos is then 2 * gpos_n 64-bit words)
    u64_t* ghi = reinterpret_cast<u64_t*>(p.gpos) + grow0;
    u64_t* glo = ghi + p.gpos_n;
    if (lane < 4) {
      if (p.det) fx_add<kFxGrad>(ghi + lane, glo + lane, (double)(bt.dt[lane] * k_box));
      else atomicAdd(&grow[lane], bt.dt[lane] * k_box);
    }
    if (p.C > 0) {
      const float k_cls = p.gout[l * 3 + 0] * p.w_cls / ((float)np * (float)p.C);
      for (int c = lane; c < p.C; c += 64) {
        const float x = ldf(row + 5 + c) + bias[5 + c];
        const float tc = c == label ? t_on : t_off;
        float gv;
        if constexpr (CF) gv = focal_logits_grad(x, tc, p.cls_gamma, p.cls_alpha) * k_cls;
        else gv = (sigmoid_f32(x) - tc) * k_cls;
        if (p.det) fx_add<kFxGrad>(ghi + 5 + c, glo + 5 + c, (double)gv);
        else atomicAdd(&grow[5 + c], gv);
      }
    }
  }
  }   // slots of this wave
  if (!BWD && lane == 0 && part_l >= 0) {
    if (p.C > 0) loss_sum_add(p, part_l * 3 + 0, (double)part_cls);
    loss_sum_add(p, part_l * 3 + 2, (double)part_box);
  }
}

// ---------------------------------------------------------------------------------------------------------
template <typename T, bool FOCAL>      // FOCAL: SoftFocalLoss on the objectness term
__global__ __launch_bounds__(256) void yolo_dense_fwd_kernel(LossArgs p) {
  __shared__ double part[2 * kLossLevels];     // deterministic mode: hi words, then lo words
  if (threadIdx.x < 2 * kLossLevels) part[threadIdx.x] = 0.0;
  __syncthreads();
  u64_t* pw = reinterpret_cast<u64_t*>(part);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < p.TA * p.N) {
    const int n = fd_div((int)i, p.fd_TA);                 // N * TA < 2^31 (host)
    const int j = (int)i - n * (int)p.TA;
    int l = 0;
    while (l + 1 < p.L && j >= (int)p.lv[l + 1].anchor_off) ++l;
    const LossLv& lv = p.lv[l];
    const int jl = j - (int)lv.anchor_off;
    const int cell = fd_div(jl, p.fd_A);
    const int a = jl - cell * p.A;
    const int c = a * p.attr + 4;
    const float x = ldf(reinterpret_cast<const T*>(lv.raw) + ((size_t)n * lv.H * lv.W + cell) * lv.Cp + c) + lv.bias[c];
    const int w = p.winner[i];
    const float tgt = w >= 0 ? p.conf_t[(size_t)l * p.S + w] : 0.f;
    if constexpr (FOCAL) {
      const float e = focal_logits(x, tgt, p.conf_gamma, p.conf_alpha);
      if (p.det) fx_add<kFxStat>(pw + l, pw + kLossLevels + l, (double)e);
      else atomicAdd(&part[l], (double)e);
    } else {
      if (p.det) fx_add<kFxStat>(pw + l, pw + kLossLevels + l, (double)bce_logits(x, tgt));
      else atomicAdd(&part[l], (double)bce_logits(x, tgt));
    }
  }
  __syncthreads();
  if (p.det) {
    if (threadIdx.x < p.L) {
      u64_t* g = reinterpret_cast<u64_t*>(p.sums);
      const u64_t h = pw[threadIdx.x], lo = pw[kLossLevels + threadIdx.x];
      const int i = threadIdx.x * 3 + 1;
      if (h) atomicAdd(g + i, h);
      if (lo >> 63) atomicOr(g + 3 * p.L + i, 1ull << 63);
      if (lo & ~(1ull << 63)) atomicAdd(g + 3 * p.L + i, lo & ~(1ull << 63));
    }
    return;
  }
  if (threadIdx.x < p.L && part[threadIdx.x] != 0.0) atomicAdd(&p.sums[threadIdx.x * 3 + 1], part[threadIdx.x]);
}

template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int n = 4; };
template <> struct Chunk<_Float16> { static constexpr int n = 8; };
template <> struct Chunk<__bf16> { static constexpr int n = 8; };

template <typename T, bool FOCAL>
__global__ __launch_bounds__(256) void yolo_dense_bwd_kernel(LossArgs p) {
  constexpr int CH = Chunk<T>::n;
  extern __shared__ float db[];                      // [Cp] bias-gradient partials of the workgroup (det: [2][Cp] words)
  u64_t* dbw = reinterpret_cast<u64_t*>(db);
  int l = 0;
  while (l + 1 < p.L && (long long)blockIdx.x >= p.lv[l + 1].block0) ++l;
  const LossLv& lv = p.lv[l];
  if (p.det) for (int c = threadIdx.x; c < 2 * lv.Cp; c += 256) dbw[c] = 0;
  else for (int c = threadIdx.x; c < lv.Cp; c += 256) db[c] = 0.f;
  __syncthreads();
  const int cpr = lv.Cp / CH;
  const int rows = p.N * lv.H * lv.W;                      // rows * cpr < 2^31 (host)
  // a level's workgroups stride over its 16-byte chunks: few, long-lived workgroups keep the number of
  // same-address bias-gradient atomics at the end small (one per workgroup per channel: with one workgroup per
  // 256 chunks the three objectness channels saw 46 k serialised atomics each, 650 us of a 60 us pass)
  const int nblk = (int)((l + 1 < p.L ? p.lv[l + 1].block0 : (long long)gridDim.x) - lv.block0);
  for (int idx = (int)(((long long)blockIdx.x - lv.block0) * 256 + threadIdx.x); idx < rows * cpr; idx += nblk * 256) {
  const int row = fd_div(idx, lv.fd_cpr);
  {
    const int c0 = (idx - row * cpr) * CH;
    const int HW = lv.H * lv.W;
    const int n = fd_div(row, lv.fd_hw), cell = row - n * HW;
    const float k_conf = p.gout[l * 3 + 1] * p.w_conf / (float)((long long)p.N * HW * p.A);
    const T* src = reinterpret_cast<const T*>(lv.raw) + (size_t)row * lv.Cp;
    const int32_t* win = p.winner + (long long)n * p.TA + lv.anchor_off + (long long)cell * p.A;
    float v[CH];
    int a_cached = -1, w_cached = -1;
    // focal: the objectness channels of this chunk (c = a*attr + 4; at most two, as attr >= 5 and CH <= 8) are done HERE,
    // once per lane, and not inside the unrolled loop below, where one lane in ten meets one at a different u than its
    // neighbours and the wavefront would walk the focal derivative at nearly every u
    float fo0 = 0.f, fo1 = 0.f;
    int cf0 = -1;
    if constexpr (FOCAL) {
      const int af = c0 <= 4 ? 0 : (c0 - 4 + p.attr - 1) / p.attr;
      cf0 = af * p.attr + 4;
      if (cf0 < c0 + CH && af < p.A) {
        const int w = win[af];
        const float tgt = w >= 0 ? p.conf_t[(size_t)l * p.S + w] : 0.f;
        fo0 = focal_logits_grad(ldf(src + cf0) + lv.bias[cf0], tgt, p.conf_gamma, p.conf_alpha) * k_conf;
      }
      const int cf1 = cf0 + p.attr;
      if (cf1 < c0 + CH && af + 1 < p.A) {
        const int w = win[af + 1];
        const float tgt = w >= 0 ? p.conf_t[(size_t)l * p.S + w] : 0.f;
        fo1 = focal_logits_grad(ldf(src + cf1) + lv.bias[cf1], tgt, p.conf_gamma, p.conf_alpha) * k_conf;
      }
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int c = c0 + u;
      v[u] = 0.f;
      if (c >= p.A * p.attr) continue;
      const int a = c / p.attr, j = c - a * p.attr;
      if (a != a_cached) { a_cached = a; w_cached = win[a]; }
      if (FOCAL && j == 4) {
        v[u] = c == cf0 ? fo0 : fo1;
      } else if (j == 4) {
        const float x = ldf(src + c) + lv.bias[c];
        const float tgt = w_cached >= 0 ? p.conf_t[(size_t)l * p.S + w_cached] : 0.f;
        v[u] = (sigmoid_f32(x) - tgt) * k_conf;
      } else if (w_cached >= 0) {
        const size_t gi = ((size_t)l * p.S + w_cached) * p.attr + j;
        if (p.det) {
          const u64_t* gw = reinterpret_cast<const u64_t*>(p.gpos);
          v[u] = (float)fx_value<kFxGrad>(gw[gi], gw[p.gpos_n + gi]);
        } else {
          v[u] = p.gpos[gi];
        }
      }
      if (v[u] != 0.f) {
        if (p.det) fx_add<kFxGrad>(dbw + c, dbw + lv.Cp + c, (double)v[u]);
        else atomicAdd(&db[c], v[u]);
      }
    }
    T* dst = reinterpret_cast<T*>(lv.draw) + (size_t)row * lv.Cp + c0;
    alignas(16) T o[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) o[u] = (T)v[u];
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
  }
  }   // chunks of this workgroup
  __syncthreads();
  if (p.det) {        // dbias: [hi (A*attr) | lo (A*attr)] words, decoded in place after the launch
    u64_t* g = reinterpret_cast<u64_t*>(lv.dbias);
    const int nb = p.A * p.attr;
    for (int c = threadIdx.x; c < nb; c += 256) {
      const u64_t h = dbw[c], lo = dbw[lv.Cp + c];
      if (h) atomicAdd(g + c, h);
      if (lo >> 63) atomicOr(g + nb + c, 1ull << 63);
      if (lo & ~(1ull << 63)) atomicAdd(g + nb + c, lo & ~(1ull << 63));
    }
    return;
  }
  for (int c = threadIdx.x; c < p.A * p.attr; c += 256)
    if (db[c] != 0.f) atomicAdd(&lv.dbias[c], (double)db[c]);
}

static int fill_args(const yv4_loss_desc* d, const yv4_loss_opts* o, LossArgs& a, const char* who) {
  YV4_REQUIRE(d, "%s: null descriptor", who);
  YV4_REQUIRE(o, "%s: null options", who);
  YV4_REQUIRE(o->box_kind >= YV4_BOX_GIOU && o->box_kind <= YV4_BOX_CIOU, "%s: unknown box_kind %d", who, o->box_kind);
  // (written so that a nan fails them)
  YV4_REQUIRE(!o->conf_focal || (o->conf_gamma >= 1.f && o->conf_alpha >= 0.f && o->conf_alpha <= 1.f),
              "%s: conf focal needs gamma >= 1 and alpha in [0, 1] (gamma %g, alpha %g)", who, (double)o->conf_gamma, (double)o->conf_alpha);
  YV4_REQUIRE(!o->cls_focal || (o->cls_gamma >= 1.f && o->cls_alpha >= 0.f && o->cls_alpha <= 1.f),
              "%s: cls focal needs gamma >= 1 and alpha in [0, 1] (gamma %g, alpha %g)", who, (double)o->cls_gamma, (double)o->cls_alpha);
  YV4_REQUIRE(d->num_levels >= 1 && d->num_levels <= kLossLevels, "%s: 1..%d levels", who, kLossLevels);
  YV4_REQUIRE(d->N > 0 && d->A >= 1 && d->A <= 8 && d->num_classes >= 0 && d->G >= 0, "%s: bad sizes", who);
  YV4_REQUIRE(d->dtype == YV4_F32 || d->dtype == YV4_F16 || d->dtype == YV4_BF16, "%s: dtype must be f32, f16 or bf16", who);
  YV4_REQUIRE(d->winner && d->npos && d->sums, "%s: work buffers missing", who);
  YV4_REQUIRE(d->G == 0 || (d->gt && d->gt_img && d->slot_anchor && d->conf_t && (d->num_classes == 0 || d->gt_label)),
              "%s: ground-truth tables missing", who);
  a = LossArgs{};
  a.L = d->num_levels; a.N = d->N; a.A = d->A; a.C = d->num_classes; a.attr = 5 + d->num_classes; a.G = d->G;
  a.S = 5LL * d->A * d->G;
  const int ch = d->dtype == YV4_F32 ? 4 : 8;
  long long off = 0;
  for (int l = 0; l < a.L; ++l) {
    const yv4_loss_level& s = d->levels[l];
    YV4_REQUIRE(s.raw && s.bias && s.H > 0 && s.W > 0 && s.stride > 0, "%s: level %d incomplete", who, l);
    YV4_REQUIRE(s.Cp % ch == 0 && s.Cp >= a.A * a.attr, "%s: level %d: pixel stride %d must be a multiple of %d and hold %d channels",
                who, l, s.Cp, ch, a.A * a.attr);
    YV4_REQUIRE(((uintptr_t)s.raw & 15) == 0, "%s: level %d: map must be 16-byte aligned", who, l);
    LossLv& t = a.lv[l];
    t.raw = s.raw; t.draw = s.draw; t.bias = s.bias; t.dbias = s.dbias;
    t.H = s.H; t.W = s.W; t.Cp = s.Cp; t.stride = s.stride;
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < 4; ++c) t.base[k][c] = s.base_anchors[k][c];
    t.anchor_off = off;
    off += (long long)s.H * s.W * a.A;
    t.fd_hw = make_fastdiv((unsigned)(s.H * s.W));
    t.fd_cpr = make_fastdiv((unsigned)(s.Cp / ch));
    // the dense backward walks 16-byte chunks with a 32-bit index that advances by up to 2048 * 256 per iteration
    YV4_REQUIRE((long long)d->N * s.H * s.W * (s.Cp / ch) < (1LL << 31) - 2048LL * 256, "%s: level %d: map too large", who, l);
  }
  a.TA = off;
  a.fd_TA = make_fastdiv((unsigned)off);
  a.fd_A = make_fastdiv((unsigned)a.A);
  YV4_REQUIRE(a.TA * a.N < (1LL << 31) && a.S * a.L < (1LL << 31), "%s: index space exceeds 31 bits", who);
  a.gt = d->gt; a.gt_label = d->gt_label; a.gt_img = d->gt_img;
  a.shape_thr = d->shape_thr; a.smooth = d->smooth; a.ratio = d->ratio; a.eps = d->eps;
  a.w_cls = d->w_cls; a.w_conf = d->w_conf; a.w_bbox = d->w_bbox;
  a.slot_anchor = d->slot_anchor; a.winner = d->winner; a.npos = d->npos; a.conf_t = d->conf_t; a.gpos = d->gpos;
  a.sums = d->sums;
  a.losses = d->losses;
  a.box_kind = o->box_kind;
  a.conf_gamma = o->conf_gamma; a.conf_alpha = o->conf_alpha; a.cls_gamma = o->cls_gamma; a.cls_alpha = o->cls_alpha;
  a.det = deterministic() ? 1 : 0;
  a.gpos_n = a.S * a.L * a.attr;
  return YV4_OK;
}

#define YV4_LOSS_DISPATCH(dtype, ...)                                   \
  do {                                                                  \
    if ((dtype) == YV4_F32) { using T = float; __VA_ARGS__; }           \
    else if ((dtype) == YV4_F16) { using T = _Float16; __VA_ARGS__; }   \
    else { using T = __bf16; __VA_ARGS__; }                             \
  } while (0)

// + the box kind and the class term's focal switch of yolo_pos_kernel
#define YV4_LOSS_KIND_CASE(K, cf, ...)                                                      \
  case K:                                                                                   \
    if (cf) { constexpr int KIND = K; constexpr bool CF = true; __VA_ARGS__; }              \
    else { constexpr int KIND = K; constexpr bool CF = false; __VA_ARGS__; }                \
    break;
#define YV4_LOSS_POS_DISPATCH(dtype, kind, cf, ...)                     \
  YV4_LOSS_DISPATCH(dtype, switch (kind) {                              \
    YV4_LOSS_KIND_CASE(YV4_BOX_GIOU, cf, __VA_ARGS__)                   \
    YV4_LOSS_KIND_CASE(YV4_BOX_IOU_LINEAR, cf, __VA_ARGS__)             \
    YV4_LOSS_KIND_CASE(YV4_BOX_IOU_LOG, cf, __VA_ARGS__)                \
    YV4_LOSS_KIND_CASE(YV4_BOX_DIOU, cf, __VA_ARGS__)                   \
    YV4_LOSS_KIND_CASE(YV4_BOX_CIOU, cf, __VA_ARGS__)                   \
    default: break;                                                     \
  })

static const yv4_loss_opts kDefaultLossOpts = {YV4_BOX_GIOU, 0, 0.f, 0.f, 0, 0.f, 0.f, {0}};

}  // namespace yv4

using namespace yv4;

extern "C" int yv4_yolo_loss_fwd(const yv4_loss_desc* d, void* stream) {
  return yv4_yolo_loss_fwd_ex(d, &kDefaultLossOpts, stream);
}

extern "C" int yv4_yolo_loss_bwd(const yv4_loss_desc* d, const float* grad_out, void* stream) {
  return yv4_yolo_loss_bwd_ex(d, &kDefaultLossOpts, grad_out, stream);
}

extern "C" int yv4_yolo_loss_fwd_ex(const yv4_loss_desc* d, const yv4_loss_opts* o, void* stream) {
  LossArgs a;
  if (int rc = fill_args(d, o, a, "yolo_loss_fwd")) return rc;
  const bool cf = o->cls_focal != 0, ff = o->conf_focal != 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  bool ok = hipMemsetAsync(a.winner, 0xFF, sizeof(int32_t) * a.TA * a.N, s) == hipSuccess;
  ok = ok && hipMemsetAsync(a.npos, 0, sizeof(int32_t) * a.L, s) == hipSuccess;
  ok = ok && hipMemsetAsync(a.sums, 0, sizeof(double) * (a.det ? 6 : 3) * a.L, s) == hipSuccess;
  if (!ok) { set_error("yolo_loss_fwd: memset failed"); return YV4_E_LAUNCH; }
  const long long slots = a.S * a.L;
  if (slots > 0) {
    hipLaunchKernelGGL(yolo_assign_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a);
    YV4_LOSS_POS_DISPATCH(d->dtype, a.box_kind, cf,
                          hipLaunchKernelGGL((yolo_pos_kernel<T, false, KIND, CF>),
                                             dim3((unsigned)((slots + 4 * kSlotsPerWave - 1) / (4 * kSlotsPerWave))), dim3(256), 0, s, a));
  }
  const long long boxes = a.TA * a.N;
  if (ff)
    YV4_LOSS_DISPATCH(d->dtype, hipLaunchKernelGGL((yolo_dense_fwd_kernel<T, true>), dim3((unsigned)((boxes + 255) / 256)), dim3(256), 0,
                                                   s, a));
  else
    YV4_LOSS_DISPATCH(d->dtype, hipLaunchKernelGGL((yolo_dense_fwd_kernel<T, false>), dim3((unsigned)((boxes + 255) / 256)), dim3(256), 0,
                                                   s, a));
  if (a.det) hipLaunchKernelGGL(loss_fx_decode_kernel<kFxStat>, dim3(1), dim3(256), 0, s, a.sums, 3 * a.L);
  if (a.losses) hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, s, a);
  YV4_CHECK_LAUNCH("yolo_loss_fwd");
  return YV4_OK;
}

extern "C" int yv4_yolo_loss_bwd_ex(const yv4_loss_desc* d, const yv4_loss_opts* o, const float* grad_out, void* stream) {
  LossArgs a;
  if (int rc = fill_args(d, o, a, "yolo_loss_bwd")) return rc;
  const bool cf = o->cls_focal != 0, ff = o->conf_focal != 0;
  YV4_REQUIRE(grad_out, "yolo_loss_bwd: grad_out missing");
  YV4_REQUIRE(a.S == 0 || a.gpos, "yolo_loss_bwd: gpos missing");
  a.gout = grad_out;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ch = d->dtype == YV4_F32 ? 4 : 8;
  long long blocks = 0;
  int max_cp = 0;
  bool ok = true;
  for (int l = 0; l < a.L; ++l) {
    YV4_REQUIRE(a.lv[l].draw && a.lv[l].dbias, "yolo_loss_bwd: level %d: draw / dbias missing", l);
    YV4_REQUIRE(((uintptr_t)a.lv[l].draw & 15) == 0, "yolo_loss_bwd: level %d: draw must be 16-byte aligned", l);
    a.lv[l].block0 = blocks;
    const long long chunks = (long long)a.N * a.lv[l].H * a.lv[l].W * (a.lv[l].Cp / ch);
    long long nb = (chunks + 255) / 256;
    if (nb > 2048) nb = 2048;
    blocks += nb;
    if (a.lv[l].Cp > max_cp) max_cp = a.lv[l].Cp;
    ok = ok && hipMemsetAsync(a.lv[l].dbias, 0, sizeof(double) * (a.det ? 2 : 1) * a.A * a.attr, s) == hipSuccess;
  }
  const long long slots = a.S * a.L;
  if (slots > 0) ok = ok && hipMemsetAsync(a.gpos, 0, (a.det ? 16 : sizeof(float)) * slots * a.attr, s) == hipSuccess;
  if (!ok) { set_error("yolo_loss_bwd: memset failed"); return YV4_E_LAUNCH; }
  YV4_REQUIRE(blocks < (1LL << 31), "yolo_loss_bwd: too many workgroups");
  if (slots > 0)
    YV4_LOSS_POS_DISPATCH(d->dtype, a.box_kind, cf,
                          hipLaunchKernelGGL((yolo_pos_kernel<T, true, KIND, CF>),
                                             dim3((unsigned)((slots + 4 * kSlotsPerWave - 1) / (4 * kSlotsPerWave))), dim3(256), 0, s, a));
  if (ff)
    YV4_LOSS_DISPATCH(d->dtype, hipLaunchKernelGGL((yolo_dense_bwd_kernel<T, true>), dim3((unsigned)blocks), dim3(256),
                                                   (a.det ? 16 : sizeof(float)) * max_cp, s, a));
  else
    YV4_LOSS_DISPATCH(d->dtype, hipLaunchKernelGGL((yolo_dense_bwd_kernel<T, false>), dim3((unsigned)blocks), dim3(256),
                                                   (a.det ? 16 : sizeof(float)) * max_cp, s, a));
  if (a.det)
    for (int l = 0; l < a.L; ++l)
      hipLaunchKernelGGL(loss_fx_decode_kernel<kFxGrad>, dim3((a.A * a.attr + 255) / 256), dim3(256), 0, s, a.lv[l].dbias,
                         a.A * a.attr);
  YV4_CHECK_LAUNCH("yolo_loss_bwd");
  return YV4_OK;
}
