/*
 * yv4.h -- C-ABI of libyv4_hip.so: the MI355X (gfx950) YOLOv4 hot path.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain
 * device pointers + sizes + a hipStream_t passed as void*, allocates nothing,
 * never synchronises the host, and returns 0 on success or a negative YV4_E_*
 * code (yv4_last_error() holds the message of the last failure on the calling
 * thread).  No torch types cross this boundary.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   yv4_mish_fwd / yv4_mish_bwd   mmdet/ops/mish_cuda/src/mish.cc:14-39
 *                                 (pybind mish_forward / mish_backward),
 *                                 math mmdet/ops/mish_cuda/src/mish.h:16-29,
 *                                 kernels src/kernel/mish_cuda.cu:25-71
 *   yv4_conv_bn_act_fwd           mmcv ConvModule as used by
 *                                 mmdet/models/backbones/darknetcsp.py:15-35
 *                                 (Conv2d -> BN(eval) -> act), residual add of
 *                                 darknetcsp.py:60-64, CSP-level cat->BN->act of
 *                                 darknetcsp.py:106-109,149-153,220-229 and the
 *                                 biased head conv yolocsp_head.py:180-185
 *   yv4_spp_pool_fwd              darknetcsp.py:176-181,203-206,222-226
 *                                 (MaxPool2d k=5,9,13 s=1 + cat)
 *   yv4_resample_nearest_fwd      necks/yolo_neck_csp.py:213-219,229
 *                                 (F.interpolate nearest + torch.cat)
 *   yv4_decode_filter             dense_heads/yolocsp_head.py:255-294,357-372,
 *                                 core/bbox/coder/yolov4_bbox_coder.py:39-67,
 *                                 core/anchor/anchor_generator.py:207-270,
 *                                 core/post_processing/bbox_nms.py:36-67
 *   yv4_nms_images / yv4_nms_prepare
 *                                 mmcv.ops.nms.batched_nms called at
 *                                 core/post_processing/bbox_nms.py:84-88
 *   yv4_nchw_to_nhwc / yv4_nhwc_to_nchw
 *                                 layout adaptors at the module boundary (the
 *                                 reference is NCHW, yolocsp_head.py:264 permutes)
 */
#ifndef YV4_H_
#define YV4_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YV4_ABI_VERSION 8

/* error codes */
#define YV4_OK 0
#define YV4_E_INVALID (-1)   /* bad argument (null pointer, bad shape, bad enum) */
#define YV4_E_UNSUPPORTED (-2) /* valid request this build has no kernel for */
#define YV4_E_LAUNCH (-3)    /* hipLaunch / hip runtime error */
#define YV4_E_CAPACITY (-4)  /* caller-provided workspace too small */

/* element types of the standalone activation op */
#define YV4_F32 0
#define YV4_F16 1
#define YV4_BF16 2
#define YV4_F64 3
/* element type of the fp8 inference plans' activations and weights (OCP e4m3fn, max 448; the fp8 entry points below
 * take it where the other entry points take YV4_F16 / YV4_BF16; the standalone activation op has no fp8 form) */
#define YV4_F8E4M3 3

/* activations of the fused conv epilogue (Mish everywhere in v4/v5,
 * LeakyReLU(slope) in the v3 path, Swish when a config overrides act_cfg) */
#define YV4_ACT_NONE 0
#define YV4_ACT_MISH 1
#define YV4_ACT_LEAKY 2
#define YV4_ACT_SWISH 3

int yv4_abi_version(void);
const char* yv4_last_error(void);
/* Name of the gfx target the kernels were compiled for ("gfx950"). */
const char* yv4_arch(void);

/* ---- Mish (standalone op; on the fast path Mish is a conv epilogue) -------
 * out[i] = x*tanh(x < 20 ? log1p(exp(x)) : x);   n elements, contiguous.
 * bwd: gin = gout * (x*(1-tsp^2)*(1-exp(-sp)) + tsp), from the saved INPUT. */
int yv4_mish_fwd(const void* in, void* out, size_t n, int dtype, void* stream);
int yv4_mish_bwd(const void* gout, const void* in, void* gin, size_t n,
                 int dtype, void* stream);
/* The same op on HOST memory (ABI 6): mish.cc:14-33 dispatches on input.is_cuda() and a CPU tensor runs
 * mish_cpu_kernel's loop (src/kernel/mish_cpu.cc:6-29) over mish.h:16-29 -- float and double only (Half / BFloat16 are
 * not dispatched there: YV4_E_UNSUPPORTED), the float forward evaluated in double as that build does.  Plain
 * single-threaded loops over libm.  Not on any plan's or train step's path -- the op's CPU behaviour, nothing else. */
int yv4_mish_fwd_host(const void* in, void* out, size_t n, int dtype);
int yv4_mish_bwd_host(const void* gout, const void* in, void* gin, size_t n, int dtype);

/* ---- layout adaptors -------------------------------------------------------
 * src NCHW (N,C,H,W) contiguous fp32 -> dst NHWC with `dst_cstride` channels per
 * pixel, written at channel offset dst_coff; channels [C, C+zero_pad) are zeroed
 * (the stem pads Cin 3 -> 4). */
int yv4_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W,
                     int dst_cstride, int dst_coff, int zero_pad, void* stream);
int yv4_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W,
                     int src_cstride, int src_coff, void* stream);

/* ---- fused conv ------------------------------------------------------------
 * Implicit-GEMM convolution on fp32 MFMA, NHWC activations:
 *   acc[m][co] = sum_{kh,kw,ci} x[n, ho*stride-pad+kh, wo*stride-pad+kw, ci]
 *                               * w[co][(kh*KW+kw)*Cin + ci]
 *   v = acc*scale1[co] + shift1[co];  v = act1(v);
 *   if (residual) v += residual[m][co];
 *   if (scale2)   v = act2(v*scale2[co] + shift2[co]);
 *   y[m*y_cstride + y_coff + co] = v
 * scale1/shift1 carry the folded eval-mode BN (or 1 / bias for a bare or biased
 * conv); scale2/shift2 carry the CSP-level BN applied to the concat half this
 * conv produces.  x / residual / y are channel-strided views so that producers
 * write straight into concat buffers (torch.cat disappears). Cin % 4 == 0,
 * x_cstride % 4 == 0, x_coff % 4 == 0 are required (16-byte loads). */
typedef struct yv4_conv_desc {
  int32_t N, H, W, Cin;      /* input  */
  int32_t Ho, Wo, Cout;      /* output */
  int32_t KH, KW, stride, pad;
  int32_t x_cstride, x_coff; /* floats per input pixel / channel offset  */
  int32_t y_cstride, y_coff;
  int32_t r_cstride, r_coff; /* residual view (ignored when residual==NULL) */
  int32_t act1, act2;        /* YV4_ACT_* */
  float slope1, slope2;      /* LeakyReLU negative slopes */
  int32_t tile;              /* 0 = auto; else a YV4_TILE_* id (benchmarking) */
  int32_t flags;             /* ABI 7: YV4_CONV_* bits, 0 = none (appended: an ABI-6 caller's struct is a prefix) */
} yv4_conv_desc;

/* flags: the output is written with NON-TEMPORAL stores (the lines are not kept in the XCD's L2).  A per-plan choice:
 * inference plans of the 16-bit wide-tile kernels gain 0.6-1.3 % with it (their outputs are next read by a kernel that
 * streams them once), training loses 0.2-0.7 % (the BatchNorm pass right behind a conv re-reads its output from the
 * cache), the fp32 wide kernels lose 2.8 % (DESIGN, non-temporal stores).  Same bits either way; kernels without a
 * non-temporal form ignore the flag. */
#define YV4_CONV_NT_OUT 1

#define YV4_TILE_AUTO 0
#define YV4_TILE_128x128 1
#define YV4_TILE_128x64 2
#define YV4_TILE_64x64 3
#define YV4_TILE_64x128 4
/* LDS-DMA kernels (need Cin % 32 == 0 and tensors below 4 GiB) */
#define YV4_TILE_DMA_64x64 5
#define YV4_TILE_DMA_128x64 6
#define YV4_TILE_DMA_128x128 7
/* register-only kernel for the 3x3/s1/p1 stem (Cin padded to 4, Cout <= 64) */
#define YV4_TILE_STEM 8
/* 1x1 / stride 1, Cin 64 / 128 / 256, Cout >= 32, no residual: one persistent 8-wave workgroup per CU, the weight slab
 * resident in LDS, wave-private rings of 32-pixel strips; same summation order as the DMA tiles (bit-identical) */
#define YV4_TILE_WS_1x1 9
/* fp32 3x3 / stride 1 / pad 1 with Cin % 32 == 0 and Cout % 16 == 0 on WIDE wave tiles (16 PT pixels x 64 channels per
 * wave on v_mfma_f32_16x16x4_f32, one accumulator set; the fp32 form of YV4_HTILE_W3x3: csrc/conv3x3_wide_f32.hip).
 * NOT bit-identical to the 32x32x2 tiles (the K sum is grouped differently); YV4_TILE_W3x3_SHAPE(i), i = 0..4 (256 x 256,
 * 192 x 256, 128 x 256, 384 x 128, 256 x 128), pins the workgroup tile shape -- yv4_conv_pick_tile returns that form, so a
 * plan that must reproduce another plan's bits can copy its tile ids. */
#define YV4_TILE_W3x3 10
#define YV4_TILE_W3x3_SHAPE(i) (10 + 16 * ((i) + 1))
/* fp32 GENERAL convolution on the same wide wave tiles (csrc/conv_wide_f32.hip, the fp32 form of YV4_HTILE_WIDE): any
 * kernel / stride / padding with Cin % 32 == 0, Cout % 16 == 0 (64 .. 2048), 4-aligned channel strides / offsets; the
 * automatic choice gives it the stride-2 3x3 layers and the deep 1x1 layers.  Not bit-identical to the 32x32x2 tiles;
 * YV4_TILE_WIDE_SHAPE(i) pins the workgroup tile shape as above and is what yv4_conv_pick_tile reports. */
#define YV4_TILE_WIDE 11
#define YV4_TILE_WIDE_SHAPE(i) (11 + 16 * ((i) + 1))
/* (round 2's fp32 ping-pong 3x3 form, removed in round 3 -- DESIGN 9.12 -- used to own id 10; the id now names the wide
 * 3x3 kernel above and is accepted and chosen automatically) */

int yv4_conv_bn_act_fwd(const yv4_conv_desc* d, const float* x, const float* w,
                        const float* scale1, const float* shift1,
                        const float* scale2, const float* shift2,
                        const float* residual, float* y, void* stream);
/* Algorithmic work of one launch, for the roofline: 2*M*Cout*K flops. */
double yv4_conv_flops(const yv4_conv_desc* d);
/* Tile id the auto heuristic picks for d (so callers can report it). */
int yv4_conv_pick_tile(const yv4_conv_desc* d);

/* ---- SPP -------------------------------------------------------------------
 * buf is an NHWC view with `cstride` channels per pixel.  Reads channels
 * [coff, coff+C) and writes MaxPool2d(k, stride 1, pad k/2) for k = 5, 9, 13 to
 * [coff+C, coff+2C), [coff+2C, coff+3C), [coff+3C, coff+4C) -- i.e. the
 * torch.cat([x, mp5, mp9, mp13], 1) buffer is completed in place. C % 4 == 0. */
int yv4_spp_pool_fwd(float* buf, int N, int H, int W, int C, int cstride,
                     int coff, void* stream);

/* ---- nearest resample into a concat buffer ---------------------------------
 * dst[n, y, x, dst_coff + c] = src[n, sy(y), sx(x), src_coff + c] with
 * sy = min(floor(y * Hs / Hd), Hs-1) (torch 'nearest').  Hs==Hd is a plain
 * channel-slice copy. C % 4 == 0. */
int yv4_resample_nearest_fwd(const float* src, float* dst, int N, int Hs, int Ws,
                             int Hd, int Wd, int C, int src_cstride,
                             int src_coff, int dst_cstride, int dst_coff,
                             void* stream);

/* ---- decode + threshold ----------------------------------------------------
 * One call handles every level of a batch.  Level l's pred map is NHWC
 * (N, H_l, W_l, A*(5+num_classes)) fp32.  For anchor-box index
 * j = level_base_l + (y*W_l + x)*A + a of image n:
 *   s = sigmoid(p);  cx = (2 s0 - 1)*stride + x*stride + stride/2 ... (the
 *   reference's literal op order, see csrc/postproc.hip)
 *   boxes[n][j] = decoded box / scale_factor[n]   (if scale_factor != NULL)
 *   conf[n][j]  = s4
 *   for each class c with s_{5+c}*s4 > score_thr: append the candidate key
 *       (~bits(score) << 32 | (j*num_classes + c)) to keys[n*key_cap + ...],
 *       and fold the box into max_coord[n] (the per-image boxes.max()).
 * num_classes == 0 is the class-agnostic head (yolocsp_head.py:155-178,357-360:
 * 5 attributes per box, one score column = conf, flat index = j).
 * topk_keys (N device values from yv4_conf_topk, or NULL) implements `nms_pre`
 * (yolocsp_head.py:349-355): boxes whose (conf, index) key ranks behind the
 * image's k-th are decoded but produce no candidates.
 * counts[n] / max_coord[n] must be zero / -inf-initialised by
 * yv4_decode_reset().  If more than key_cap candidates pass for an image the
 * count keeps counting (so the caller can see the overflow) but keys beyond the
 * capacity are dropped.  cls rows are written for the boxes that are admitted
 * as candidates' sources only: the rows of boxes turned away by nms_pre (or, in
 * yv4_decode_filter_v3, by conf_thr) are left unwritten; boxes and conf are
 * written for every box. */
typedef struct yv4_level_desc {
  const float* pred;  /* device pointer, NHWC */
  int32_t H, W;
  int32_t stride;     /* featmap stride in pixels (8/16/32) */
  /* base anchors (x1,y1,x2,y2) of one grid cell, A <= 8 rows, exactly as
   * YOLOAnchorGenerator.gen_single_level_base_anchors builds them
   * (core/anchor/anchor_generator.py:639-665): centre stride/2, float32 */
  float base_anchors[8][4];
} yv4_level_desc;

int yv4_decode_reset(int32_t* counts, float* max_coord, int N, void* stream);
int yv4_decode_filter(const yv4_level_desc* levels, int num_levels, int N, int A,
                      int num_classes, float score_thr,
                      const float* scale_factor /* (N,4) device or NULL */,
                      float* boxes /* (N, total_anchors, 4) */,
                      float* conf /* (N, total_anchors) or NULL */,
                      float* cls /* (N, total_anchors, num_classes) sigmoid, or NULL */,
                      uint64_t* keys, int64_t key_cap, int32_t* counts,
                      float* max_coord, const uint64_t* topk_keys /* (N) or NULL */,
                      void* stream);

/* nms_pre pre-selection: topk_keys[n] = the k-th smallest key
 * (~order(conf) << 32 | anchor index) of image n, i.e. the admission threshold of
 * `conf_pred.topk(k)` with ties broken towards the lower anchor index.  Requires
 * 0 < k < anchors per image (the reference applies top-k only then).  work:
 * yv4_conf_topk_work(N, anchors per image) bytes of device memory. */
size_t yv4_conf_topk_work(int N, int64_t total_anchors);
int yv4_conf_topk(const yv4_level_desc* levels, int num_levels, int N, int A,
                  int num_classes, int k, void* work, uint64_t* topk_keys,
                  void* stream);

/* ---- YOLOv3 head (mmdet/models/dense_heads/yolo_head.py:210-391) ----------------------
 * Same buffers and key format as yv4_decode_filter, YOLOV3Head semantics:
 *   box: cx = (sigmoid(t0) - 0.5)*stride + anchor_cx, w = exp(t2)*anchor_w
 *        (core/bbox/coder/yolo_bbox_coder.py:61-89);
 *   candidates: boxes inside their LEVEL's top-k by objectness (topk_keys_per_level: N*num_levels
 *   values from yv4_conf_topk_levels, or NULL), with objectness >= conf_thr (<= 0: off), classes with
 *   sigmoid(cls) > score_thr; the key carries cls*objectness (multiclass_nms' score_factors,
 *   core/post_processing/bbox_nms.py:52-62).  NMS itself is yv4_nms_images / yv4_nms_split. */
int yv4_decode_filter_v3(const yv4_level_desc* levels, int num_levels, int N, int A,
                         int num_classes, float score_thr, float conf_thr,
                         const float* scale_factor, float* boxes, float* conf, float* cls,
                         uint64_t* keys, int64_t key_cap, int32_t* counts, float* max_coord,
                         const uint64_t* topk_keys_per_level, void* stream);
/* Per-level top-k thresholds: topk_keys[n*num_levels + l] = k-th key of level l of image n, or the
 * all-admitting key when the level has <= k boxes (core/export/onnx_helper.py:45-78). */
size_t yv4_conf_topk_levels_work(int N, int64_t total_anchors, int num_levels);
int yv4_conf_topk_levels(const yv4_level_desc* levels, int num_levels, int N, int A,
                         int num_classes, int k, void* work, uint64_t* topk_keys, void* stream);

/* ---- batched NMS -----------------------------------------------------------
 * Per image n (one workgroup each): sort its counts[n] candidate keys by
 * (score desc, flat index asc), then greedy NMS in that order on the
 * class-offset boxes  box + label*(max_coord[n] + 1)  (mmcv batched_nms
 * semantics), suppressing j when inter/(area_i + area_j - inter) > iou_thr
 * (fp32, IEEE division).  Stops after max_out survivors (multiclass_nms
 * `max_num`).  A candidate's box is boxes[n][flat / fused_classes] and its
 * label flat % fused_classes; with fused_classes == 0 the box is
 * boxes[n][flat] and the label labels[n*label_stride + flat] (the standalone
 * batched_nms op).
 * Outputs per image: out_dets (max_out,5) = x1,y1,x2,y2,score (un-offset
 * boxes), out_labels (max_out) int32, out_index (max_out) int64 = flat index of
 * each survivor, out_count.  Images with counts[n] >= split_thr (mmcv
 * `split_thr`, 10000) or > key_cap take mmcv's per-class path: they are only
 * flagged here (out_count[n] = -1) and must go through yv4_nms_split. */
int yv4_nms_images(uint64_t* keys /* sorted in place */, int64_t key_cap, const int32_t* counts,
                   const float* max_coord, const float* boxes,
                   int64_t boxes_per_image, const int32_t* labels,
                   int64_t label_stride, int fused_classes, int N,
                   float iou_thr, int max_out, int split_thr, float* out_dets,
                   int32_t* out_labels, int64_t* out_index, int32_t* out_count,
                   void* stream);

/* mmcv's n >= split_thr path for ONE image: per-class NMS, survivors re-sorted
 * by (score desc, flat index asc), first max_out returned.  `keys` holds that
 * image's n candidate keys (any order); work must hold yv4_nms_split_work(n)
 * bytes.  n is a host value: the caller reads counts[] back first (the
 * reference syncs at the same place, bbox_nms.py:66). */
size_t yv4_nms_split_work(int64_t n);
int yv4_nms_split(const uint64_t* keys, int64_t n, float max_coord,
                  const float* boxes, const int32_t* labels, int fused_classes,
                  float iou_thr, int max_out, void* work, float* out_dets,
                  int32_t* out_labels, int64_t* out_index, int32_t* out_count,
                  void* stream);

/* The suppression predicate of every NMS entry point, process-wide (set it once, before launching):
 *   YV4_NMS_IOU_DIV (default)  inter / (Sa + Sb - inter) > iou_thr    -- mmcv-full 1.3.x's CPU kernel (nms_cpu) and
 *                                                                        the definition SURVEY 8c fixes; oracle/nms_ref.c
 *   YV4_NMS_IOU_MUL            inter > iou_thr * (Sa + Sb - inter)    -- mmcv-full 1.3.x's CUDA kernel (devIoU), i.e.
 *                                                                        what the reference executes on a GPU
 * Both in fp32 without contraction; they select differently only on pairs whose IoU rounds across iou_thr
 * (tests/golden/nms_boundary.npz).  mmcv is third party and absent from the reference tree (call site
 * mmdet/core/post_processing/bbox_nms.py:84): parity unpinned against either kernel.
 * Returns YV4_OK / YV4_E_ARG. */
#define YV4_NMS_IOU_DIV 0
#define YV4_NMS_IOU_MUL 1
int yv4_nms_set_iou_form(int form);
int yv4_nms_get_iou_form(void);

/* ---- soft-NMS (csrc/soft_nms.hip; additive within ABI 8) ---------------------------------------------------------------
 * mmcv-full 1.3.x soft_nms(boxes, scores, iou_threshold, sigma, min_score, method, offset=0) (mmcv's softnms_cpu; the
 * reference reaches it through batched_nms(nms_cfg type='soft_nms'), core/post_processing/bbox_nms.py:84).  mmcv is third
 * party and absent; this is the definition the library implements.  One array of candidates in input (flat-index) order:
 *
 *   i = 0; nb = n
 *   while i < nb:
 *     m = FIRST position in [i, nb) with the largest current score            (strict '<' scan)
 *     swap entries i and m; emit entry i (box, current score, original index)
 *     pos = i + 1
 *     while pos < nb:
 *       ovr = inter / (area_i + area_pos - inter)                                (fp32, IEEE division, no contraction)
 *       NAIVE:    weight = 0        if ovr >= iou_thr else 1
 *       LINEAR:   weight = 1 - ovr  if ovr >= iou_thr else 1
 *       GAUSSIAN: weight = expf(-(ovr*ovr) / sigma)
 *       score[pos] *= weight
 *       if score[pos] < min_score: entry pos = entry nb-1; nb -= 1; continue     (re-examine pos)
 *       pos += 1
 *     i += 1
 *
 * The comparison is `>=` (mmcv's softnms_cpu); the division form only (yv4_nms_set_iou_form does not apply: mmcv 1.3.x
 * has no GPU soft-NMS).  GAUSSIAN's exp may differ from a host expf in the last bit.  The output is the selection order.
 * Equivalent form of the end swaps of one step: the k-th discarded position from the left below the new end receives the
 * k-th surviving entry from the right at or above it. */
#define YV4_SOFT_NMS_NAIVE 0
#define YV4_SOFT_NMS_LINEAR 1
#define YV4_SOFT_NMS_GAUSSIAN 2
/* yv4_nms_images' buffers and semantics (class offset box + label*(max_coord[n] + 1), fused classes or labels, images
 * with counts[n] >= split_thr flagged out_count[n] = -1), with soft-NMS over the image's candidates in FLAT-INDEX order
 * (the keys are sorted in place by their low word).  out_dets carries the decayed scores, in selection order; the loop
 * stops after max_out selections.  Images with more than 10240 candidates are flagged like split ones (the host then
 * runs yv4_soft_nms_split, per_label = 0 below split_thr).
 * Returns YV4_E_INVALID (no device work) for an unknown method, sigma <= 0 with GAUSSIAN, or bad sizes. */
int yv4_soft_nms_images(uint64_t* keys, int64_t key_cap, const int32_t* counts, const float* max_coord,
                        const float* boxes, int64_t boxes_per_image, const int32_t* labels, int64_t label_stride,
                        int fused_classes, int N, int method, float iou_thr, float sigma, float min_score, int max_out,
                        int split_thr, float* out_dets, int32_t* out_labels, int64_t* out_index, int32_t* out_count,
                        void* stream);
/* ONE image, n (host value) candidate keys in any order, work of yv4_soft_nms_split_work(n) bytes:
 *   per_label = 1: mmcv's n >= split_thr branch -- soft-NMS per label over that label's candidates in flat-index order,
 *                  survivors re-sorted by (DECAYED score desc, flat index asc), the first max_out returned.  A label stops
 *                  after max_out selections unless its next selection ties the score of its max_out-th one.
 *   per_label = 0: one soft-NMS over all n candidates (the single call, for n above the images kernel's limit), selection
 *                  order, the first max_out.
 * max_coord: the class-offset unit minus one (-1: no offset).  One problem (a label, or all n with per_label = 0) holds
 * at most 524288 candidates; per_label = 0 checks it up front, a larger label makes the call report out_count = -2. */
size_t yv4_soft_nms_split_work(int64_t n);
int yv4_soft_nms_split(const uint64_t* keys, int64_t n, float max_coord, const float* boxes, const int32_t* labels,
                       int fused_classes, int per_label, int method, float iou_thr, float sigma, float min_score,
                       int max_out, void* work, float* out_dets, int32_t* out_labels, int64_t* out_index,
                       int32_t* out_count, void* stream);

/* ---- deterministic mode (ABI 6) ----------------------------------------------------------------
 * The reference's training step is bit-reproducible run to run wherever torch's is (torch.nn.BatchNorm2d,
 * mmdet/models/backbones/darknetcsp.py:15-35, sums its statistics in a fixed order); this library's default sums
 * the BatchNorm statistics, the BatchNorm backward's dbeta / dgamma, the loss sums, the positives' row gradients,
 * the head's bias gradients, the SPP backward scatter and the gradient norm with atomics in arrival order: equal
 * to rounding, not to the bit -- and a 110-layer network under batch statistics turns one ulp into percents of
 * the loss within a hundred steps.  yv4_set_deterministic(1) switches all of those accumulations to 64-bit
 * FIXED-POINT integer words (integer addition is associative: the result does not depend on the arrival order;
 * a non-finite or out-of-range addend reads back as NaN) and the gradient norm to per-workgroup partials added
 * in index order.  With the deterministic weight gradient (yv4_conv_wgrad_det, the default of the Python host)
 * two runs of a training step from the same state give the same bits.  Process-wide; switch it between steps.
 * SCRATCH SIZES below ("work", "sums", "dbias", "gpos", "zero_after") are stated for both modes: the
 * deterministic forms need twice the 64-bit words (hi | lo), so callers allocate the larger size always. */
int yv4_set_deterministic(int on);
int yv4_get_deterministic(void);

/* Build candidate keys for the standalone batched_nms op from plain
 * boxes/scores (n candidates of one image): keys[i] = ~bits(score_i)<<32 | i,
 * counts[0] = n, max_coord[0] = max over all box coordinates. */
int yv4_nms_prepare(const float* boxes, const float* scores, int64_t n,
                    uint64_t* keys, int32_t* counts, float* max_coord,
                    void* stream);

/* ---- training side (fp32) -----------------------------------------------------
 * Replaces the autograd of mmcv ConvModule in training mode (cuDNN backward-filter /
 * backward-data, ATen batch_norm fwd/bwd with batch statistics, MishCudaFunction.backward,
 * mmdet/ops/mish_cuda/mish.py:27-36) for the blocks of mmdet/models/backbones/darknetcsp.py.
 *
 * yv4_conv_wgrad: dW[co][(kh,kw,ci)] += sum_m dY[m][co] * x[n, ho*s-p+kh, wo*s-p+kw, ci];
 *   `d` is the FORWARD descriptor; the y_* fields describe the dY view; dW has the packed
 *   forward layout (Cout, KH*KW*Cin) and must be zero on entry (partial sums are added with
 *   float atomics).  Cin, Cout and all view strides/offsets must be multiples of 4.
 * The data gradient is yv4_conv_bn_act_fwd on dY with the weights transposed+flipped (pad
 *   K-1-p); for stride 2 dY is zero-dilated first:
 * yv4_dilate2_fwd: dst (N,2H,2W,C dense) [n,2y,2x,c] = src[n,y,x,c], zeros elsewhere.
 * yv4_bn_train_stats: per-channel batch mean / 1/sqrt(biased var + eps) of an NHWC view with M
 *   rows; updates running_mean/var (unbiased var, `momentum`) when given. work: 4*C doubles (2*C used unless
 *   deterministic).
 * yv4_bn_act_fwd:  y = act((x-mean)*invstd*gamma+beta) (+ residual).
 * yv4_bn_act_bwd:  from dy (gradient w.r.t. y), the saved conv output x and the batch
 *   statistics: dx, dgamma, dbeta (the activation is recomputed, nothing else is saved).  */
int yv4_conv_wgrad(const yv4_conv_desc* d, const float* x, const float* dy, float* dw, void* stream);
int yv4_dilate2_fwd(const float* src, float* dst, int N, int H, int W, int C, int src_cstride,
                    int src_coff, void* stream);
int yv4_bn_train_stats(const float* x, int64_t M, int C, int x_cstride, int x_coff, float eps,
                       float momentum, double* work, float* mean, float* invstd,
                       float* running_mean, float* running_var, void* stream);
int yv4_bn_act_fwd(const float* x, int x_cstride, int x_coff, const float* mean,
                   const float* invstd, const float* gamma, const float* beta,
                   const float* residual, int r_cstride, int r_coff, float* y, int y_cstride,
                   int y_coff, int64_t M, int C, int act, float slope, void* stream);
int yv4_bn_act_bwd(const float* x, int x_cstride, int x_coff, const float* dy, int dy_cstride,
                   int dy_coff, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float* dx, int dx_cstride, int dx_coff, float* dgamma,
                   float* dbeta, double* work, int64_t M, int C, int act, float slope, void* stream);

/* ---- 16-bit operand convolution (fp16 / bf16 in, fp32 accumulate) ---------------------
 * The reduced-precision form of yv4_conv_bn_act_fwd (BASELINE configs[2..4]; the reference
 * runs its ConvModules in half under mmcv's wrap_fp16_model / autocast, darknetcsp.py:15-35):
 * x, w, residual and (unless out_dtype == YV4_F32) y are NHWC / packed tensors of `dtype`
 * (YV4_F16 or YV4_BF16); scale/shift stay fp32; the epilogue runs in fp32 and rounds once.
 * Same descriptor as the fp32 entry; channel counts, strides and offsets of the 16-bit views
 * must be multiples of 8 (16-byte pixel chunks), w is (Cout, KH*KW*Cin) with Cin padded to 8.
 * desc->tile: YV4_TILE_AUTO or one of YV4_HTILE_*. */
#define YV4_HTILE_128x128 1
#define YV4_HTILE_128x64 2
#define YV4_HTILE_64x64 3
/* 3x3 / stride 1 / pad 1, Cin % 64 == 0, even Cout >= 64, 16-bit output, even channel strides / offsets
 * (conv3x3_pp_h16.hip): one PERSISTENT 8-wave workgroup per CU in ping-pong, 256 pixels x 128 channels per tile, the
 * three kw taps of a (chunk, kh) share one LDS image of the activations, the LDS-DMA ring runs on across tiles, the
 * epilogue stores channel pairs straight from the accumulators.  Same K order and epilogue expressions as the generic
 * tiles.  (Id 5, the 256 x 64 form of round 2's non-persistent kernel, is gone and refused.) */
#define YV4_HTILE_PP3x3 4
/* 3x3 / stride 1 / pad 1 with Cin % 64 == 0 and Cout % 16 == 0 on WIDE wave tiles (16 PT pixels x 64 channels per wave on
 * v_mfma_f32_16x16x32, PT = 2 / 3 / 4 / 6 / 8; workgroup tiles 256 x 256, 192 x 256, 128 x 256, 384 x 128, 256 x 128, 384 x 64 or 256 x 64 chosen
 * per layer so that whole rounds of CUs are filled; csrc/conv3x3_wide_h16.hip).  Same K order and epilogue expressions
 * as the other tiles; measured bit-identical to them (tests/test_gpu_h16.py::test_wide3x3_matches_generic_bitwise). */
#define YV4_HTILE_W3x3 5
/* ... with the tile shape forced (i = 0..6: 256 x 256, 192 x 256, 128 x 256, 384 x 128, 256 x 128, 384 x 64, 256 x 64): tests, tile sweeps */
#define YV4_HTILE_W3x3_SHAPE(i) (5 + 8 * ((i) + 1))
/* The same wave tiles as a general implicit GEMM (any kernel size / stride / padding with Cin % 64 == 0, Cout % 16 == 0,
 * 16-bit output; a K tile = one (64-channel chunk, tap) gathered with the tap's offset): the stride-2 3x3 layers, the deep
 * / wide 1x1 layers, the scattered classes of stride-2 data gradients (csrc/conv_wide_h16.hip).  Bit-identical to the
 * generic tiles.  YV4_HTILE_WIDE_SHAPE(i), i = 0..4, forces a workgroup tile shape as above. */
#define YV4_HTILE_WIDE 8
#define YV4_HTILE_WIDE_SHAPE(i) (8 + 8 * ((i) + 1))
/* 1x1 / stride 1, Cin <= 256, even Cout >= 16 with a 16-bit output (residual allowed) or any Cout >= 16 with an fp32
 * output (no residual) (conv1x1_ws_h16.hip): one persistent 8-wave workgroup per CU, the weight slab resident in LDS,
 * wave-private rings of 32-pixel strips */
#define YV4_HTILE_WS_1x1 6
/* 3x3 / stride 1 / pad 1 with few channels -- Cin 16, 32 or 64, even Cout in [16, 64], 16-bit output
 * (conv3x3_small_h16.hip): one persistent 8-wave workgroup per CU on 16 x 16 output tiles, the weights resident in LDS,
 * the 18 x 18 input tile double-buffered through LDS-DMA */
#define YV4_HTILE_S3x3 7
int yv4_conv_bn_act_fwd_h16(const yv4_conv_desc* d, int dtype, int out_dtype, const void* x,
                            const void* w, const float* scale1, const float* shift1,
                            const float* scale2, const float* shift2, const void* residual,
                            void* y, void* stream);
int yv4_conv_h16_pick_tile(const yv4_conv_desc* d);
/* Stem of the 16-bit path (3-channel image, 3x3 s1 p1, Cout <= 64): x and w are fp32 exactly as
 * for yv4_conv_bn_act_fwd's stem tile, the arithmetic is fp32, only y is `out_dtype`. */
int yv4_conv_stem_fwd(const yv4_conv_desc* d, const float* x, const float* w,
                      const float* scale1, const float* shift1, void* y, int out_dtype,
                      void* stream);

/* The first two layers of CSPDarknet as one launch for the 16-bit inference plans (stem_down_h16.hip): the stem
 * Conv(3 -> C1, 3x3, s1) + BN + act (darknetcsp.py:357-366) and the next stage's conv_downscale Conv(C1 -> C2, 3x3, s2)
 * + BN + act (darknetcsp.py:290-300), straight from the NCHW fp32 image (N, 3, H, W) to the NHWC 16-bit map
 * (N, ceil(H/2), ceil(W/2), C2) at channel offset y_coff of pixels of y_cstride channels.  w1: the fp32 stem weights
 * as yv4_conv_stem_fwd takes them, (C1, 9 taps x 4 channels); the stem is computed on 16-bit MFMAs with a three-term
 * hi / lo split of the fp32 products (result = the fp32 stem's to fp32 accumulation noise) and rounded to `dtype`
 * like its stored output; w2: (C2, 9 * C1) in `dtype`, as yv4_conv_bn_act_fwd_h16 takes it.  C1 in {16, 32},
 * C2 in {32, 64}. */
int yv4_stem_down_fwd_h16(int dtype, const float* x_nchw, int N, int H, int W, const float* w1,
                          const float* scale1, const float* shift1, int C1, int act1, float slope1,
                          const void* w2, const float* scale2, const float* shift2, int C2, int act2,
                          float slope2, void* y, int y_cstride, int y_coff, void* stream);

/* 16-bit forms of the layout adaptors and the SPP pools (same argument meaning as the fp32
 * entries; the boundary tensors stay fp32 NCHW like the reference's, the NHWC side is `dtype`).
 * The nearest resample / concat copy has no 16-bit entry: call yv4_resample_nearest_fwd with the
 * channel arguments halved (a 16-bit view with C % 8 == 0 is an fp32 view with C/2 channels). */
int yv4_nchw_to_nhwc_h16(const float* src, void* dst, int N, int C, int H, int W,
                         int dst_cstride, int dst_coff, int zero_pad, int dtype, void* stream);
int yv4_nhwc_to_nchw_h16(const void* src, float* dst, int N, int C, int H, int W,
                         int src_cstride, int src_coff, int dtype, void* stream);
int yv4_spp_pool_fwd_h16(void* buf, int N, int H, int W, int C, int cstride, int coff,
                         int dtype, void* stream);

/* 16-bit forms of the training kernels (BASELINE configs[2], [4]: bf16 training): activations and
 * their gradients are `dtype` (YV4_F16 / YV4_BF16) NHWC views, statistics / gamma / beta / dW stay
 * fp32, reductions run in double.  Same argument meaning as the fp32 entries above.  The data
 * gradient is yv4_conv_bn_act_fwd_h16 on dY; zero-dilation of a 16-bit map is yv4_dilate2_fwd
 * with the channel arguments halved. */
int yv4_conv_wgrad_h16(const yv4_conv_desc* d, int dtype, const void* x, const void* dy,
                       float* dw, void* stream);
/* Deterministic weight gradient (round 2): same contract as yv4_conv_wgrad / yv4_conv_wgrad_h16 (dw += the weight
 * gradient, dtype YV4_F32 / YV4_F16 / YV4_BF16 operands), but the chunks of the N*Ho*Wo reduction store their partial
 * sums to slabs of `workspace` (yv4_conv_wgrad_workspace bytes; 0 = a single chunk, no workspace needed) and a small
 * kernel adds the slabs to dw in chunk order: run-to-run bit-identical, no float atomics. */
size_t yv4_conv_wgrad_workspace(const yv4_conv_desc* d, int dtype);
int yv4_conv_wgrad_det(const yv4_conv_desc* d, int dtype, const void* x, const void* dy, float* dw,
                       float* workspace, size_t workspace_bytes, void* stream);
int yv4_bn_train_stats_h16(const void* x, int dtype, int64_t M, int C, int x_cstride, int x_coff,
                           float eps, float momentum, double* work, float* mean, float* invstd,
                           float* running_mean, float* running_var, void* stream);
int yv4_bn_act_fwd_h16(const void* x, int dtype, int x_cstride, int x_coff, const float* mean,
                       const float* invstd, const float* gamma, const float* beta,
                       const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                       int y_coff, int64_t M, int C, int act, float slope, void* stream);
int yv4_bn_act_bwd_h16(const void* x, int dtype, int x_cstride, int x_coff, const void* dy,
                       int dy_cstride, int dy_coff, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, void* dx, int dx_cstride,
                       int dx_coff, float* dgamma, float* dbeta, double* work, int64_t M, int C,
                       int act, float slope, void* stream);

/* yv4_bn_act_bwd_h16 (eval_mode = 0) / yv4_bn_eval_act_bwd (eval_mode = 1) with dgamma / dbeta ADDED to the given
 * arrays -- the parameters' own gradients -- instead of overwriting them (flags bit 0 = eval_mode). */
int yv4_bn_act_bwd_accum(const void* x, int dtype, int x_cstride, int x_coff, const void* dy,
                         int dy_cstride, int dy_coff, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, void* dx, int dx_cstride,
                         int dx_coff, float* dgamma, float* dbeta, double* work, int64_t M, int C,
                         int act, float slope, int flags /* 1: eval-mode BN, 2: work already zero */,
                         void* stream);

/* SyncBN (the configs under configs/yolov5_ddp: norm_cfg type 'SyncBN' = torch.nn.SyncBatchNorm): the train-mode BN
 * kernels above with the cross-rank exchange between their two halves.  Forward: yv4_bn_partial_sums
 * leaves [sum x (C) | sum x^2 (C)] of the local rows in `work` (double); the caller all-reduces `work`
 * (SUM) and the row count, then yv4_bn_finalize (replicas = 1; > 1: `work` is that many consecutive
 * [2*C] blocks to be added up first, any count, see yv4_conv_fwd_stats; with clear_work every one of them is zeroed;
 * in deterministic mode replicas = YV4_STATS_REPLICAS means the conv epilogue's fixed-point words) turns the totals into mean / invstd and updates the
 * running statistics (unbiased variance over M_total).  Backward: yv4_bn_act_bwd_sums leaves
 * [sum dz (C) | sum dz*xhat (C)] in `work` and writes the LOCAL dgamma / dbeta (what
 * torch.nn.SyncBatchNorm returns: DDP averages them afterwards); the caller all-reduces `work`;
 * yv4_bn_act_bwd_apply computes dx with the totals over M_total rows.  rows_dev (optional): the total
 * row count as one double in device memory -- it is all-reduced together with the sums, so no host
 * round trip is needed to learn it; when given it overrides M_total. */
int yv4_bn_partial_sums(const void* x, int dtype, int64_t M, int C, int x_cstride, int x_coff,
                        double* work, void* stream);
/* The statistics pass fused into the producing convolution: y = conv(x, w) with the identity epilogue
 * (`ones` / `zeros`: Cout unit scales / zero shifts; y may be a channel slice of a wider buffer) and
 * stats = YV4_STATS_REPLICAS x [sum y (Cout) | sum y^2 (Cout)] doubles whose column sums are the
 * per-channel totals (the kernel spreads its atomics over the replicas; the buffer is cleared here).
 * dtype YV4_F32 / YV4_F16 / YV4_BF16 = type of x, w and y.  Feed it to yv4_bn_finalize with
 * replicas = YV4_STATS_REPLICAS. */
#define YV4_STATS_REPLICAS 64
int yv4_conv_fwd_stats(const yv4_conv_desc* d, int dtype, const void* x, const void* w,
                       const float* ones, const float* zeros, void* y, double* stats,
                       int stats_is_zero /* the caller keeps the buffer clean (yv4_bn_finalize clear_work) */,
                       void* stream);
int yv4_bn_finalize(double* work, int replicas, int64_t M_total, const double* rows_dev, int C,
                    float eps, float momentum, float* mean, float* invstd, float* running_mean,
                    float* running_var, int clear_work /* zero `work` once read */,
                    double* zero_after /* NULL, or 4*C doubles to clear for the layer's backward reduction */,
                    void* stream);
/* The totals of a yv4_conv_fwd_stats buffer as 2*C doubles [sum | sum of squares] (what SyncBN all-reduces before
 * yv4_bn_finalize(replicas = 1)), in either mode; clear_stats: the replicas are zeroed as they are read. */
int yv4_conv_stats_fold(double* stats, int C, int clear_stats, double* out, void* stream);
int yv4_bn_act_bwd_sums(const void* x, int dtype, int x_cstride, int x_coff, const void* dy,
                        int dy_cstride, int dy_coff, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, float* dgamma, float* dbeta,
                        double* work, int64_t M, int C, int act, float slope, void* stream);
int yv4_bn_act_bwd_apply(const void* x, int dtype, int x_cstride, int x_coff, const void* dy,
                         int dy_cstride, int dy_coff, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, void* dx, int dx_cstride,
                         int dx_coff, const double* work, int64_t M, int64_t M_total,
                         const double* rows_dev, int C, int act, float slope, void* stream);

/* A conv weight (Cout, Cin, KH, KW), addressed through its element strides (contiguous or channels_last), to
 * the packed operand of the conv kernels in one pass: rows x (KHo*KWo*ICp), K ordered (kh, kw, channel), the
 * channel count zero-padded to a multiple of pad_to, cast to `dtype`.  Output tap (kh, kw) reads source tap
 * (kh0 + kh*kh_step, kw0 + kw*kw_step).  transpose = 0: rows = Cout, channels = Cin (the forward operand:
 * KHo = KH, kh0 = 0, step 1); 1: rows = Cin, channels = Cout -- mirrored taps (kh0 = KH-1, step -1) give the
 * operand of the data gradient, a tap subset the operand of one parity class of a stride-2 data gradient. */
int yv4_pack_weight(const float* w, int64_t s_co, int64_t s_ci, int64_t s_kh, int64_t s_kw, int Cout,
                    int Cin, int KH, int KW, int KHo, int KWo, int kh0, int kh_step, int kw0,
                    int kw_step, int transpose, int pad_to, void* dst, int dtype, void* stream);

/* yv4_pack_weight over a table of weights in ONE launch (a training step packs every conv weight twice -- forward
 * operand and data-gradient operand -- 750 launches of a few microseconds each on YOLOv4-L; the table is built once and
 * replayed after every optimizer step).  The table lives in DEVICE memory; descriptor i serves workgroups
 * [first_block, first_block + nblocks), rows_per_block output rows each (the caller lays the ranges out back to
 * back, total_blocks = their sum); the other fields are yv4_pack_weight's arguments.  Any rows_per_block >= 1 is
 * correct; the pass is fastest when a workgroup owns whole rows r with all their KHo*KWo taps (forward operand) or groups
 * of max(8, 64 / taps) such rows (transpose = 1: the source is contiguous ACROSS r), since a workgroup stages the source
 * box of its rows in LDS in source order. */
typedef struct yv4_pack_desc {
  const float* w;
  int64_t s_co, s_ci, s_kh, s_kw;
  void* dst;
  int32_t Cout, Cin, KHo, KWo, kh0, kh_step, kw0, kw_step, transpose, pad_to, dtype;
  int32_t first_block, nblocks, rows_per_block;
} yv4_pack_desc;
int yv4_pack_weights_multi(const yv4_pack_desc* table_dev, int n, int total_blocks, void* stream);

/* Backward of yv4_resample_nearest_fwd for INTEGER scale factors (the neck's 2x upsample into its concat buffer,
 * necks/yolo_neck_csp.py:213-219 / torch's upsample_nearest2d_backward): dx (N, Hs, Ws, C) dense = the sum of the
 * (Hd / Hs) x (Wd / Ws) pixels of dy that read it; dy is a channel slice (dy_cstride, dy_coff) of an (N, Hd, Wd, .) tensor
 * of `dtype`; fp32 sum, one rounding. */
int yv4_resample_nearest_bwd(const void* dy, void* dx, int N, int Hs, int Ws, int Hd, int Wd, int C,
                             int dy_cstride, int dy_coff, int dtype, void* stream);

/* One parity class of the data gradient of a stride-2 convolution: a stride-1 convolution of dY whose
 * output pixel (n, ho, wo) is stored at y[n, ho*sh + oh, wo*sw + ow, y_coff + c] of an
 * (N, Hy, Wy, y_cstride) tensor.  d->Ho / d->Wo are taken as given (rows past the input's edge read
 * zeros), d->stride must be 1, the epilogue is scale1/shift1 only.  For the 3x3 / stride 2 / pad 1 convs
 * of darknetcsp.py:288-335 and yolo_neck_csp.py the four classes (1, 2, 2 and 4 taps) cost exactly the
 * forward FLOPs; the zero-dilated form (yv4_dilate2_fwd + yv4_conv_bn_act_fwd) costs 4x. */
int yv4_conv_scatter_fwd(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1,
                         const float* shift1, float* y, int Hy, int Wy, int sh, int sw, int oh,
                         int ow, void* stream);
int yv4_conv_scatter_fwd_h16(const yv4_conv_desc* d, int dtype, const void* x, const void* w,
                             const float* scale1, const float* shift1, void* y, int Hy, int Wy,
                             int sh, int sw, int oh, int ow, void* stream);

/* Backward of an EVAL-mode BatchNorm (+ activation) inside a training graph (frozen stages /
 * norm_eval, darknetcsp.py:466-480): mean / invstd are the running statistics (constants), so
 * dx = gamma * invstd * dy * act'(z); dgamma / dbeta as in yv4_bn_act_bwd.  The forward is
 * yv4_bn_act_fwd(_h16) called with the running statistics. */
int yv4_bn_eval_act_bwd(const void* x, int dtype, int x_cstride, int x_coff, const void* dy,
                        int dy_cstride, int dy_coff, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, void* dx, int dx_cstride,
                        int dx_coff, float* dgamma, float* dbeta, double* work, int64_t M, int C,
                        int act, float slope, void* stream);

/* SPP backward: xcat is the forward's concat buffer (its first C channels are the pooled input),
 * dcat the gradient w.r.t. the 4C-channel concat; dx (N, H, W, C) fp32, dense, ZERO on entry, receives
 * the identity branch plus the three max-pool scatters (first maximum in row-major window order,
 * like ATen).  dtype is the element type of xcat / dcat (YV4_F32 / F16 / BF16). */
int yv4_spp_pool_bwd(const void* xcat, int x_cstride, int x_coff, const void* dcat, int d_cstride,
                     int d_coff, float* dx, int N, int H, int W, int C, int dtype, void* stream);

/* ---- optimizer side of the training step (flat fp32 arenas) -------------------------
 * The reference steps torch.optim.SGD(nesterov) with one param group per parameter
 * (core/custom_hooks/warmup_hooks.py:24-32 requires that), un-scales and clips gradients in
 * Fp16GradAccumulateOptimizerHook.after_train_iter (core/custom_hooks/accum_optim_hooks.py:37-60)
 * and averages all 658 state entries in a Python loop (StateEMAHook.after_train_iter,
 * core/custom_hooks/ema_hooks.py:80-98).  Here parameters, gradients, momentum buffers and EMA
 * copies are slices of four flat arenas and each of those steps is one streaming kernel; every
 * decision (clip coefficient, skip on overflow, loss-scale growth) stays on the device.
 *
 * yv4_grad_prepare: GradScaler.unscale_ + clip_grad_norm_(max_norm, 2) folded into one
 *   multiplier.  scale_state = {scale, growth_tracker} on the device or NULL (scale 1);
 *   max_norm <= 0 disables clipping; work: 2 + YV4_GRAD_PREPARE_MAX_WG doubles (2 used unless deterministic: then
 *   one partial per workgroup, added in index order); ctrl (4 floats, device) receives
 *   {grad multiplier = clip_coef/scale, total L2 norm of the unscaled gradients,
 *    found_inf (0/1), 1/scale}.
 * yv4_sgd_step: p -= lr*(nesterov ? g + m*b : b), b = m*b + g, g = grad*ctrl[0] + wd*p, with
 *   (lr, momentum, weight_decay, nesterov) per segment: seg_off has nseg+1 entries (float
 *   offsets, multiples of 4, seg_off[0] = 0, seg_off[nseg] = n), seg_hyper nseg*4 floats.
 *   No-op when ctrl[2] != 0 (GradScaler.step semantics).  ctrl may be NULL (multiplier 1).
 * yv4_loss_scale_update: GradScaler.update for the dynamic loss scale.
 * yv4_ema_update: ema = momentum*ema + (1-momentum)*online over n floats.                */
#define YV4_GRAD_PREPARE_MAX_WG 2048
int yv4_grad_prepare(const float* grad, int64_t n, const float* scale_state, float max_norm,
                     double* work, float* ctrl, void* stream);
int yv4_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n,
                 const int64_t* seg_off, const float* seg_hyper, int nseg, const float* ctrl,
                 void* stream);
int yv4_loss_scale_update(float* scale_state, const float* ctrl, float growth_factor,
                          float backoff_factor, int growth_interval, void* stream);
int yv4_ema_update(float* ema, const float* online, int64_t n, float momentum, void* stream);

/* ---- YOLOCSPHead training loss, forward and backward ------------------------------------------
 * Replaces responsible_indices (core/anchor/yolov4_anchor_generator.py:12-134, neighbor = 2),
 * get_targets_no_assigner + loss_single_no_assigner (models/dense_heads/yolocsp_head.py:437-575), the
 * decode (yolov4_bbox_coder.py:39-67), aligned GIoU and the three sigmoid-BCE / GIoU reductions for ALL
 * levels: forward = assign + positives + dense objectness pass, backward = positives + one pass that
 * writes the whole gradient of each level's head-conv output (its dtype, its NHWC layout) and the bias
 * gradient.  Nothing returns to the host in between.
 *   raw:   (N, H, W, Cp) head conv output WITHOUT bias, channel c = a*(5+C) + j, Cp >= A*(5+C)
 *   gt (G,4) fp32 x1 y1 x2 y2, gt_label (G) int64, gt_img (G) int64: the batch's ground truths concatenated
 *   candidate slot s = (k*A + a)*G + g  (k: 0 own cell, 1 left, 2 up, 3 right, 4 down) -- the position the
 *   positive has in the reference's index lists; duplicates of one anchor box resolve to the largest s
 *   (what the reference's index_put gives when run in order), deterministically.
 * work buffers (device): slot_anchor, conf_t: L*5*A*G; winner: N*anchors-per-image int32; npos: L int32;
 *   sums: L*3 double = [sum of class BCE | sum of objectness BCE | sum of (1 - GIoU)] per level, in a buffer of
 *   2*L*3 doubles; gpos (backward): L*5*A*G*(5+C) float in a buffer of 4x that many floats; dbias: A*(5+C)
 *   doubles per level in a buffer of twice as many (the second halves are the deterministic mode's lo words;
 *   results are always the doubles / floats at the front).
 * Losses: cls = w_cls*sum/(npos*C), conf = w_conf*sum/(N*H*W*A), bbox = w_bbox*sum/npos (0 where a level has no positive) --
 *   written to `losses` (L*3 float, [cls | conf | bbox] per level) by the forward call itself when the pointer is given
 *   (ABI 6: what yolocsp_head.py:553-575 computes with a dozen tensor ops per level), else left to the host.
 * yv4_yolo_loss_bwd: grad_out (L,3) float (device) = upstream gradients of [cls, conf, bbox] per level. */
#define YV4_LOSS_MAX_LEVELS 5
typedef struct yv4_loss_level {
  const void* raw;
  void* draw;          /* backward: gradient of raw, same shape / dtype */
  const float* bias;   /* A*(5+C) */
  double* dbias;       /* backward: A*(5+C) results, 2*A*(5+C) doubles of room */
  int32_t H, W, Cp, stride;
  float base_anchors[8][4];
} yv4_loss_level;
typedef struct yv4_loss_desc {
  yv4_loss_level levels[YV4_LOSS_MAX_LEVELS];
  int32_t num_levels, N, A, num_classes /* 0: class-agnostic */, G, dtype;
  const float* gt;
  const int64_t* gt_label;
  const int64_t* gt_img;
  float shape_thr, smooth /* one_hot_smoother */, ratio /* conf_iou_loss_ratio */, eps /* GIoU */;
  float w_cls, w_conf, w_bbox;
  int32_t* slot_anchor;
  int32_t* winner;
  int32_t* npos;
  float* conf_t;
  float* gpos;
  double* sums;
  float* losses;       /* optional (ABI 6): L*3 float results of the forward, see above */
} yv4_loss_desc;
int yv4_yolo_loss_fwd(const yv4_loss_desc* d, void* stream);
int yv4_yolo_loss_bwd(const yv4_loss_desc* d, const float* grad_out, void* stream);

/* ---- the same loss with the other box losses and SoftFocalLoss (additive within ABI 8) ----------------
 * yv4_yolo_loss_fwd_ex / _bwd_ex take the descriptor above plus yv4_loss_opts; yv4_yolo_loss_fwd / _bwd are these calls
 * with {YV4_BOX_GIOU, no focal}.  Assignment, winner resolution, work buffers, sums, the deterministic mode and the
 * one-pass gradient write do not depend on the options.
 * box_kind (models/losses/iou_loss.py:14-36,105-219; fp32, the reference's expression order; ov = overlap, a1 / a2 the
 * areas, cw / ch the enclosing box's clamped extents, eps = yv4_loss_desc.eps):
 *   YV4_BOX_GIOU        iou = ov / max(a1 + a2 - ov, eps);  loss = 1 - (iou - (E - U) / E),  E = max(cw * ch, eps)
 *   YV4_BOX_IOU_LINEAR  iou = max(ov / max(a1 + a2 - ov, 1e-6), eps);  loss = 1 - iou   (1e-6: bbox_overlaps' own default)
 *   YV4_BOX_IOU_LOG     the same iou;  loss = -log(iou)
 *   YV4_BOX_DIOU        iou = ov / (a1 + a2 - ov + eps);  c2 = cw^2 + ch^2 + eps  (eps is ADDED, not a clamp);
 *                       rho2 = ((tx1 + tx2) - (x1 + x2))^2 / 4 + ((ty1 + ty2) - (y1 + y2))^2 / 4;  loss = 1 - (iou - rho2 / c2)
 *   YV4_BOX_CIOU        DIoU's iou, c2, rho2;  v = 4 / pi^2 * (atan(w2 / (h2 + eps)) - atan(w1 / (h1 + eps)))^2;
 *                       loss = 1 - (iou - (rho2 / c2 + v^2 / (1 - iou + v))), differentiated through v, iou and the
 *                       denominator (nothing detached).  Where this is 0 / 0 (iou == 1 and v == 0) value and gradient
 *                       are nan, as in the reference: the point is not special-cased.
 *   Subgradients are torch's: one half on a tie of max / min against the target and of max(union, 1e-6); clamp(min = c)
 *   passes the gradient where x >= c.  The objectness target of a positive is (1 - r) + r * clamp(1 - loss, 0, 1) for
 *   every kind (so 0 wherever -log(iou) >= 1).
 * conf_focal / cls_focal (SoftFocalLoss, models/dense_heads/yolocsp_head.py:21-50), independently for the objectness and
 *   the class term, with soft targets t:  loss = bce * (t*alpha + (1-t)*(1-alpha)) * (1 - p_t)^gamma,
 *   p_t = t*p + (1-t)*(1-p), p = sigmoid(x); the derivative goes through all three factors.  gamma >= 1 (below 1 the
 *   derivative is unbounded at p_t = 1), 0 <= alpha <= 1.  gamma / alpha are ignored where the switch is 0.
 * Both calls validate the options before the device is touched (-1 + yv4_last_error: null opts, unknown kind,
 * gamma < 1, alpha outside [0, 1]). */
#define YV4_BOX_GIOU 0
#define YV4_BOX_IOU_LINEAR 1
#define YV4_BOX_IOU_LOG 2
#define YV4_BOX_DIOU 3
#define YV4_BOX_CIOU 4
typedef struct yv4_loss_opts {
  int32_t box_kind;      /* YV4_BOX_* */
  int32_t conf_focal;    /* 0 / 1 */
  float conf_gamma, conf_alpha;
  int32_t cls_focal;     /* 0 / 1 */
  float cls_gamma, cls_alpha;
  int32_t reserved[9];   /* zero */
} yv4_loss_opts;
int yv4_yolo_loss_fwd_ex(const yv4_loss_desc* d, const yv4_loss_opts* opts, void* stream);
int yv4_yolo_loss_bwd_ex(const yv4_loss_desc* d, const yv4_loss_opts* opts, const float* grad_out, void* stream);

/* ---- YOLOV3Head training loss, forward and backward (ABI 8) ------------------------------------------
 * Replaces GridAssigner.assign (core/bbox/assigners/grid_assigner.py:73-156), responsible_flags + grid_anchors
 * (core/anchor/anchor_generator.py:667-727), BboxOverlaps2D (core/bbox/iou_calculators/iou2d_calculator.py),
 * YOLOBBoxCoder.encode (core/bbox/coder/yolo_bbox_coder.py:26-60), PseudoSampler and loss / loss_single /
 * get_targets / _get_targets_single (models/dense_heads/yolo_head.py:396-586) for ALL levels and images of a batch:
 * forward = assignment + the four loss sums per level, backward = one pass that writes the whole gradient of every
 * level's prediction map.  Nothing returns to the host in between.
 *   pred:  fp32 logits (N, A*(5+C), H, W) read through the element strides sn, sc, sh, sw (NCHW and channels-last
 *          maps without a copy), channel a*(5+C) + j; dpred (backward) is written with the same strides.
 *   gt (G,4) fp32 x1 y1 x2 y2, gt_label (G) int64, gt_img (G) int64 NON-DECREASING: the batch's ground truths
 *          concatenated image by image.
 *   Anchors of an image: all levels concatenated in level order, (y*W + x)*A + a inside a level.
 *   Negatives: max IoU over the image's ground truths in (neg_lo, neg_hi] -- neg_iou_thr = t is (-1, t] (IoUs are
 *   >= 0), the tuple form (lo, hi) is (lo, hi]; with no ground truth every anchor is negative.  Threshold positives,
 *   per-gt claims (gt_max_assign_all), one-hot smoothing (smoother) and the coder's eps (eps, eps_hi = fp32 of
 *   1 - eps) as the reference; iou_eps is BboxOverlaps2D's union clamp.  A ground truth whose centre cell lies off a
 *   level's map has no responsible cell at that level (the reference raises or wraps its index there).
 * Losses per level [cls | conf | xy | wh] = loss_weight[k] * sum, divided by the element count where
 *   reduce_mean[k] (weight_reduce_loss with reduction='mean'), written to `losses` (L*4 float, device) by the
 *   forward.  yv4_yolov3_loss_bwd: grad_out (L,4) float (device) = upstream gradients of those.
 * work buffers (device): img_off N+1, gt_cell L*G, gt_max G, gt_arg G int32; assigned N*(anchors per image) int32 --
 *   after the forward it holds assigned_gt_inds of every anchor (-1 / 0 / k, k-1 indexing the image's ground truths);
 *   the backward reads it, so it must survive until then; sums 2*L*4 doubles (the second half: the deterministic
 *   mode's lo words). */
#define YV4_V3_LOSS_MAX_LEVELS 5
typedef struct yv4_v3_loss_level {
  const float* pred;
  float* dpred;            /* backward: gradient of pred, same strides */
  int64_t sn, sc, sh, sw;  /* element strides of pred (and dpred) */
  int32_t H, W, stride, reserved;
  float base_anchors[8][4];
} yv4_v3_loss_level;
typedef struct yv4_v3_loss_desc {
  yv4_v3_loss_level levels[YV4_V3_LOSS_MAX_LEVELS];
  int32_t num_levels, N, A, num_classes, G, gt_max_assign_all;
  const float* gt;
  const int64_t* gt_label;
  const int64_t* gt_img;
  float pos_iou_thr, neg_lo, neg_hi, min_pos_iou;
  float eps, eps_hi, iou_eps, smoother;
  float loss_weight[4];    /* cls, conf, xy, wh */
  int32_t reduce_mean[4];  /* 0: reduction='sum', 1: reduction='mean' */
  int32_t* img_off;
  int32_t* gt_cell;
  int32_t* gt_max;
  int32_t* gt_arg;
  int32_t* assigned;
  double* sums;
  float* losses;
} yv4_v3_loss_desc;
int yv4_yolov3_loss_fwd(const yv4_v3_loss_desc* d, void* stream);
int yv4_yolov3_loss_bwd(const yv4_v3_loss_desc* d, const float* grad_out, void* stream);

/* ---- test-time input pipeline (Resize keep_ratio -> Pad -> Normalize -> ImageToTensor of
 * configs/yolov4/yolov4l_coco_mosaic.py:70-84) for one 8-bit HWC image: bilinear resize with OpenCV's 8-bit
 * fixed-point INTER_LINEAR arithmetic to (new_h, new_w), padding to (Hp, Wp) with pad_val, (v - mean) * (1/std)
 * in fp32 with the channel order swapped if to_rgb (mean / std in OUTPUT channel order, host pointers), written as
 * 3 fp32 planes of Hp*Wp (plane_stride elements apart) -- the image's slot of an NCHW batch.
 * pad_before_normalize: the Pad transform precedes Normalize (the pad value is normalised as well).
 * PARITY UNPINNED: the arithmetic being mirrored is mmcv's / OpenCV's (absent from the build image). */
int yv4_letterbox_u8(const uint8_t* src, int src_h, int src_w, int src_pitch, float* dst, int Hp, int Wp,
                     int64_t plane_stride, int new_h, int new_w, const float* mean3, const float* std3,
                     int to_rgb, int pad_val, int pad_before_normalize, void* stream);

/* ---- evaluation: the reference's two Cython ops, batched over (image, class) problems ----------
 * mmdet/ops/eval_utils/iou/iou_coco.pyx:8-56 and match/match_coco.pyx:8-57, called per image and class
 * from core/evaluation/mean_ap_flexible.py:19-37.  Problem p owns detections [det_off[p], det_off[p+1])
 * (rows of `det`, x1 y1 x2 y2), ground truths [gt_off[p], gt_off[p+1]) and the row-major
 * (num_det x num_gt) IoU block at iou_off[p]; the offset tables have P+1 int64 entries (device).
 * yv4_iou_coco_batched: IoU with the crowd convention (union = detection area for crowd gts), 0 for
 *   non-overlapping pairs, union <= 0 -> 1e-7; bit-exact fp32.
 * yv4_match_coco_batched: per IoU threshold t, detections in order take the best still-available gt
 *   (crowd gts stay available; a match to a regular gt is not given up for an ignore gt);
 *   matched[det_off[p]*num_thrs + t*num_det + d] = gt index inside the problem or -1.
 *   work: num_thrs * total_gt bytes. */
int yv4_iou_coco_batched(const float* det, const float* gt, const uint8_t* is_crowd,
                         const int64_t* det_off, const int64_t* gt_off, const int64_t* iou_off,
                         int P, int64_t total_pairs, float* iou, void* stream);
int yv4_match_coco_batched(const float* iou, const int64_t* det_off, const int64_t* gt_off,
                           const int64_t* iou_off, const float* iou_thrs, int num_thrs,
                           const uint8_t* is_ignore, const uint8_t* is_crowd, int P, uint8_t* work,
                           int32_t* matched, void* stream);

/* ---- VOC-style mAP (csrc/map_eval.hip; additive within ABI 8) ------------------------------------------------------
 * mmdet/core/evaluation/bbox_overlaps.py:4-48 and the two true/false-positive rules of mean_ap.py (tpfp_default
 * :153-237, tpfp_imagenet :59-150), which eval_map calls per image and class and once per IoU threshold, batched over
 * P (image, class) problems with the table layout of the calls above: the offset tables have P+1 int64 entries
 * (device), problem p owns rows [off[p], off[p+1]) of each box array and the row-major (n1 x n2) block at iou_off[p].
 * All pointers but `stream` are device pointers; boxes are x1 y1 x2 y2 float32, 16-byte aligned.
 *
 * yv4_bbox_overlaps_batched: overlap / max(union, eps) per pair in the reference's fp32 operation order
 *   (area = (x2-x1)*(y2-y1), overlap = max(xe-xs,0)*max(ye-ys,0), union = (area1+area2)-overlap for YV4_OVERLAPS_IOU,
 *   area1 for YV4_OVERLAPS_IOF); bit-exact.  The reference's operand swap for rows > cols changes no bit (one
 *   commutative add) and is not made.  total_pairs = iou_off[P]; 0 is legal (nothing is launched). */
#define YV4_OVERLAPS_IOU 0
#define YV4_OVERLAPS_IOF 1
int yv4_bbox_overlaps_batched(const float* boxes1, const float* boxes2, const int64_t* off1, const int64_t* off2,
                              const int64_t* iou_off, int P, int64_t total_pairs, int mode, float eps, float* iou,
                              void* stream);
/* yv4_tpfp_batched: tp / fp flags of every detection for num_thrs IoU thresholds and num_ranges area ranges from ONE
 *   IoU block per problem (the reference recomputes it per threshold).
 *   det (total_det, 4): the detections in their ORIGINAL order; order[det_off[p] + s] = index inside problem p of the
 *     s-th detection visited (the host's np.argsort(-scores)), rank = its inverse (rank[det_off[p] + order[..s]] = s).
 *     YV4_TPFP_DEFAULT reads rank only, YV4_TPFP_IMAGENET reads order only; the other may be null.
 *   gt (total_gt, 4): per problem the class's gts followed by its ignored gts, gt_ignore one byte each (1 = ignored).
 *   iou: yv4_bbox_overlaps_batched(det, gt) -- for YV4_TPFP_IMAGENET against gt - 1 (the host subtracts), while `gt`
 *     here stays the unshifted boxes (their areas select the range).
 *   gt_ratio (total_gt; imagenet only): w*h / ((w+10)*(h+10)) per gt as the host's numpy evaluates it; the gt's
 *     threshold is min(gt_ratio, iou_thrs[t]).
 *   area_ranges: num_ranges (min, max) float32 pairs, or null with num_ranges == 1 for "no range".  A box is in range
 *     when area >= min && area < max.
 *   tp, fp: (num_thrs, num_ranges, total_det) bytes; problem p's (T, K, nd) block is the column slice
 *     [det_off[p], det_off[p+1]), columns in the original detection order.
 *   YV4_TPFP_DEFAULT: a detection whose row maximum (first-occurrence argmax g) reaches iou_thrs[t] is nothing when g
 *     is ignored or out of range, else tp when it has the smallest rank among the detections that reach t with the
 *     same argmax (an integer atomicMin per (gt, t), then a parallel pass), else fp.
 *   YV4_TPFP_IMAGENET: one sequential walk per (problem, t): detections in `order` take the best still-uncovered gt
 *     with iou >= its threshold (first maximum wins); the gt is covered even when ignored; tp when the gt is neither
 *     ignored nor out of range.
 *   Both: an unmatched detection is fp when its own area is in range; a problem without gts marks every in-range
 *     detection fp; problems without detections and total_det == 0 are legal.
 *   work: yv4_tpfp_work(mode, total_det, total_gt, num_thrs) bytes, 4-byte aligned, contents undefined before and
 *     after.  total_det and total_gt must be below 0x7f7f7f7f. */
#define YV4_TPFP_DEFAULT 0
#define YV4_TPFP_IMAGENET 1
size_t yv4_tpfp_work(int mode, int64_t total_det, int64_t total_gt, int num_thrs);
int yv4_tpfp_batched(int mode, const float* det, const float* gt, const uint8_t* gt_ignore, const float* gt_ratio,
                     const int32_t* order, const int32_t* rank, const int64_t* det_off, const int64_t* gt_off,
                     const int64_t* iou_off, int P, int64_t total_det, int64_t total_gt, const float* iou,
                     const float* iou_thrs, int num_thrs, const float* area_ranges, int num_ranges, void* work,
                     uint8_t* tp, uint8_t* fp, void* stream);

/* ---- COCO bbox evaluation (csrc/coco_eval.hip; additive within ABI 8) ------------------------------------------------
 * pycocotools' COCOeval with iouType='bbox' and useCats=1 (computeIoU / evaluateImg / accumulate), as
 * mmdet/datasets/coco.py:547-551 configures it; the definition is restated in mmdet-yolov4_amd/coco_eval.py.
 * Problem p = image * K + category (images and categories in the order of their sorted ids) owns the ground truths
 * [gt_off[p], gt_off[p+1]) and, after yv4_coco_rank, the sorted positions [det_off[p], det_off[p+1]).  All pointers
 * but `stream` and `max_dets` are device pointers.  Every float64 value is one IEEE operation of the definition in
 * its order and every sum is an integer: bit-exact against the definition, identical bytes from run to run.
 *
 * yv4_coco_rank: one stable key-value sort of the flat detection table by (problem, descending score).
 *   det (total_det, 5) float32 x1 y1 x2 y2 score in the caller's order; prob (total_det) int32: the detection's
 *     problem, or a value outside [0, P) for a detection that takes no part (it is sorted behind every problem).
 *   order (total_det) uint32: order[s] = row of `det` at sorted position s; sprob (total_det) int32: its problem
 *     (P for "no part"); det_off (P+1) int64.  The rank of position s inside its problem is s - det_off[sprob[s]];
 *     equal scores keep the caller's order.
 *   match_need (1) int64: the doubles of workspace yv4_coco_match needs for num_at = A * T walks with this
 *     max_det = maxDets[-1] (the problems whose IoU block or matched bits do not fit LDS); the caller reads it back.
 *   work: yv4_coco_rank_work(total_det) bytes, 8-byte aligned.  total_det == 0 is legal (det_off is zeroed). */
size_t yv4_coco_rank_work(int64_t total_det);
int yv4_coco_rank(const float* det, const int32_t* prob, int64_t total_det, int P, int max_det, int num_at,
                  const int64_t* gt_off, void* work, uint32_t* order, int32_t* sprob, int64_t* det_off,
                  int64_t* match_need, void* stream);
/* yv4_coco_match: one wave per problem; its first min(num_det, max_det) detections in rank order against its gts.
 *   gt_box (total_gt, 4) float64 x y w h; gt_area (total_gt) float64 (the annotation's own area); gt_flag (total_gt)
 *     bytes: bit 0 = iscrowd, bit 1 = ignore (COCOeval overwrites ignore by iscrowd; the caller decides).
 *   iou_thrs (T) float64; area_rng (A, 2) float64 [lo, hi], both bounds inclusive; A <= 64.
 *   The IoU block (float64, union = detection area for a crowd gt, 0 when w <= 0 or h <= 0) is computed once and
 *     shared by the A x T greedy walks, one per lane (groups of 64 when A * T > 64).
 *   flags (total_det, A * T) bytes, zeroed first: flags[s * A*T + a * T + t] bit 0 = sorted position s is matched,
 *     bit 1 = it is ignored (its gt is ignored in range a, or it is unmatched and its own area is outside the range).
 *   counts (K, A) int32, zeroed first: the gts with ignore == 0 and area inside range a, per category.
 *   work / work_len: at least *match_need doubles (may be null / 0 when that is 0).  state (2) int64: [1] != 0
 *     afterwards means the workspace was too small and problems were skipped. */
int yv4_coco_match(const float* det, const uint32_t* order, const int64_t* det_off, const double* gt_box,
                   const double* gt_area, const uint8_t* gt_flag, const int64_t* gt_off, int P, int K, int64_t total_det,
                   int max_det, const double* iou_thrs, int T, const double* area_rng, int A, double* work,
                   int64_t work_len, int64_t* state, uint8_t* flags, int32_t* counts, void* stream);
/* yv4_coco_accumulate: a second stable sort, by (category, descending score) from the (image-major, rank) order of
 *   yv4_coco_rank -- ties fall as COCOeval's mergesort over the concatenated images leaves them -- then per
 *   (k, a, m, t) over the category's detections with rank < maxDets[m] (and < maxDets[-1]): integer cumulative tp / fp,
 *   rc = tp / npig, pr = tp / (fp + tp + 2^-52), pr's suffix maximum, and np.searchsorted(rc, rec_thrs, 'left').
 *   max_dets (M <= 16) int32 on the HOST; rec_thrs (R <= 256) float64, ascending.
 *   precision, scores (T, R, K, A, M) and recall (T, K, A, M) float64: -1 where counts[k][a] == 0.
 *   work: yv4_coco_accumulate_work(total_det, K, A * T) bytes, 8-byte aligned. */
size_t yv4_coco_accumulate_work(int64_t total_det, int K, int num_at);
int yv4_coco_accumulate(const float* det, const uint32_t* order, const int32_t* sprob, const int64_t* det_off,
                        const uint8_t* flags, const int32_t* counts, int P, int K, int64_t total_det,
                        const int32_t* max_dets, int M, int T, int A, const double* rec_thrs, int R, void* work,
                        double* precision, double* recall, double* scores, void* stream);

/* ---- COCO error analysis (csrc/coco_error.hip; additive within ABI 8) -------------------------------------------------
 * The matching of tools/analysis_tools/coco_error_analysis.py's 1 + 2 K COCOeval runs in one pass (the definition is
 * restated in mmdet-yolov4_amd/coco_error.py).  Its per-category runs relabel every annotation of c's supercategory
 * ("Sim") or of any other category ("Oth") as category c with ignore = 1 and iscrowd = 1, and keep only c's detections:
 * against the base run only the set of ground truths a detection of c may be matched to changes.  So the problems
 * p = image * K + category, their rank order and det_off are yv4_coco_rank's (with num_at = A * (T + 2); its match_need
 * is not used), and yv4_coco_accumulate follows unchanged with T + 2 in the place of T.  All pointers but `stream` are
 * device pointers; float64 throughout, one IEEE operation per operation of the definition, integer sums.
 *
 * The ground truths are image-major, in annotation order inside an image: image i owns [gt_img_off[i], gt_img_off[i+1]).
 *   gt_box (total_gt, 4) float64 x y w h; gt_area (total_gt) float64; gt_flag (total_gt) bytes: bit 0 = iscrowd,
 *     bit 1 = ignore; gt_cat (total_gt) int32: the K-axis position of the annotation's category, or -1 for a category
 *     outside the K axis (it takes part in the Oth walks only); gt_img_off (P / K + 1) int64.
 *   cat_group (K) int32: the supercategory group of each K-axis position; equal values = same supercategory.
 *
 * yv4_coco_error_need: *need (1) int64 = the doubles of workspace yv4_coco_error_match needs for num_walks =
 *   A * (T + 2) walks with this max_det: the problems whose IoU block (min(num_det, max_det) x the image's gts) exceeds
 *   YV4_COCO_ERROR_LDS_PAIRS doubles, or whose image has more than YV4_COCO_ERROR_LDS_GTS gts.  The caller reads it back.
 *
 * yv4_coco_error_match: one wave per problem that has detections (groups of 64 walks when A * (T + 2) > 64).
 *   The IoU block of the problem's first min(num_det, max_det) detections in rank order against ALL gts of the image is
 *     computed once: the ordinary union by the gt's own crowd bit for a gt with gt_cat == k, union = detection area
 *     (the crowd form) for every other gt.  It sits in LDS up to the two capacities above, else in `work`.
 *   Walks, one per lane, w = a * (T + 2) + t: t < T the base walk at iou_thrs[t] over the gts with gt_cat == k;
 *     t == T the Sim walk at conf_thr over those and the gts with gt_cat >= 0 and cat_group[gt_cat] == cat_group[k];
 *     t == T + 1 the Oth walk at conf_thr over all gts of the image.  A gt of k keeps its own flags and area test; every
 *     other gt is ignored and crowd in every area range.  The walk is yv4_coco_match's: not-ignored gts first, stable in
 *     annotation order (a foreign gt sits among k's own ignored ones in that order), no second pass after a match, a
 *     taken gt is skipped unless crowd, iou < best is skipped, equality passes (the later gt wins).
 *   flags (total_det, A * (T + 2)) bytes, zeroed first: flags[s * A*(T+2) + w], bits as yv4_coco_match's.
 *   counts (K, A) int32, zeroed first: as yv4_coco_match's (only gts with gt_cat == k count; the same in all runs).
 *   work / work_len: at least *need doubles (may be null / 0 when that is 0).  state (2) int64: [1] != 0 afterwards
 *     means the workspace was too small and problems were skipped.
 *   YV4_E_INVALID before anything is launched: a null pointer, A > 64, non-positive sizes, K * A * (T + 2) >= 2^31. */
enum { YV4_COCO_ERROR_LDS_PAIRS = 9216, YV4_COCO_ERROR_LDS_GTS = 512 };   /* the LDS capacities above */
int yv4_coco_error_need(const int64_t* det_off, const int64_t* gt_img_off, int P, int K, int max_det, int num_walks,
                        int64_t* need, void* stream);
int yv4_coco_error_match(const float* det, const uint32_t* order, const int64_t* det_off, const double* gt_box,
                         const double* gt_area, const uint8_t* gt_flag, const int32_t* gt_cat, const int64_t* gt_img_off,
                         const int32_t* cat_group, int P, int K, int64_t total_det, int64_t total_gt, int max_det,
                         const double* iou_thrs, int T, double conf_thr, const double* area_rng, int A, double* work,
                         int64_t work_len, int64_t* state, uint8_t* flags, int32_t* counts, void* stream);

/* ---- VOC-style mAP from the flat result table (csrc/map_flat.hip; additive within ABI 8) ------------------------------
 * The two ends the list path of eval_map leaves to the host: ordering the detections and accumulating tp / fp into
 * recall, precision and AP.  Between them run yv4_bbox_overlaps_batched and yv4_tpfp_batched, unchanged.  N images x C
 * classes give P = C * N problems, class-major: problem p = class * N + image, so a class is one contiguous slice of
 * every table.  All pointers but `stream` are device pointers.  The definition is restated in
 * mmdet-yolov4_amd/map_eval.py; every floating-point value is one IEEE operation of it, counts are integers, and two
 * runs give identical bytes.
 *
 * yv4_map_rank: two stable sorts of the flat table, by (class, descending score) and then by problem.
 *   det (total_det, 5) float32 x1 y1 x2 y2 score, labels / img_index (total_det) int64 in the caller's order.  A row
 *     whose label is outside [0, C) or whose image index is outside [0, N) takes no part.  Dv = the rows that do.
 *     Equal scores (+0 and -0 are equal) keep the caller's order, in both orders below.  Scores are expected finite.
 *   gt_off (P+1) int64: the problems' ground-truth offsets (input).
 *   det4 (total_det, 4) float32, 16-byte aligned: the boxes gathered problem-major, inside a problem in visiting
 *     order (descending score); det_off (P+1) int64 with det_off[P] = Dv.  Rows at and beyond Dv hold the boxes that
 *     take no part.
 *   order, rank (total_det) int32: the tables yv4_tpfp_batched reads.  The boxes already sit in visiting order, so
 *     both hold a position's rank inside its problem.
 *   iou_off (P+1) int64: exclusive sums of num_det * num_gt per problem.
 *   cls_order (total_det) int32: the per-class global order.  Class c owns [det_off[c*N], det_off[(c+1)*N]); entry j
 *     of that slice is the problem-major position (the column of yv4_tpfp_batched's tp / fp) of the class's j-th
 *     detection by descending score.
 *   info (C + 2) int64, for ONE read-back: [0] = iou_off[P] (sizes the IoU buffer), [1] = Dv, [2 + c] = the
 *     detections of class c.
 *   work: yv4_map_rank_work(total_det) bytes, 8-byte aligned.  total_det == 0 is legal: det_off, iou_off and info are
 *     zeroed and nothing else is touched. */
size_t yv4_map_rank_work(int64_t total_det);
int yv4_map_rank(const float* det, const int64_t* labels, const int64_t* img_index, int64_t total_det, int N, int C,
                 const int64_t* gt_off, void* work, float* det4, int64_t* det_off, int32_t* order, int32_t* rank,
                 int64_t* iou_off, int32_t* cls_order, int64_t* info, void* stream);
/* yv4_map_accumulate: mean_ap.py:353-396 and average_precision (:12-58) per (threshold t, class c, area range k).
 *   tp, fp (num_thrs, num_ranges, total_det) bytes as yv4_tpfp_batched wrote them for total_det = Dv columns;
 *   cls_order, det_off: from yv4_map_rank; num_gts (C, num_ranges) int64: the class's regular gts per area range.
 *   Over the class's detections in cls_order: integer cumulative ctp / cfp (a class must hold fewer than 2^24
 *   detections; the caller checks info), recall = float32(ctp) / max(num_gts, float32 eps) in float64, precision =
 *   float32(ctp) / max(float32(ctp) + float32(cfp), float32 eps) in float32.
 *   YV4_MAP_AP_AREA: mrec = [0, recall, 1], mpre = [0, precision, 0] in float64, mpre's suffix maximum, and the sum
 *     of (mrec[i+1] - mrec[i]) * mpre[i+1] over the i with mrec[i+1] != mrec[i], added in ascending i into a single
 *     float64 accumulator, rounded to float32.
 *   YV4_MAP_AP_11POINTS: for the levels j * 0.1 (float64), j = 0 .. 10, the maximum precision among the positions with
 *     recall >= level (0 if none), added in that order in float32, divided by 11 in float32.
 *   ap (num_thrs, C, num_ranges) float32; last_recall float64 / last_precision float32, both (num_thrs, C,
 *     num_ranges): the curves' last points, 0 for a class without detections; num_dets (C) int64.
 *   recall (float64) / precision (float32), both (num_thrs, num_ranges, total_det) or both null: the full curves,
 *     class c's in columns [det_off[c*N], det_off[(c+1)*N]) in cls_order.
 *   work: yv4_map_accumulate_work(total_det, num_thrs, num_ranges) bytes, 4-byte aligned. */
#define YV4_MAP_AP_AREA 0
#define YV4_MAP_AP_11POINTS 1
size_t yv4_map_accumulate_work(int64_t total_det, int num_thrs, int num_ranges);
int yv4_map_accumulate(const uint8_t* tp, const uint8_t* fp, const int32_t* cls_order, const int64_t* det_off,
                       const int64_t* num_gts, int64_t total_det, int N, int C, int num_thrs, int num_ranges, int mode,
                       void* work, float* ap, double* last_recall, float* last_precision, double* recall,
                       float* precision, int64_t* num_dets, void* stream);

/* ---- per-image mAP (csrc/map_image.hip; additive within ABI 8) --------------------------------------------------------
 * tools/analysis_tools/analyze_results.py's bbox_map_eval for every image of a dataset at once: the accumulation of
 * yv4_map_accumulate per PROBLEM p = class * N + image instead of per class, then per image the mean over its classes
 * and over the thresholds.  It follows yv4_map_rank, yv4_bbox_overlaps_batched and yv4_tpfp_batched (num_ranges == 1),
 * unchanged.  All pointers but `stream` are device pointers; every table comes with its element count, checked against
 * N, C, num_thrs, total_det and total_gt on the host before any launch (YV4_E_INVALID, nothing is written).  No float
 * atomics: two runs give identical bytes.  The definition is restated in tests/_image_map_ref.py.
 *
 * yv4_map_image_ap: per problem p and threshold t.
 *   tp, fp (num_thrs, 1, total_det) bytes as yv4_tpfp_batched wrote them for total_det = Dv columns (tpfp_elems >=
 *     num_thrs * total_det); a problem's columns [det_off[p], det_off[p+1]) are already in visiting order.
 *   det_off, gt_off (P+1) int64 (off_elems >= P + 1); gt_ignore (total_gt) bytes.
 *   ngt[p] = the gts of [gt_off[p], gt_off[p+1]) whose gt_ignore byte is 0.
 *   ap[t, p]: yv4_map_accumulate's YV4_MAP_AP_AREA rule over the problem's own detections: integer cumulative ctp /
 *     cfp, recall = float32(ctp) / max(ngt, float32 eps) in float64, precision = float32(ctp) / max(float32(ctp) +
 *     float32(cfp), float32 eps) in float32, mrec = [0, recall, 1], mpre = [0, precision, 0] in float64, mpre's suffix
 *     maximum, the terms (mrec[i+1] - mrec[i]) * mpre[i+1] where recall changes added in ascending i into ONE float64
 *     accumulator, rounded to float32.  A problem without detections scores 0.
 *   ap (num_thrs, P) float32 (ap_elems >= num_thrs * P); ngt (P) int32 (ngt_elems >= P).
 *   work: yv4_map_image_ap_work(total_det) bytes (4 bytes a detection: the thresholds are walked in turn; only
 *     problems of more than 64 detections use it), 4-byte aligned.  total_det == 0 is legal (tp / fp may be null).  An offset outside its table is clamped.
 *
 * yv4_map_image_mean: per image i and threshold t the ap[t, c*N+i] of the classes with ngt[c*N+i] > 0, in ascending c.
 *   image_map_thr[t, i] (num_thrs, N) float32 = their numpy float32 mean: numpy's pairwise sum, then ONE float32
 *     division by the count -- fewer than 8 values: added left to right from 0; 8 to 128: eight accumulators over the
 *     multiples of 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail then added left to right; more: split
 *     at n2 = n / 2, n2 -= n2 % 8, each half by the same rule, the two sums added.  No class with gts: 0.
 *   image_map[i] (N) float64 = (((0 + m_0) + m_1) + .. + m_{T-1}) / T in float64 over the widened image_map_thr[t, i]. */
size_t yv4_map_image_ap_work(int64_t total_det);
int yv4_map_image_ap(const uint8_t* tp, const uint8_t* fp, int64_t tpfp_elems, const int64_t* det_off,
                     const int64_t* gt_off, int64_t off_elems, const uint8_t* gt_ignore, int64_t total_gt,
                     int64_t total_det, int N, int C, int num_thrs, void* work, size_t work_bytes, float* ap,
                     int64_t ap_elems, int32_t* ngt, int64_t ngt_elems, void* stream);
int yv4_map_image_mean(const float* ap, int64_t ap_elems, const int32_t* ngt, int64_t ngt_elems, int N, int C,
                       int num_thrs, double* image_map, int64_t map_elems, float* image_map_thr, int64_t thr_elems,
                       void* stream);

/* ---- proposal recall (csrc/recall.hip; additive within ABI 8) -----------------------------------------------------------
 * mmdet/core/evaluation/recall.py's _recalls for every image and every proposal number of a dataset in ONE launch.  It
 * follows yv4_map_rank called with C = 1 and a zero label column, unchanged: that leaves the boxes image-major, inside
 * an image in descending-score order with equal scores in the caller's order, and det_off.  (For boxes without scores
 * the caller builds the two tables itself.)  All pointers but `prop_nums` and `stream` are device pointers; every table
 * comes with its element count, checked against N, M, T, total_det and total_gt on the host before any launch
 * (YV4_E_INVALID, nothing is written).  No float atomics: two runs give identical bytes.  The definition is restated in
 * tests/_recall_ref.py.
 *
 * yv4_recall_match:
 *   det4 (total_det, 4) float32 and det_off (N+1) int64: image i owns the boxes [det_off[i], det_off[i+1]) in visiting
 *     order; gt4 (total_gt, 4) float32 and gt_off (N+1) int64 likewise (off_elems >= N + 1 for both).  Boxes 16-byte
 *     aligned and expected finite.  An offset outside its table is clamped.
 *   prop_nums (M <= 16) int32 on the HOST, each >= 0, in any order; iou_thrs (T <= 256) float64.
 *   Per image: cols = min(n, prop_nums[M-1]) -- the LAST entry, as recall.py:96 has it.  Per image and k, on the first
 *     c = min(cols, prop_nums[k]) boxes: the IoU block is bbox_overlaps(gts, boxes) of yv4_bbox_overlaps_batched (fp32,
 *     the reference's operation order, `eps`), computed in the kernel and never stored; then G steps (G = the image's
 *     gts), each: every row's maximum with its first-occurrence argmax, the FIRST row holding the largest maximum, that
 *     value recorded, its row and its column set to -1.  With G > c the surplus steps record -1; with c == 0 the G
 *     steps record 0; an image without gts records nothing.
 *   gt_ious (M, total_gt) float32 or null (gt_ious_elems >= M * total_gt): image i's step j at [k, gt_off[i] + j].
 *   counts (M, T) int64 (counts_elems >= M * T), zeroed by the call: counts[k, t] = the recorded values v of row k with
 *     (double)v >= iou_thrs[t].  recall = counts / total_gt is the caller's division.
 *   lds_cap: a pair with G + c <= min(lds_cap, 1280) keeps its boxes and its row state in LDS; a larger pair reads the
 *     boxes from the tables and keeps its state in `work`.  0 selects 1280.  Both forms give the same bytes; nothing is
 *     ever truncated.
 *   work: yv4_recall_work(total_det, total_gt, N, M) bytes, 8-byte aligned (12 bytes per gt and proposal number, one
 *     bit per box and proposal number).  total_det == 0 and total_gt == 0 are legal (det4 / gt4 may then be null). */
size_t yv4_recall_work(int64_t total_det, int64_t total_gt, int N, int M);
int yv4_recall_match(const float* det4, const int64_t* det_off, const float* gt4, const int64_t* gt_off, int64_t off_elems,
                     int N, int64_t total_det, int64_t total_gt, const int32_t* prop_nums, int M, const double* iou_thrs,
                     int T, float eps, int lds_cap, void* work, size_t work_bytes, float* gt_ious, int64_t gt_ious_elems,
                     int64_t* counts, int64_t counts_elems, void* stream);

/* ---- metric='fast-bbox' from the flat result table (csrc/flex_eval.hip; additive within ABI 8) -----------------------
 * mean_ap_flexible.py's eval_map_flexible with IOU2DCoCo, MatcherCoCo and the 'All' + ScaleBreakdown groups
 * (datasets/coco.py:464-496), scored from the flat table without a visit to the host.  The definition, restated in
 * mmdet-yolov4_amd/eval_utils.py:
 *   Input: dets (D, 5) float32, labels (D) int64, img_index (D) int64; the ground truth class-major with B breakdown
 *     rows gt_bkd (B, G) (row 0 'All', then one per scale range; an ignored gt is 0 in every row).
 *   Problems: N images x C classes give P = C * N problems, p = c * N + i, as in yv4_map_rank.  Matching problem
 *     q = p * B + b shares problem p's IoU block and ignores the gts with gt_bkd[b] == 0.
 *   Order: yv4_map_rank's two stable orders; equal scores keep the table's order (the list path's ties follow numpy's
 *     argsort()[::-1]: the one stated difference).
 *   Per class c, breakdown b, threshold t, over the class's detections in cls_order (a detection sits in problem p at
 *     local position d): mg_own = matched[q(p, b)][t][d], mg_last = matched[q(p, B-1)][t][d];
 *     tp = (shared_tp ? mg_last : mg_own) > -1 (shared_tp restates the reference, whose breakdowns share one tp array);
 *     in = mg_own > -1 ? gt_bkd[b][gt_off[p] + mg_own] : (b == 0 || lo_b <= area < hi_b), area = (x2-x1)*(y2-y1) with
 *     each float32 operation rounded on its own and the bounds rounded to float32 once on the host.  A problem without
 *     ground truth matches nothing.
 *   With k the running count of `in` and ctp the running count of `in & tp` (integers): precision = double(ctp) /
 *     double(k), recall = double(ctp) / double(num_gt) (/ 1e-7 when num_gt == 0), both over the `in` positions only.
 *     AP: precision's suffix maximum, then the sum of (recall_m - recall_prev) * envelope_m over the positions where
 *     recall changes (recall_prev starts at 0), added in rank order into a single float64 accumulator, rounded to
 *     float32.  (numpy adds pairwise: the definition's one freedom.)
 *   No float atomics: two runs give identical bytes.  All pointers but `stream` are device pointers.
 *
 * yv4_flex_tables: the Q = P * B problem tables yv4_match_coco_batched reads, from yv4_map_rank's det_off / iou_off
 *   (both P+1): q_det_off[p*B + b] = B * det_off[p] + b * nd[p], q_det_off[Q] = B * det_off[P]; q_iou_off[q] =
 *   iou_off[p], q_iou_off[Q] = iou_off[P].  Both outputs hold Q+1 int64.  The gt-side tables (q_gt_off and the ignore /
 *   crowd flags per (problem, breakdown)) are static per dataset and come from the host.
 * yv4_flex_accumulate: the rule above, one workgroup per (class, breakdown, threshold).
 *   matched: yv4_match_coco_batched's output for the Q problems (B * total_det * num_thrs int32); det4, cls_order,
 *     det_off: from yv4_map_rank, total_det = its Dv; gt_off (P+1) int64; gt_bkd (num_bkd, total_gt) bytes;
 *     num_gt (C, num_bkd) int64; area_bounds (num_bkd - 1, 2) float32 (lo, hi), may be null when num_bkd == 1.
 *   A class must hold fewer than 2^24 detections (the caller checks yv4_map_rank's info).
 *   num_det int64, recall float64 (the last recall, 0 when num_det == 0), ap float32: each (C, num_bkd, num_thrs).
 *   work: yv4_flex_accumulate_work(total_det, num_thrs, num_bkd) bytes, 8-byte aligned.  total_det == 0 is legal and
 *     gives zeros. */
int yv4_flex_tables(const int64_t* det_off, const int64_t* iou_off, int P, int B, int64_t* q_det_off,
                    int64_t* q_iou_off, void* stream);
size_t yv4_flex_accumulate_work(int64_t total_det, int num_thrs, int num_bkd);
int yv4_flex_accumulate(const int32_t* matched, const float* det4, const int32_t* cls_order, const int64_t* det_off,
                        const int64_t* gt_off, const uint8_t* gt_bkd, const int64_t* num_gt, const float* area_bounds,
                        int64_t total_det, int64_t total_gt, int N, int C, int num_bkd, int num_thrs, int shared_tp,
                        void* work, int64_t* num_det, double* recall, float* ap, void* stream);

/* ---- the flat result table of a test loop (csrc/results.hip; additive within ABI 8) ------------------------------------
 * yv4_results_append: append one batch's post-processing output to the flat table yv4_coco_rank takes, in the order
 * of the reference's _det2json (mmdet/datasets/coco.py:179-199): image, then class, then the row order NMS left.
 *   dets (N, max_per_img, 5) float32, labels (N, max_per_img) int32, count (N) int32: the plan's own buffers.
 *   img_index (N) int64: the image's position in the dataset; a negative value skips that row of the batch.
 *   Image n writes min(max(count[n], 0), max_per_img) rows from `base` + the counts of the kept images before it; inside
 *     an image the rows are a stable counting sort by label (rows of one class keep their order: yv4_coco_rank breaks
 *     score ties by position).  Labels are expected in [0, num_classes) and are NOT checked on the device (num_classes
 *     is validated as positive and otherwise documents the contract); any value sorts, none can move a write out of
 *     the image's range.  Rows at or beyond `capacity` are not written: the caller keeps base + total <= capacity.
 *   out_dets (capacity, 5) float32, out_labels (capacity) int64, out_img (capacity) int64.  Rows outside
 *     [base, base + total) are left as they are.  No workspace, no atomics: identical bytes from run to run.
 *   One workgroup per image with the image's labels in LDS: max_per_img <= YV4_RESULTS_MAX_PER_IMG (16 KB of int32
 *     labels of the 160 KB of LDS per workgroup; the reference's configs use 100 to 1000), YV4_E_UNSUPPORTED above it.
 *   YV4_E_INVALID without a launch for N < 0, max_per_img or num_classes <= 0, base < 0, capacity < base or a null
 *     pointer; N == 0 is legal and does nothing. */
#define YV4_RESULTS_MAX_PER_IMG 4096
int yv4_results_append(const float* dets, const int32_t* labels, const int32_t* count, const int64_t* img_index, int N,
                       int max_per_img, int num_classes, int64_t base, int64_t capacity, float* out_dets,
                       int64_t* out_labels, int64_t* out_img, void* stream);

/* ---- split-K form of yv4_conv_bn_act_fwd for single-image (latency) plans ---------------------------------------
 * The reference's only published protocol is batch 1 (tools/analysis_tools/benchmark.py:83-109).  There the deep layers
 * have a handful of output tiles and hundreds of K slices each; this entry splits K over several workgroups per tile
 * (partials in per-split slabs of `workspace`, added in slab order by a finishing kernel that applies the epilogue:
 * deterministic, no atomics).  The summation order differs from yv4_conv_bn_act_fwd's, so the two agree to fp32
 * rounding, not bit for bit.  yv4_conv_splitk_workspace returns the bytes `workspace` must hold (0 and *ksplit = 1
 * when the layer is not split: the call then forwards to yv4_conv_bn_act_fwd). */
size_t yv4_conv_splitk_workspace(const yv4_conv_desc* d, int* ksplit);
int yv4_conv_bn_act_fwd_splitk(const yv4_conv_desc* d, const float* x, const float* w, const float* scale1,
                               const float* shift1, const float* scale2, const float* shift2,
                               const float* residual, float* y, float* workspace, size_t workspace_bytes,
                               void* stream);

/* The same for 16-bit operands (yv4_conv_bn_act_fwd_h16): 64 x 64 tiles, K slices of 64, fp32 partial slabs, a finishing
 * kernel with the 16-bit tiles' epilogue expressions (16-bit or fp32 output).  Layers outside the uniform-K tiles
 * (Cin % 64 != 0) are not split: the call forwards to yv4_conv_bn_act_fwd_h16. */
size_t yv4_conv_h16_splitk_workspace(const yv4_conv_desc* d, int* ksplit);
int yv4_conv_bn_act_fwd_h16_splitk(const yv4_conv_desc* d, int dtype, int out_dtype, const void* x, const void* w,
                                   const float* scale1, const float* shift1, const float* scale2,
                                   const float* shift2, const void* residual, void* y, float* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- train-side input pipeline (configs/yolov4/yolov4l_coco_mosaic.py:22-69) ----------------------------------
 * Replaces, per batch: Resize(keep_ratio) of 4 source images + MosaicPipeline (mmdet/datasets/pipelines/
 * transforms.py:1906-1983) + the Albu block [PadIfNeeded, RandomCrop, RandomScale, CenterCrop, HorizontalFlip]
 * (albumentations, third party) + HueSaturationValueJitter (transforms.py:1986-2021) + GtBBoxesFilter
 * (transforms.py:2024-2052) + Normalize + ImageToTensor/collate, which the reference runs in CPU dataloader workers.
 * One yv4_aug_image per OUTPUT image describes its four sources and the random draws (made by the host):
 *   src[i], sh/sw/pitch[i]  decoded 8-bit BGR source i (HWC, 3 channels, device memory), i = mosaic tile
 *                           (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right, transforms.py:1943-1951)
 *   rh/rw[i]                its size after Resize (mmcv rescale_size)
 *   cxy                     mosaic centre = max(rh[0], rh[1], rw[0], rw[2]) (transforms.py:1934); canvas is 2cxy x 2cxy
 *   left, top               PadIfNeeded offsets; x1, y1 RandomCrop origin in the padded canvas; C crop size (1280)
 *   S                       size of the crop after RandomScale (int(C * scale)); o = (S - out) / 2 CenterCrop origin
 *   flip                    HorizontalFlip applied; hsv_on + lut[3][256]: the hue / saturation / value LUTs of
 *                           transforms.py:2004-2008 for this image's random gains. */
typedef struct {
  const void* src[4];
  int32_t sh[4], sw[4], pitch[4];
  int32_t rh[4], rw[4];
  int32_t cxy, left, top, x1, y1, C, S, o, flip, hsv_on;
  uint8_t lut[3][256];
} yv4_aug_image;

/* Pixels of N output images (out_size x out_size).  imgs: N descriptors in DEVICE memory.  out_u8 (optional):
 * (N, out, out, 3) 8-bit BGR image after the geometric chain, before the colour jitter; out_nchw (optional):
 * (N, 3, out, out) fp32 after jitter + (v - mean) * (1 / std) with the BGR -> RGB swap of to_rgb. */
int yv4_mosaic_augment_u8(const yv4_aug_image* imgs, int N, int out_size, uint8_t* out_u8, float* out_nchw,
                          const float* mean3, const float* std3, int to_rgb, int pad_val, void* stream);

/* Boxes of the same N output images.  boxes (total, 4) pascal_voc in SOURCE image coordinates, labels / tile (total,)
 * (tile = which of the 4 sources the box belongs to), seg (N + 1) ranges.  Per box: Resize scale + clip (float32),
 * mosaic shift, the Albu chain in float64 with its BboxParams filter (clipped area > min_area, clipped / unclipped
 * area > min_visibility), GtBBoxesFilter (w, h > min_size, aspect ratio < max_aspect_ratio).  Survivors are written in
 * input order to out_boxes (N, cap, 4) / out_labels (N, cap), their number (<= cap) to out_count (N). */
int yv4_augment_boxes(const yv4_aug_image* imgs, int N, int out_size, const float* boxes, const int32_t* labels,
                      const int32_t* tile, const int64_t* seg, int cap, double min_area, double min_visibility,
                      float min_size, float max_aspect_ratio, float* out_boxes, int32_t* out_labels,
                      int32_t* out_count, void* stream);

/* ---- FP8 (OCP e4m3fn) inference (csrc/conv_f8.hip) ------------------------------------------------------------------
 * A code is e4m3(clamp(v * inv_s, -448, 448)), rounded to nearest even; NaN is never produced.  Activations carry one fp32
 * scale s per buffer (inv_s = 1/s computed by the caller), weights one per output channel.
 *
 * Fused conv with e4m3 operands and fp32 accumulation (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales).  x and w
 * are e4m3 codes: x an NHWC view, w (Cout, KH*KW*Cin) in (kh, kw, ci) order.  The dequantization is the caller's
 * business: scale1 = s1 * sw[co] * sx (folded in double, rounded to fp32).  Epilogue:
 *   v = act1(acc * scale1 + shift1);  v += residual * r_scale (e4m3 view);  v = act2(v * scale2 + shift2) (optional);
 *   y = out_dtype == YV4_F8E4M3 ? e4m3(clamp(v * y_inv_scale, +-448)) : v (fp32).
 * Cin and the input view's cstride / coff must be multiples of 16 (YV4_E_UNSUPPORTED otherwise); output and residual
 * views may sit at any channel offset.  desc->tile: YV4_TILE_AUTO or one of YV4_F8TILE_*. */
#define YV4_F8TILE_128x128 1
#define YV4_F8TILE_128x64 2
#define YV4_F8TILE_64x64 3
int yv4_conv_bn_act_fwd_f8(const yv4_conv_desc* d, int out_dtype, const void* x, const void* w, const float* scale1,
                           const float* shift1, const float* scale2, const float* shift2, const void* residual,
                           float r_scale, float y_inv_scale, void* y, void* stream);
/* The tile YV4_TILE_AUTO resolves to for this descriptor. */
int yv4_conv_f8_pick_tile(const yv4_conv_desc* d);
/* x: an NHWC view of dtype YV4_F32 / YV4_F16 / YV4_BF16 -> y: an e4m3 view of the same shape, y = e4m3(clamp(x *
 * inv_scale, +-448)).  C, strides and offsets must be multiples of 4. */
int yv4_quantize_f8(const void* x, int dtype, int N, int H, int W, int C, int x_cstride, int x_coff, void* y,
                    int y_cstride, int y_coff, float inv_scale, void* stream);
/* SPP on e4m3 codes: as yv4_spp_pool_fwd_h16 (channels [coff, coff+C) -> mp5 / mp9 / mp13 into the next three C-channel
 * slots of the same buffer), codes compared in sign-magnitude order: the max is exact.  C, cstride, coff % 4 == 0. */
int yv4_spp_pool_fwd_f8(void* buf, int N, int H, int W, int C, int cstride, int coff, void* stream);

/* ---- test-time augmentation of YOLOV3Head (csrc/tta.hip, csrc/preprocess.hip) -------------------------------------
 * Flip codes of MultiScaleFlipAug's flip_direction (datasets/pipelines/test_time_aug.py; bit 0 mirrors x, bit 1 y). */
#define YV4_FLIP_NONE 0
#define YV4_FLIP_HORIZONTAL 1
#define YV4_FLIP_VERTICAL 2
#define YV4_FLIP_DIAGONAL 3
/* Largest number of augmentations one yv4_tta_merge call takes. */
#define YV4_TTA_MAX_AUGS 16

/* yv4_letterbox_u8 followed by RandomFlip of the RESIZED (new_h x new_w) image (transforms.py RandomFlip with
 * mmcv.imflip, between Resize and Normalize / Pad in configs/yolo/yolov3_d53_*): a permutation of the unflipped
 * output's resized region, bit for bit; the pad region is unchanged.  flip: YV4_FLIP_*. */
int yv4_letterbox_u8_flip(const uint8_t* src, int src_h, int src_w, int src_pitch, float* dst, int Hp, int Wp,
                          int64_t plane_stride, int new_h, int new_w, const float* mean3, const float* std3,
                          int to_rgb, int pad_val, int pad_before_normalize, int flip, void* stream);

/* ---- a whole test batch in one launch (csrc/preprocess.hip; additive within ABI 8) --------------------------------
 * One entry per output slot, that is per (augmentation, image) of a MultiScaleFlipAug batch:
 *   src, src_h, src_w,      the 8-bit HWC source in DEVICE memory and its row pitch in bytes (>= 3 * src_w: a view
 *   src_pitch               inside a wider canvas is taken where it lies)
 *   new_h, new_w            the resized extent (Resize(keep_ratio=True))
 *   pad_h, pad_w            the image's own padded extent (Pad(size_divisor)); new <= pad <= canvas
 *   H, W                    the slot's canvas: what collate pads every image of its batch to.  Canvases differ between
 *                           the scales of a pipeline, so one table covers all of them
 *   flip                    YV4_FLIP_* of the resized region
 *   dst_off                 where the slot's 3 * H * W floats (planar C, H, W) begin in dst, in floats
 *   inv_sx, inv_sy          the resize ratios, computed on the host with yv4_letterbox_u8's expression:
 *                           1.0 / ((double)new_w / (double)src_w) and 1.0 / ((double)new_h / (double)src_h) */
typedef struct yv4_letterbox_slot {
  const uint8_t* src;
  double inv_sx, inv_sy;
  int64_t dst_off;
  int32_t src_h, src_w, src_pitch;
  int32_t new_h, new_w;
  int32_t pad_h, pad_w;
  int32_t H, W;
  int32_t flip;
} yv4_letterbox_slot;

/* yv4_letterbox_u8_flip for N slots in ONE launch on `stream`, the batch's collate included: every element of every
 * slot is written -- inside new_h x new_w the interpolated pixel, from there to pad_h x pad_w the pad value (normalised
 * if pad_before_normalize), from there to H x W 0.0f (collate pads after Normalize) -- so dst needs no zero fill, and
 * every element is bit-equal to yv4_letterbox_u8_flip into a (pad_h, pad_w) image placed in a zeroed canvas.  table:
 * the HOST table, validated here (every slot by yv4_letterbox_u8's checks; pad_h <= H, pad_w <= W; the ratios equal
 * the expression above; dst_off >= 0 and dst_off + 3*H*W <= dst_elems; N <= 65535: YV4_E_INVALID before the launch);
 * table_dev: the same N entries in DEVICE memory (8-byte aligned), which the kernel trusts.  A slot whose W is a
 * multiple of 4 and whose first float is 16-byte aligned is written with 16-byte stores, four x a thread; any other
 * slot one float at a time.  Slots that overlap in dst are the caller's error. */
int yv4_letterbox_u8_batch(const yv4_letterbox_slot* table, const yv4_letterbox_slot* table_dev, int N, float* dst,
                           int64_t dst_elems, const float* mean3, const float* std3, int to_rgb, int pad_val,
                           int pad_before_normalize, void* stream);

/* Slot tables of YOLOV3Head.get_bboxes(with_nms=False) (yolo_head.py:254-311): per image, the levels' boxes in the
 * reference's concatenation order.  A level of n_l = H_l*W_l*A boxes contributes k_l = nms_pre slots when
 * 0 < nms_pre < n_l (conf.topk(nms_pre), sorted: descending objectness, ties to the lower anchor index), else n_l
 * slots in anchor order.  slots (N, S) int32, S = sum_l k_l: slots[n*S + s] = anchor index within the image (what
 * yv4_decode_filter_v3's boxes / conf / cls rows are indexed by).  conf: (N, total_anchors) objectness from
 * yv4_decode_filter_v3; level_anchors: num_levels HOST values n_l; topk_keys: (N*num_levels) admission keys of
 * yv4_conf_topk_levels (required when some level is cut, else may be NULL).  Levels with k_l <= 8192 sort in LDS;
 * larger ones use the library's radix sort in `work` (yv4_topk_slots_work bytes, 0 when none is needed). */
size_t yv4_topk_slots_work(int num_levels, const int32_t* level_anchors, int nms_pre);
int yv4_topk_slots(const float* conf, int N, int64_t total_anchors, int num_levels, const int32_t* level_anchors,
                   int nms_pre, const uint64_t* topk_keys, void* work, int32_t* slots, int64_t S, void* stream);

/* One augmentation of yv4_tta_merge: image n of the batch reads boxes + n*total*4, conf + n*total,
 * cls + n*total*num_classes (yv4_decode_filter_v3 with scale_factor NULL) and slots + n*S (yv4_topk_slots). */
typedef struct yv4_tta_aug {
  const float* boxes;
  const float* conf;
  const float* cls;
  const int32_t* slots;
  int64_t total;
  int32_t S;
  int32_t flip;         /* YV4_FLIP_* */
} yv4_tta_aug;

/* Merge of BBoxTestMixin.aug_test_bboxes (dense_test_mixins.py:38-100) up to multiclass_nms, for N images at once.
 * Merged slot m of image n = (augmentation a, slot s) in augmentation order, m = sum_{a'<a} S_a' + s.  Per slot:
 * bbox_mapping_back (core/bbox/transforms.py:5-55): bbox_flip over that augmentation's img_shape, then / scale_factor
 * (fp32, in that order) -> boxes_out[n][m]; per class c with cls > score_thr the key
 * (~order(cls * conf) << 32 | (m*num_classes + c)) is appended to keys[n*key_cap ...] and the mapped box folded into
 * max_coord[n] -- the buffers yv4_nms_images / yv4_nms_split take with fused_classes = num_classes and
 * boxes_per_image = S_total.  meta: device (num_augs, N, 6) fp32 rows img_h, img_w, scale_factor[4].
 * counts / max_coord must be reset by yv4_decode_reset first.  augs: num_augs HOST descriptors.
 * If more than key_cap candidates pass for an image the count keeps counting (so the caller can see the overflow) but
 * keys beyond the capacity are dropped. */
int yv4_tta_merge(const yv4_tta_aug* augs, int num_augs, int N, int num_classes, float score_thr, const float* meta,
                  float* boxes_out, uint64_t* keys, int64_t key_cap, int32_t* counts, float* max_coord, void* stream);

/* ---- train-side input pipeline of the YOLOv3 mstrain recipe (csrc/augment_v3.hip; additive within ABI 8) -----------
 * configs/yolo/yolov3_d53_mstrain-608_273e_coco.py:59-78: PhotoMetricDistortion -> Expand -> MinIoURandomCrop ->
 * Resize(keep_ratio) -> RandomFlip -> Normalize -> Pad(size_divisor) -> collate, the pixels of a batch in one launch.
 * One yv4_v3aug_image per OUTPUT image carries its source and the host's draws (the draws, MinIoURandomCrop's acceptance
 * loop and the boxes stay on the host).  The float pixel definitions are stated in csrc/augment_v3.hip.
 *   src, sh, sw, pitch      decoded 8-bit BGR source (HWC, 3 channels, device memory), row pitch in bytes
 *   bright_on/_delta        random brightness: v += delta
 *   contrast_mode/_alpha    YV4_V3AUG_CONTRAST_*: v *= alpha before BGR -> HSV (the reference's mode 1), after HSV -> BGR
 *                           (mode 0), or not at all
 *   sat_on/_alpha           S *= alpha, unclipped; hue_on/_delta: H += delta, then > 360 -> -360, < 0 -> +360
 *   perm_on, perm[3]        channel permutation: out[c] = in[perm[c]]
 *   eh, ew, etop, eleft     Expand's canvas and the offsets of the image in it (sh, sw, 0, 0 when Expand is skipped);
 *   fill[3]                 its fill value per channel, not distorted
 *   cx, cy, cw, ch          MinIoURandomCrop's patch in the canvas (0, 0, ew, eh when the image is returned unchanged)
 *   rh, rw                  size after Resize; ph, pw: after Pad (informative: everything outside rh x rw is written 0)
 *   flip                    YV4_FLIP_* of the resized region */
#define YV4_V3AUG_CONTRAST_NONE 0
#define YV4_V3AUG_CONTRAST_FIRST 1
#define YV4_V3AUG_CONTRAST_LAST 2
typedef struct yv4_v3aug_image {
  const void* src;
  int32_t sh, sw, pitch;
  int32_t bright_on, contrast_mode, sat_on, hue_on, perm_on;
  float bright_delta, contrast_alpha, sat_alpha, hue_delta;
  int32_t perm[3];
  int32_t eh, ew, etop, eleft;
  float fill[3];
  int32_t cx, cy, cw, ch;
  int32_t rh, rw, ph, pw;
  int32_t flip;
  int32_t reserved;
} yv4_v3aug_image;

/* Pixels of N output images into out_nchw (N, 3, Hmax, Wmax) fp32: image n's resized region at the top left, zeros
 * elsewhere (Pad and the collate's padding to the batch maximum).  imgs: N descriptors in DEVICE memory; mean3 / std3:
 * HOST values.  Returns YV4_E_INVALID (-1) on null pointers, N / Hmax / Wmax <= 0 or a zero std before touching the
 * device.  A tap outside the placed source reads the fill value, and stores are bounded by Hmax x Wmax, whatever the
 * descriptors say. */
int yv4_v3_augment_u8(const yv4_v3aug_image* imgs, int N, float* out_nchw, int Hmax, int Wmax, const float* mean3,
                      const float* std3, int to_rgb, void* stream);

/* ---- baseline JPEG decoding (csrc/jpeg_host.cpp, csrc/jpeg.hip; additive within ABI 8) -----------------------------
 * A hybrid decoder with the quantised coefficients as the seam: the host parses the file and runs the Huffman decode
 * (yv4_jpeg_parse / yv4_jpeg_entropy_decode make no HIP call and work without a GPU); the device dequantises, runs
 * libjpeg's "islow" integer IDCT, the fancy chroma upsampling and the integer YCbCr conversion, and writes interleaved
 * 8-bit pixels (yv4_jpeg_reconstruct, a whole batch of images of different sizes and samplings in one call).  The
 * arithmetic is libjpeg-turbo's default decode (JDCT_ISLOW, do_fancy_upsampling), so the pixels equal what cv2.imdecode,
 * turbojpeg and Pillow return, bit for bit.  EXIF orientation is read by the parse (yv4_jpeg_info.orientation) and
 * applied by the pixel stage only where the caller asks for it (yv4_jpeg_layout_oriented); yv4_jpeg_layout never does.
 *
 * Accepted: 8-bit SOF0 / SOF1 Huffman files with one interleaved scan; 1 component, or 3 components (YCbCr) with luma
 * sampling 1x1, 2x1 or 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0); 8-bit quantisation tables.  Progressive, arithmetic,
 * lossless, 12-bit, 4-component / CMYK, RGB-tagged, 16-bit-table, otherwise-sampled and multi-scan files return
 * YV4_E_UNSUPPORTED; malformed input (truncation, a code in no table, a coefficient index past 63, a missing table,
 * zero dimensions, more entropy-coded data than the header's MCUs) returns YV4_E_INVALID.  yv4_last_error names the
 * reason.  Every read is bounds-checked against len: no input makes the host half read or write outside its buffers.
 *
 * yv4_jpeg_info (filled by the host half):
 *   width, height, ncomp    image size in pixels; 1 or 3 components
 *   hs, vs                  sampling factors per component (a single component counts as 1x1, as libjpeg treats it)
 *   tq, td, ta              quantisation / DC Huffman / AC Huffman table selectors per component
 *   restart_interval        MCUs between RSTn markers, 0: none
 *   mcus_x, mcus_y          MCU grid; an MCU is (8 * hs[0]) x (8 * vs[0]) pixels
 *   blocks_w, blocks_h      8x8 blocks per component on the MCU-padded grid
 *   ncoef                   coefficients of the image: 64 * sum(blocks_w * blocks_h)
 *   orientation             EXIF tag 0x0112 of the first APP1 segment that begins "Exif\0\0": 1 .. 8 when IFD0 holds it as
 *                           one SHORT, 0 otherwise (no such segment, a short or inconsistent one, an offset outside it,
 *                           another type, count or value) -- never an error
 *   scan_offset             byte offset of the entropy-coded data
 *   quant                   the four quantisation tables in natural (row-major) order; zero where not defined
 * Coefficient layout: int16, natural order, 64 per block; each component is its own plane of blocks, block-row-major
 * over the MCU-padded grid, component 0 first. */
typedef struct yv4_jpeg_info {
  int32_t width, height, ncomp;
  int32_t hs[3], vs[3];
  int32_t tq[3], td[3], ta[3];
  int32_t restart_interval;
  int32_t mcus_x, mcus_y;
  int32_t blocks_w[3], blocks_h[3];
  int32_t orientation;
  int64_t ncoef;
  int64_t scan_offset;
  uint16_t quant[4][64];
} yv4_jpeg_info;

/* Parse the markers up to and including SOS into info.  Returns YV4_OK, YV4_E_UNSUPPORTED or YV4_E_INVALID. */
int yv4_jpeg_parse(const uint8_t* data, size_t len, yv4_jpeg_info* info);

/* Parse, then Huffman-decode the scan into coef (HOST memory, capacity coef_capacity int16 elements; pinned memory is
 * what an upload wants).  The first info->ncoef elements are zero-filled by the call and then written; YV4_E_CAPACITY
 * when coef_capacity < info->ncoef (info is filled, nothing is written to coef).  On YV4_E_INVALID the coefficients
 * decoded so far stay in the buffer. */
int yv4_jpeg_entropy_decode(const uint8_t* data, size_t len, yv4_jpeg_info* info, int16_t* coef, int64_t coef_capacity);

/* One image of a reconstruct call.  yv4_jpeg_layout fills a dense table; the caller may then place the outputs
 * elsewhere (out_off, out_pitch).
 *   coef_off                first coefficient of the image in the batch's coefficient buffer (int16 elements, % 64 == 0)
 *   plane_off               byte offset of each component's 8-bit plane (blocks_w * 8 wide, blocks_h * 8 high) in the
 *                           workspace (% 8 == 0)
 *   out_off, out_pitch      byte offset of the image's first pixel in the output buffer and its row pitch (>= 3 * width)
 *   unit_base, tile_base    work units of the images before this one: ceil(blocks / 32) IDCT units and
 *                           ceil(width / 256) * ceil(height / 4) pixel tiles per image (none for an image with
 *                           orientation 2 .. 8: those are written by a launch of their own)
 *   width .. blocks_h       as in yv4_jpeg_info: the DECODED picture D, height x width
 *   orientation             the EXIF orientation to apply, 0 or 1: none.  The output O is width x height for 2 .. 4 and
 *                           height x width (height pixels a row, width rows) for 5 .. 8, and out_pitch counts against O's
 *                           row.  With h = height, w = width:
 *                             2  O[y,x] = D[y, w-1-x]        5  O[y,x] = D[x, y]
 *                             3  O[y,x] = D[h-1-y, w-1-x]    6  O[y,x] = D[h-1-x, y]
 *                             4  O[y,x] = D[h-1-y, x]        7  O[y,x] = D[h-1-x, w-1-y]
 *                                                            8  O[y,x] = D[x, w-1-y] */
typedef struct yv4_jpeg_image {
  int64_t coef_off;
  int64_t plane_off[3];
  int64_t out_off;
  int64_t unit_base, tile_base;
  int32_t out_pitch;
  int32_t width, height, ncomp;
  int32_t hs, vs;
  int32_t tq[3];
  int32_t blocks_w[3], blocks_h[3];
  int32_t orientation;
} yv4_jpeg_image;

/* Host only: the dense table of N parsed images -- coefficients back to back, planes 256-byte aligned in the
 * workspace, outputs at pitch 3 * width and 256-byte aligned offsets.  totals[0..2]: coefficient elements, workspace
 * bytes, output bytes of the batch. */
int yv4_jpeg_layout(const yv4_jpeg_info* infos, int N, yv4_jpeg_image* table, int64_t* totals);

/* yv4_jpeg_layout with EXIF orientation: where apply != 0, image n's yv4_jpeg_info.orientation goes into the table and
 * its output is laid out as the oriented picture (pitch 3 * height for 5 .. 8).  apply == 0 is yv4_jpeg_layout. */
int yv4_jpeg_layout_oriented(const yv4_jpeg_info* infos, int N, int apply, yv4_jpeg_image* table, int64_t* totals);

/* Coefficients -> pixels for N images in two launches on `stream`, and one more for every image whose orientation is
 * 2 .. 8 (32 x 32 pixel tiles turned through LDS).  table: the HOST table, validated here against
 * coef_elems / work_bytes / out_bytes (YV4_E_INVALID before any launch); table_dev: the same N entries in DEVICE memory,
 * which the kernels trust.  coef (N images' int16 coefficients), quant ((N, 4, 64) uint16, image n's yv4_jpeg_info.quant),
 * work and out are DEVICE memory; coef and quant 16-byte, work 8-byte aligned.  Pixels are interleaved (h, w, 3): B, G, R
 * (what cv2 and mmcv.imread return), or R, G, B with rgb != 0; one component is written three times.  Bytes of out that
 * are no pixel of an image are not touched. */
int yv4_jpeg_reconstruct(const yv4_jpeg_image* table, const yv4_jpeg_image* table_dev, int N, const int16_t* coef,
                         int64_t coef_elems, const uint16_t* quant, uint8_t* work, int64_t work_bytes, uint8_t* out,
                         int64_t out_bytes, int rgb, void* stream);

/* ---- the Huffman scan on the device (csrc/jpeg_entropy_core.h, csrc/jpeg_entropy_host.cpp, csrc/jpeg_entropy.hip;
 * additive within ABI 8) --------------------------------------------------------------------------------------------
 * The other side of the coefficient seam: the same files yv4_jpeg_entropy_decode accepts, the same coefficients, decoded
 * by a kernel from the file's bytes.  The unit of parallelism is the SEGMENT: a run of whole MCUs whose bytes start on
 * a byte boundary in the initial state (DC predictors zero, first block of an MCU).  A file with a restart interval
 * has one segment per interval, any other file is one segment.  Segments are independent: one lane decodes one segment,
 * a workgroup is one wave of 64 lanes over up to 64 consecutive segments of ONE image, with that image's Huffman
 * tables in LDS.  yv4_jpeg_reconstruct, yv4_jpeg_layout and yv4_jpeg_image are unchanged.
 *
 * A batch is described by four tables, each built on the host and copied to the device:
 *   yv4_jpeg_scan      one per image: where its file lies in the batch's bytes, where its coefficients go, its MCU grid,
 *                      its slice of the segment table and of the packed Huffman tables
 *   yv4_jpeg_segment   byte range WITHIN THE FILE [begin, end), first MCU and MCU count.  bit_off and pred (a bit offset
 *                      into the first byte and carried-in DC predictors) were meant for entry points inside a segment;
 *                      those live in yv4_jpeg_entry instead ("self-synchronising chunks" below): they must be zero
 *   yv4_jpeg_wg        one per workgroup: image, first segment (within the image) and count (1 .. 64)
 *   yv4_jpeg_huff      one packed Huffman table: the 9-bit lookahead (code length << 8 | symbol, 0: a longer code), the
 *                      largest code and the value offset of each length 10 .. 16 (-1: no code of that length), the values
 * A lane that meets an error stores its code into the image's status word (atomic max, so the outcome is the same on
 * every run) and stops; the other segments go on.  YV4_JPEG_ERR_TRAILING: at least 8 real bits are left after a
 * segment's last MCU -- data where a restart marker is due or, behind the last segment, more entropy-coded data than
 * the header's MCUs. */
#define YV4_JPEG_MAX_HUFF 6            /* tables one image can reference: 3 DC + 3 AC */
#define YV4_JPEG_WG_SEGMENTS 64        /* segments per workgroup */
#define YV4_JPEG_ERR_OVERRUN 1         /* a block whose decode reached past the end of its segment's bytes */
#define YV4_JPEG_ERR_CODE 2            /* a code that is in no table */
#define YV4_JPEG_ERR_DC_CATEGORY 3     /* a DC magnitude category above 11 */
#define YV4_JPEG_ERR_INDEX 4           /* a coefficient index past 63 */
#define YV4_JPEG_ERR_TRAILING 5        /* data where a restart marker or the end of the scan is due */

typedef struct yv4_jpeg_huff {
  uint16_t look[512];
  int32_t maxcode[8];       /* [l - 10] for code lengths 10 .. 16; [7] unused */
  int32_t valoff[8];
  uint8_t vals[256];
} yv4_jpeg_huff;

typedef struct yv4_jpeg_scan {
  int64_t data_off, data_len;      /* the file in the batch's bytes */
  int64_t coef_off, ncoef;         /* the image's coefficients in the batch's buffer (int16 elements) */
  int64_t seg_base;                /* its first entry in the segment table */
  int32_t nseg;
  int32_t ncomp, mcus_x, mcus_y;
  int32_t hs, vs;                  /* luma sampling; chroma is 1x1 */
  int32_t td[3], ta[3];            /* per component: index of its DC / AC table among the image's packed tables */
  int32_t huff_base, nhuff;        /* its first packed table and their number (1 .. YV4_JPEG_MAX_HUFF) */
} yv4_jpeg_scan;

typedef struct yv4_jpeg_segment {
  int64_t begin, end;
  int32_t first_mcu, mcu_count;
  int32_t bit_off;
  int32_t reserved;
  int16_t pred[4];
} yv4_jpeg_segment;

typedef struct yv4_jpeg_wg {
  int32_t image, first_seg, count, reserved;
} yv4_jpeg_wg;

/* Host only, no HIP call: parse the headers (as yv4_jpeg_parse: the same YV4_E_UNSUPPORTED / YV4_E_INVALID), pack the
 * Huffman tables the scan references into huff (room for YV4_JPEG_MAX_HUFF) and walk the entropy-coded bytes once for
 * markers into the segment table segs (room for seg_capacity).  The rules are the host decoder's at a restart: RSTn in
 * order modulo 8, 0xFF fill bytes before a marker allowed, ceil(MCUs / interval) - 1 markers; a marker that is missing
 * or out of order, and an RSTn behind the last segment, are YV4_E_INVALID.  scan comes back with data_off, coef_off,
 * seg_base and huff_base zero for the caller to place, and scan->nseg = restart_interval ? ceil(MCUs / interval) : 1
 * is set before the capacity check (YV4_E_CAPACITY: nothing is written to segs). */
int yv4_jpeg_scan_prepare(const uint8_t* data, size_t len, yv4_jpeg_info* info, yv4_jpeg_scan* scan, yv4_jpeg_huff* huff,
                          yv4_jpeg_segment* segs, int64_t seg_capacity);

/* Host only: the workgroup table of N placed images -- image n's segments in runs of YV4_JPEG_WG_SEGMENTS, images in
 * order.  *count is the number of workgroups; with wgs NULL only the count is made, else YV4_E_CAPACITY if it exceeds
 * wg_capacity. */
int yv4_jpeg_entropy_workgroups(const yv4_jpeg_scan* scans, int N, yv4_jpeg_wg* wgs, int64_t wg_capacity, int64_t* count);

/* Host only: the decode the kernel runs, over the same tables, on the CPU.  Validates like
 * yv4_jpeg_entropy_decode_device, zero-fills the batch's coefficient range and status[0 .. N), decodes every segment and
 * leaves the largest YV4_JPEG_ERR_* code of each image (0: none) in status.  All pointers are HOST memory. */
int yv4_jpeg_entropy_decode_segments(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs,
                                     int N, int64_t nseg, int64_t nwg, const uint8_t* bytes, int64_t bytes_len,
                                     const yv4_jpeg_huff* huff, int64_t nhuff, int16_t* coef, int64_t coef_elems,
                                     int32_t* status);

/* The Huffman decode of N images in one launch on `stream`.  scans / segs / wgs: the HOST tables, validated here against
 * nseg, nwg, bytes_len, nhuff and coef_elems (every offset and count, the MCU ranges, the workgroup runs; YV4_E_INVALID
 * before any launch); scans_dev / segs_dev / wgs_dev: the same entries in DEVICE memory (8-byte aligned), which the
 * kernel trusts.  bytes (the files), huff (4-byte aligned), coef and status (N int32) are DEVICE memory.  The call
 * zero-fills the batch's coefficient range and status on the stream, then launches; afterwards status[n] is 0 or
 * image n's largest YV4_JPEG_ERR_* code, and coef feeds yv4_jpeg_reconstruct as the host decoder's output does.  No
 * read leaves a segment's bytes and no store an image's coefficient range, whatever the bytes hold. */
int yv4_jpeg_entropy_decode_device(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs,
                                   const yv4_jpeg_scan* scans_dev, const yv4_jpeg_segment* segs_dev,
                                   const yv4_jpeg_wg* wgs_dev, int N, int64_t nseg, int64_t nwg, const uint8_t* bytes,
                                   int64_t bytes_len, const yv4_jpeg_huff* huff, int64_t nhuff, int16_t* coef,
                                   int64_t coef_elems, int32_t* status, void* stream);

/* The reason behind a YV4_JPEG_ERR_* code, as static text. */
const char* yv4_jpeg_entropy_strerror(int code);

/* ---- self-synchronising chunks: many lanes per segment (additive within ABI 8) ------------------------------------------
 * A file without restart markers is one segment, hence one lane above.  Here every segment's bytes [begin, end) are cut
 * into CHUNKS of chunk_bytes raw bytes (stuffed bytes included; an empty segment is one empty chunk) and one lane
 * decodes one chunk.  A coded symbol -- a Huffman code and its magnitude bits -- belongs to the chunk in which its first
 * bit lies.  The decoder state at a symbol boundary is one word:
 *     (bit position in the file: byte * 8 + bit) << 16 | block index within the MCU << 8 | zigzag index k
 * with k = 0 for "a DC symbol is next"; the position's byte is never the 0x00 of a stuffed 0xFF00 pair.
 *   1. sync     Chunk 0 of a segment starts in the true state, every other chunk from a guess (its first bit, block 0,
 *               k = 0).  A lane decodes, storing nothing, up to the first symbol that starts at or behind its chunk's
 *               end and records that exit state, the blocks it completed and per component the sum of the DC
 *               differences modulo 2^16.  In each of max_rounds further rounds a chunk whose predecessor's exit differs
 *               from the entry it was decoded from is decoded again from that exit.  Errors met on the way say only
 *               that the entry was wrong.
 *   2. proof    A segment's chain is accepted only if, for every chunk c > 0, the exit of chunk c - 1 EQUALS the entry
 *               chunk c was last decoded from.  Chunk 0's entry is true, so by induction an accepted chain is the
 *               sequential decode.  Exclusive sums over the chain give each chunk's first block ordinal and DC
 *               predictors; the entry's block index must be that ordinal modulo the blocks per MCU, the segment's
 *               total mcu_count times the blocks per MCU, and the last chunk must end on a block boundary with fewer
 *               than 8 real bits left.
 *   3. decode   One lane per chunk decodes again from its proven entry and stores DC and nonzero AC terms into the
 *               zero-filled planes.  A block that straddles a chunk's end is finished by the next lane.
 * An image with any chain not accepted, any check failed or any error inside an accepted chain is UNDECIDED: its word
 * in `undecided` is nonzero, its coefficients are unspecified, and the caller decodes it again with the one lane per
 * segment decode above, which alone decides status codes.  The chunk decode never raises status.
 *
 * chunk_bytes: YV4_JPEG_MIN_CHUNK_BYTES .. YV4_JPEG_MAX_CHUNK_BYTES.  The reader's look-back is one byte and is guarded
 * by the segment's begin, so it sets no floor; 4 keeps a chunk no smaller than the longest symbol (31 bits) in all but
 * stuffed bytes.  max_rounds: 0 .. YV4_JPEG_MAX_ROUNDS (0: only single-chunk segments are ever accepted).
 *
 * yv4_jpeg_segment.bit_off / pred stay zero: entry points live in yv4_jpeg_entry. */
#define YV4_JPEG_MIN_CHUNK_BYTES 4
#define YV4_JPEG_MAX_CHUNK_BYTES (1 << 20)
#define YV4_JPEG_MAX_ROUNDS 4096
#define YV4_JPEG_WG_CHUNKS 64          /* chunks per workgroup */

typedef struct yv4_jpeg_chunk {
  int32_t image;
  int32_t seg;             /* its segment, counted within the batch's segment table */
  int32_t index, count;    /* its place among the segment's chunks, and their number */
} yv4_jpeg_chunk;

typedef struct yv4_jpeg_entry {   /* written by the decode: what one chunk was decoded from and what it left */
  uint64_t entry;          /* the state (above) its last pass started from */
  uint64_t exit[2];        /* the state at the first symbol behind the chunk, or all ones after an error; round r
                              writes exit[r & 1], and exit[max_rounds & 1] is the final one */
  int32_t nblk;            /* blocks completed in the chunk */
  int32_t first_block;     /* ordinal, within the segment, of the block the entry lies in; -1: the chunk is not proven */
  uint16_t dc[3];          /* per component, the sum of the DC differences decoded in the chunk, modulo 2^16 */
  uint16_t tail;           /* 1: fewer than 8 real bits are left behind the exit */
  int16_t pred[3];         /* the DC predictors at the entry */
  int16_t reserved;
} yv4_jpeg_entry;

/* Host only, no HIP call: the chunk table of N placed images (scans / segs as yv4_jpeg_scan_prepare made and the caller
 * placed them).  chunks: every chunk of the batch, images, segments and chunks in order; seg_first (nseg + 1 entries):
 * each segment's first chunk, then the chunk count; wgs: runs of up to YV4_JPEG_WG_CHUNKS consecutive chunks of one
 * image (first_seg holds the run's first CHUNK, counted within the batch).  *nchunk / *nwg are the counts; with chunks
 * NULL only they are made, else YV4_E_CAPACITY if they exceed chunk_capacity / wg_capacity.  YV4_E_INVALID for a
 * chunk_bytes out of range, a segment with end < begin or more than 2^31 - 1 chunks. */
int yv4_jpeg_chunks_build(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, int N, int64_t nseg,
                          int32_t chunk_bytes, yv4_jpeg_chunk* chunks, int64_t chunk_capacity, int32_t* seg_first,
                          yv4_jpeg_wg* wgs, int64_t wg_capacity, int64_t* nchunk, int64_t* nwg);

/* Host only: the whole method on the CPU over the same tables with the same core, then the one lane per segment decode
 * of every undecided image (its coefficient range zero-filled again first).  All pointers are HOST memory.  Validates
 * like yv4_jpeg_entropy_decode_device_sync.  entries (nchunk): the records as the chunk decode left them; undecided
 * (N int32): nonzero where the image took the second decode; status (N int32): the final YV4_JPEG_ERR_* code of each
 * image, equal to yv4_jpeg_entropy_decode_segments'; *rounds (may be NULL): the last round in which any chunk was
 * decoded again. */
int yv4_jpeg_entropy_decode_sync(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_chunk* chunks,
                                 const int32_t* seg_first, const yv4_jpeg_wg* wgs, int N, int64_t nseg, int64_t nchunk,
                                 int64_t nwg, const uint8_t* bytes, int64_t bytes_len, const yv4_jpeg_huff* huff,
                                 int64_t nhuff, int32_t chunk_bytes, int32_t max_rounds, yv4_jpeg_entry* entries,
                                 int16_t* coef, int64_t coef_elems, int32_t* status, int32_t* undecided, int32_t* rounds);

/* The chunk decode of N images on `stream`: 1 + max_rounds sync launches (one wave per yv4_jpeg_wg run, the image's
 * tables in LDS), one launch for the sums and checks (one workgroup per segment), one for the storing decode.  No lane
 * waits on another workgroup; a round is a launch.  The HOST tables are validated before any launch (YV4_E_INVALID);
 * the *_dev copies (8-byte aligned; seg_first_dev 4-byte) are trusted.  entries_dev: nchunk records of DEVICE scratch.
 * The call zero-fills the batch's coefficient range, status and undecided (N int32 each, DEVICE).  Afterwards
 * undecided[n] != 0 names the images to decode again with yv4_jpeg_entropy_decode_device; status stays zero.  No read
 * leaves a segment's bytes and no store an image's coefficient range, whatever the bytes hold. */
int yv4_jpeg_entropy_decode_device_sync(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                        const yv4_jpeg_chunk* chunks, const int32_t* seg_first, const yv4_jpeg_wg* wgs,
                                        const yv4_jpeg_scan* scans_dev, const yv4_jpeg_segment* segs_dev,
                                        const yv4_jpeg_chunk* chunks_dev, const int32_t* seg_first_dev,
                                        const yv4_jpeg_wg* wgs_dev, int N, int64_t nseg, int64_t nchunk, int64_t nwg,
                                        const uint8_t* bytes, int64_t bytes_len, const yv4_jpeg_huff* huff, int64_t nhuff,
                                        int32_t chunk_bytes, int32_t max_rounds, yv4_jpeg_entry* entries_dev,
                                        int16_t* coef, int64_t coef_elems, int32_t* status, int32_t* undecided,
                                        void* stream);

/* ---- baseline JPEG encoding (csrc/jpeg_enc_core.h, csrc/jpeg_enc_host.cpp, csrc/jpeg_enc.hip; additive within ABI 8) --
 * libjpeg's default encoder, restated: jccolor.c's 16-bit fixed-point YCbCr, jcsample.c's h2v1 / h2v2 box filters,
 * jccoefct.c's edge rules (replicated last column and row, dummy blocks that repeat the previous block's quantised DC),
 * jfdctint.c's islow forward DCT, jcdctmgr.c's rounding division by 8 q, jpeg_set_quality(force_baseline)'s scaling of
 * the Annex K tables, the four Annex K Huffman tables, one interleaved scan without restart markers.  It is integer
 * arithmetic from the first pixel to the last stuffed byte, so the file equals what libjpeg-turbo writes (through
 * Pillow, turbojpeg or cv2.imwrite) for the same pixels, quality and sampling, byte for byte; tests/_jpeg_enc_ref.py is
 * the definition.  A batch of images of mixed sizes, samplings and qualities goes through in one call per stage.
 *
 * Two seams.  Pixels -> quantised coefficients (yv4_jpeg_encode_coefficients): int16 in the DECODER's coefficient layout
 * (natural order, one plane per component over the MCU-padded grid, component 0 first), dummy blocks filled, so that
 * yv4_jpeg_entropy_decode of libjpeg's file is the expected buffer element for element.  Coefficients -> the stuffed
 * scan bytes and their count (yv4_jpeg_encode_scan).  The host writes SOI .. SOS in front (yv4_jpeg_encode_header) and
 * FF D9 behind.  yv4_jpeg_encode_host is both stages on the CPU, compiled from the core the kernels run.
 *
 * yv4_jpeg_enc_image, one per image.  The caller fills width, height (1 .. 65535), channels (3: interleaved pixels,
 * B G R or R G B; 1: a gray plane, one component taken as is), hs x vs (the luma sampling: 1x1, 2x1 or 2x2 for three
 * channels -- 4:4:4, 4:2:2, 4:2:0 -- and 1x1 for one) and quality (1 .. 100); yv4_jpeg_encode_layout fills the rest
 * and places the batch densely.  The caller may then move an image's regions (src_off / src_pitch, coef_off, work_off,
 * out_off / out_cap); every entry point validates the table against the buffers' sizes before it runs anything.
 *   src_off, src_pitch      byte offset of the first pixel in the pixel buffer, and the row pitch (>= channels * width)
 *   coef_off                first coefficient in the coefficient buffer (int16 elements, % 64 == 0)
 *   work_off                byte offset of the image's work region (% 8 == 0): bit counts, running sums, the packed
 *                           stream before stuffing
 *   out_off, out_cap        where the scan bytes go and the room there.  The room is a derived bound, never read back
 *                           from the device: a block codes to at most YV4_JPEG_ENC_BLOCK_BITS bits -- a DC code of up to 11
 *                           bits (the chrominance table's category 11) with 11 value bits, 63 AC codes of up to 16 bits
 *                           with 10 value bits each -- and stuffing at most doubles the bytes:
 *                           out_cap >= 2 * ceil(nblocks * YV4_JPEG_ENC_BLOCK_BITS / 8)
 *   wg_base, swg_base       workgroups of the images before this one in the block grid (YV4_JPEG_ENC_WG_BLOCKS blocks
 *                           each) and in the stuffing grid (as many 32-bit words of the bound each): dense
 *                           (a call takes fewer than 2^24 workgroups a grid: YV4_E_INVALID past that)
 *   nblocks .. quant        blocks of the image; MCU grid; blocks per component on the MCU-padded grid and on the real
 *                           grid (ceil(ceil(width * h_c / hs) / 8), rows likewise); the luminance and chrominance
 *                           quantisation tables in natural order */
#define YV4_JPEG_ENC_WG_BLOCKS 256     /* blocks one workgroup of the bit-offset scan covers */
#define YV4_JPEG_ENC_BLOCK_BITS 1660   /* (11 + 11) + 63 * (16 + 10) */
#define YV4_JPEG_ENC_HEADER_MAX 640    /* room yv4_jpeg_encode_header asks for (it writes 623 bytes for three components) */

typedef struct yv4_jpeg_enc_image {
  int64_t src_off, coef_off, work_off, out_off, out_cap;
  int64_t wg_base, swg_base;
  int64_t nblocks;
  int32_t src_pitch, width, height, channels, ncomp, hs, vs, quality;
  int32_t mcus_x, mcus_y;
  int32_t blocks_w[3], blocks_h[3], real_w[3], real_h[3];
  uint16_t quant[2][64];
} yv4_jpeg_enc_image;

/* Host only, no HIP call: checks what the caller filled in (YV4_E_INVALID naming the image: an empty image, a side
 * above 65535, a quality outside 1 .. 100, another sampling), fills the rest and places the batch: pixels at pitch
 * channels * width and work / output regions at 256-byte aligned offsets, coefficients back to back.  totals[0 .. 5]:
 * pixel bytes, coefficient elements, workspace bytes, output bytes, block workgroups, stuffing workgroups. */
int yv4_jpeg_encode_layout(yv4_jpeg_enc_image* table, int N, int64_t* totals);

/* Host only: the check every entry point below makes before it runs anything -- each entry is what its size, sampling
 * and quality give, the workgroup bases are dense, and every region lies inside its buffer (pitch >= the row, out_cap >=
 * the bound).  YV4_OK or YV4_E_INVALID. */
int yv4_jpeg_encode_validate(const yv4_jpeg_enc_image* table, int N, int64_t pixel_bytes, int64_t coef_elems,
                             int64_t work_bytes, int64_t out_bytes);

/* Host only: SOI, APP0 (JFIF 1.01, density 1:1), one DQT per table, SOF0, the DHT segments (DC0, AC0, DC1, AC1; a gray
 * image DC0 and AC0) and SOS of one image, as libjpeg writes them -> out (capacity >= YV4_JPEG_ENC_HEADER_MAX, else
 * YV4_E_CAPACITY), *length bytes.  The file is this, the scan bytes, FF D9. */
int yv4_jpeg_encode_header(const yv4_jpeg_enc_image* im, uint8_t* out, int64_t capacity, int64_t* length);

/* Host only, all pointers HOST memory: the method on the CPU over the same table and the same work regions.  stage 1:
 * pixels -> coef; stage 2: coef -> out and sizes (N int64: the scan bytes of each image); stage 3: both.  Buffers a stage
 * does not use may be NULL.  rgb != 0: the pixels are R, G, B.  coef 2-byte, work 8-byte aligned. */
int yv4_jpeg_encode_host(const yv4_jpeg_enc_image* table, int N, int stage, const uint8_t* pixels, int64_t pixel_bytes,
                         int rgb, int16_t* coef, int64_t coef_elems, uint8_t* work, int64_t work_bytes, uint8_t* out,
                         int64_t out_bytes, int64_t* sizes);

/* Stage 1 on `stream`, one launch: one lane per 8x8 block.  table: HOST, validated here; table_dev: the same N entries in
 * DEVICE memory (8-byte aligned), trusted.  pixels and coef are DEVICE memory, coef 16-byte aligned.  Elements of coef
 * outside the images' regions are not touched. */
int yv4_jpeg_encode_coefficients(const yv4_jpeg_enc_image* table, const yv4_jpeg_enc_image* table_dev, int N,
                                 const uint8_t* pixels, int64_t pixel_bytes, int rgb, int16_t* coef, int64_t coef_elems,
                                 void* stream);

/* Stage 2 on `stream`, seven launches: bits per block; their running sum across workgroups; the zero-fill of the words
 * the stream will touch; the pack (atomic OR); 0xFF bytes per word; their running sum; the stuffed write.  No workgroup
 * waits on another inside a launch and no result depends on arrival order.  coef, work (8-byte aligned), out and sizes
 * (N int64, 8-byte aligned) are DEVICE memory; bytes outside the images' regions are not touched. */
int yv4_jpeg_encode_scan(const yv4_jpeg_enc_image* table, const yv4_jpeg_enc_image* table_dev, int N, const int16_t* coef,
                         int64_t coef_elems, uint8_t* work, int64_t work_bytes, uint8_t* out, int64_t out_bytes,
                         int64_t* sizes, void* stream);

/* ---- drawing detections (csrc/draw.hip; additive within ABI 8) -------------------------------------------------------
 * Boxes and their labels onto interleaved 8-bit images in place: one launch per batch, one lane per pixel.  The rule is
 * the package's own (tests/_draw_ref.py restates it; the reference's matplotlib rendering is not reproduced).  A pixel
 * takes the LAST box of its image, in input order, whose label or frame covers it, the label over the frame; boxes whose
 * score is not above score_thr are skipped.  Corners are truncated to int32.  The frame is `thickness` pixels inward
 * from the rectangle [x1, x2] x [y1, y2], clipped to the image, in bbox_color.  The label's top-left is at (x1, y1): the
 * class name, '|' and the score as d.dd with floor(score * 100 + 0.5) in float32, in a 5x7 glyph table scaled by
 * max(1, font_size / 7), one scaled pixel of padding at the left and top and of spacing behind each glyph, nine scaled
 * rows high; glyph pixels take text_color, the rest of the label the pixel's own value / 5.
 *
 * yv4_draw_image: pix_off / pitch / width / height place the image in the pixel buffer; box_base / nbox name its rows of
 * dets ((nbox_total, 5) float32: x1, y1, x2, y2, score) and labels (int32); wg_base: workgroups (256 pixels each) of the
 * images before it, filled by yv4_draw_layout.  names: (num_classes + 1) rows of YV4_DRAW_NAME_BYTES bytes, a row's
 * first byte its length and the characters (0x20 .. 0x7E) behind it; the last row is the name of a label outside
 * 0 .. num_classes - 1.  Colours are B, G, R in 0 .. 255 (the channel order of the pixels is the caller's business). */
#define YV4_DRAW_NAME_BYTES 32

typedef struct yv4_draw_image {
  int64_t pix_off, box_base, wg_base;
  int32_t pitch, width, height, nbox;
} yv4_draw_image;

typedef struct yv4_draw_style {
  int32_t bbox_color[3], text_color[3];
  int32_t thickness, font_size, num_classes;
  float score_thr;
} yv4_draw_style;

/* Host only: fills wg_base of every entry; *workgroups: their total. */
int yv4_draw_layout(yv4_draw_image* table, int N, int64_t* workgroups);

/* One launch on `stream`.  table: HOST, validated against pixel_bytes and nbox_total before the launch (YV4_E_INVALID);
 * table_dev, pixels, dets, labels and names are DEVICE memory.  Bytes that are no pixel of a frame or label keep their
 * value. */
int yv4_draw_boxes(const yv4_draw_image* table, const yv4_draw_image* table_dev, int N, uint8_t* pixels, int64_t pixel_bytes,
                   const float* dets, const int32_t* labels, int64_t nbox_total, const uint8_t* names,
                   const yv4_draw_style* style, void* stream);

/* The same per-pixel function on the CPU, all pointers HOST memory. */
int yv4_draw_boxes_host(const yv4_draw_image* table, int N, uint8_t* pixels, int64_t pixel_bytes, const float* dets,
                        const int32_t* labels, int64_t nbox_total, const uint8_t* names, const yv4_draw_style* style);

/* The same two calls with `flags` (yv4_draw_boxes / yv4_draw_boxes_host are these with flags 0).  YV4_DRAW_NO_SCORE:
 * boxes without a score, as ground truth is drawn -- the rows of dets are still five floats wide and the fifth is not
 * read, the label is the class name alone, and no box is skipped by score_thr.  Any other bit: YV4_E_INVALID. */
#define YV4_DRAW_NO_SCORE 1
int yv4_draw_boxes_ex(const yv4_draw_image* table, const yv4_draw_image* table_dev, int N, uint8_t* pixels,
                      int64_t pixel_bytes, const float* dets, const int32_t* labels, int64_t nbox_total,
                      const uint8_t* names, const yv4_draw_style* style, int flags, void* stream);
int yv4_draw_boxes_host_ex(const yv4_draw_image* table, int N, uint8_t* pixels, int64_t pixel_bytes, const float* dets,
                           const int32_t* labels, int64_t nbox_total, const uint8_t* names, const yv4_draw_style* style,
                           int flags);

#ifdef __cplusplus
}
#endif
#endif /* YV4_H_ */
