#!/usr/bin/env python
"""Headline benchmark: images/sec of the YOLOv4-L 608x608 fp32 inference hot path
(NCHW->NHWC, 115 fused MFMA convs, SPP, PAN resamples, decode+threshold, per-image NMS,
detections copied to pinned host memory) on N MI355X GPUs, one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Images are independent (per-image NMS, eval-mode BN), so ranks shard the batch with no
data-path collective: weak scaling, value = all ranks' images / max-over-ranks time.
Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, ms_per_step (the
wall time of one timed step) and the configuration.  A plain run does only that: set up, warm
up, time --steps steps, write the last timed step's detections if --dump-outputs DIR is given
(DIR/dets.npy, labels.npy, count.npy) and print the line.  With --full the line also holds
  roofline     fp32 MFMA: algorithmic conv FLOPs / HIP-event time of the conv launches
               measured inside the timed region, against the 157.3 TFLOP/s fp32 matrix peak
  output_check images 0-1 of the timed step against a batch-2 plan, bit for bit
  cpu_baseline the CPU oracle (plain torch CPU restatement of the reference) timed on this
               box's host cores on a bounded sample (rank 0, N=1 only), and
               output_check_oracle: image 0's pred maps against that oracle
  train_step   the bf16 batch-64/GPU training step (BASELINE.json configs[2]) measured by
               tools/train_bench.py in a child process per rank, data-parallel over RCCL when N > 1
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters
PEAK_H16_MFMA_TFLOPS = 2500.0   # dense bf16/fp16 MFMA peak, same guide (not the 2:1-sparsity figure)
PEAK_HBM_GBPS = 8000.0          # HBM3E, same guide

MODELS = {
    'yolov4l': dict(scale='v4l5p', neck_in=[256, 512, 512], neck_out=[256, 512, 1024], csp_rep=2),
    'yolov4s': dict(scale='v4s5p', neck_in=[128, 256, 256], neck_out=[128, 256, 512], csp_rep=1),
    # configs/yolov5/yolov5l_coco_mosaic.py: _base_ yolov4l + backbone v5l5p (out 2,3,4) + YOLOV5Neck
    # configs/yolo/yolov3_d53_mstrain-608_273e_coco.py (the only path with a published upstream fps)
    'yolov3': dict(scale='darknet53', v3=True),
    'yolov5l': dict(scale='v5l5p', neck='YOLOV5Neck', neck_in=[256, 512, 1024], neck_out=[256, 512, 1024], csp_rep=2,
                    out_indices=[2, 3, 4]),
}


def model_cfg(name):
    m = MODELS[name]
    if m.get('v3'):
        return dict(
            type='YOLOV3', backbone=dict(type='Darknet', depth=53, out_indices=(3, 4, 5)),
            neck=dict(type='YOLOV3Neck', num_scales=3, in_channels=[1024, 512, 256], out_channels=[512, 256, 128]),
            bbox_head=dict(type='YOLOV3Head', num_classes=80, in_channels=[512, 256, 128], out_channels=[1024, 512, 256],
                           loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
                           loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
                           loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
                           loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum')),
            train_cfg=dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0)),
            test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, conf_thr=0.005,
                          nms=dict(type='nms', iou_threshold=0.45), max_per_img=100))
    return dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=m['scale'], out_indices=m.get('out_indices', [3, 4, 5])),
        neck=dict(type=m.get('neck', 'YOLOV4Neck'), in_channels=m['neck_in'], out_channels=m['neck_out'],
                  csp_repetition=m['csp_rep']),
        bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=m['neck_out']),
        train_cfg=dict(),
        test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65),
                      max_per_img=300))


def synthetic_images(batch, size, seed, device):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (batch, 3, size, size), generator=g, dtype=torch.uint8)
    return ((img.float() - 114.0) / 255.0).to(device)     # img_norm_cfg of configs/yolov4/*


def synthetic_gts(batch, size, seed, device):
    """SURVEY 8d ground truth of the training configurations: per image Poisson(12) boxes (>= 1), centre
    U[0, size), w and h log-uniform in [8, 400], clipped to the image; labels U{0..79}."""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    lo, hi = torch.log(torch.tensor(8.0)), torch.log(torch.tensor(400.0))
    for _ in range(batch):
        n = max(1, int(torch.poisson(torch.tensor(12.0), generator=g)))
        c = torch.rand(n, 2, generator=g) * size
        wh = torch.exp(torch.rand(n, 2, generator=g) * (hi - lo) + lo)
        b = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, size)
        boxes.append(b.to(device))
        labels.append(torch.randint(0, 80, (n,), generator=g).to(device))
    return boxes, labels


def init_head(det, plan, img, target_per_img, logit_std=2.0):
    """Random head whose logits have std ~2 around a common bias, the bias bisected so that
    about `target_per_img` (box, class) scores pass score_thr -- the realistic post-process
    regime (an untrained head passes ~everything)."""
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd.plan import pack_conv_weight
    head_ops = [o for o in plan.ops if o.kind == 'conv' and o.name.startswith('pred_conv')]
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for conv, op in zip(det.bbox_head.convs_pred, head_ops):
            # features are Mish outputs of unit-variance pre-activations: E[x^2] ~ 0.45
            std = logit_std / (0.45 * conv.in_channels) ** 0.5
            conv.weight.copy_(torch.empty(conv.weight.shape).normal_(0, std, generator=g).to(conv.weight.device))
            op.info['launch']['w'].copy_(pack_conv_weight(conv.weight)[0])
    lo, hi = -16.0, 0.0
    count = 0.0
    for _ in range(16):
        b = 0.5 * (lo + hi)
        with torch.no_grad():
            for conv, op in zip(det.bbox_head.convs_pred, head_ops):
                bias = conv.bias.view(3, 85)
                bias.zero_()
                bias[:, 4:] = b
                op.info['launch']['t1'].copy_(conv.bias)
        plan.run(img)
        torch.cuda.synchronize()
        count = float(plan.post['counts'].float().mean())
        if count > target_per_img:
            hi = b
        else:
            lo = b
    return count


def tile_of_kernel(name):
    """Tile class (the names of ``_lib.TILE_NAMES`` / ``HTILE_NAMES`` + the fused / persistent kernels) of a kernel name as
    rocprofv3 prints it; None for kernels that are not convolutions."""
    import re
    m = re.search(r'conv_mfma_f32_dma_kernel<(\d+), (\d+)', name)
    if m:
        return f'dma{m.group(1)}x{m.group(2)}'
    m = re.search(r'conv_mfma_f32_kernel<(\d+), (\d+)', name)
    if m:
        return f'{m.group(1)}x{m.group(2)}'
    m = re.search(r'conv_mfma_h16_kernel<(?:true|false), (\d+), (\d+)', name)
    if m:
        return f'h16_{m.group(1)}x{m.group(2)}'
    for pat, tile in (('conv1x1_ws_f32_kernel', 'ws_1x1'), ('conv3x3_wide_f32_kernel', 'w3x3'), ('conv_wide_f32_kernel', 'wide'), ('conv1x1_ws_kernel', 'h16_ws_1x1'), ('conv3x3_small_kernel', 'h16_s3x3'),
                      ('stem_down', 'stem_down'), ('conv_stem3x3_kernel', 'stem3x3'), ('conv3x3_pp_h16_kernel', 'h16_pp3x3'),
                      ('conv3x3_wide_h16_kernel', 'h16_w3x3'), ('conv_wide_h16_kernel', 'h16_wide')):
        if re.search(pat, name):
            return tile
    return None


def pmc_traffic(tile_name, run_key, alg_bytes_per_launch, launches_per_step):
    """HBM bytes per launch of the dominant conv tile class from the committed rocprofv3 --pmc summary of THIS command
    (counters cannot be read from inside the bench): the newest ``profiles/rNN_pmc_per_kernel*.json`` that holds a run
    named ``run_key``.  The summary carries the ``roofline.tiles`` block of the bench line printed under the profiler; it
    is REFUSED (traffic null, the reason in ``traffic_source``) unless that block's launch set equals this run's: same
    launches per step of the tile class and the same algorithmic bytes per launch within 2 % -- a summary of another
    kernel selection or another layer set says nothing about this run."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_per_kernel*.json')), reverse=True)
    for f in files:
        try:
            d = json.load(open(f))
        except Exception:
            continue
        run = d.get(run_key)
        if not isinstance(run, dict) or '_run' not in run:
            continue
        rel = os.path.relpath(f, ROOT) + ':' + run_key
        t = run['_run'].get('tiles', {}).get(tile_name)
        if t is None:
            return None, f'refused: {rel} was taken when no launch used tile {tile_name}'
        if t['launches_per_step'] != launches_per_step or \
                abs(t['algorithmic_bytes_per_launch'] - alg_bytes_per_launch) > 0.02 * alg_bytes_per_launch:
            return None, (f"refused: {rel} profiled {t['launches_per_step']} launches/step of {tile_name} at "
                          f"{t['algorithmic_bytes_per_launch']} algorithmic B/launch, this run has {launches_per_step} at "
                          f'{round(alg_bytes_per_launch)}')
        tot, n = 0.0, 0
        for k, e in run.items():
            if k != '_run' and tile_of_kernel(k) == tile_name and 'hbm_bytes_per_launch' in e:
                tot += e['hbm_bytes_per_launch'] * e['launches_sampled']
                n += e['launches_sampled']
        if n == 0:
            return None, f'refused: {rel} holds no counters for tile {tile_name}'
        return round(tot / n), rel
    return None, None


def host_cpu_budget():
    """CPUs this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(det, size, budget_s=25.0):
    """The CPU oracle (oracle/: the reference's graph in torch CPU ops + C NMS) on this box.
    Test infrastructure used as a yardstick only; never on the product path."""
    from oracle import yolov4_oracle as O
    sd = {k: v.detach().cpu().clone() for k, v in det.state_dict().items()}
    if det_scale(det) == 'darknet53':
        return cpu_baseline_v3(det, sd, size, budget_s)
    stages, reps = O.ARCH[det_scale(det)]
    img = synthetic_images(1, size, 99, 'cpu')
    sf = [[1.0, 1.0, 1.0, 1.0]]
    threads = host_cpu_budget()
    torch.set_num_threads(threads)
    n, t_total = 0, 0.0
    with torch.no_grad():
        t0 = time.perf_counter()
        O.simple_test(img, sd, stages, reps, [3, 4, 5], sf, 80)      # warm-up (oneDNN primitive cache)
        warm = time.perf_counter() - t0
        while t_total + warm < budget_s and n < 64:
            t0 = time.perf_counter()
            O.simple_test(img, sd, stages, reps, [3, 4, 5], sf, 80)
            t_total += time.perf_counter() - t0
            n += 1
        if n == 0:      # a single forward already exceeds the budget: report the warm-up run
            n, t_total = 1, warm
    return dict(value=round(n / t_total, 4), unit='images/sec', cores=threads, kind='port',
                sample=f'{n} single-image {size}x{size} forward+decode+NMS runs of the CPU oracle '
                       f'({t_total:.1f} s, {threads} torch threads = cgroup CPU quota), same weights as the GPU run')


def cpu_baseline_v3(det, sd, size, budget_s):
    from oracle import yolov3_oracle as V3
    img = synthetic_images(1, size, 99, 'cpu')
    threads = host_cpu_budget()
    torch.set_num_threads(threads)
    cfg = det.bbox_head.test_cfg

    def run():
        with torch.no_grad():
            feats = V3.darknet(img, sd, det.backbone.layers, det.backbone.out_indices)
            preds = V3.yolov3_head(V3.yolov3_neck(feats, sd), sd)
            return V3.get_bboxes_v3(preds, [[1.0, 1.0, 1.0, 1.0]], 80, nms_pre=cfg['nms_pre'], score_thr=cfg['score_thr'],
                                    conf_thr=cfg['conf_thr'], iou_threshold=cfg['nms']['iou_threshold'],
                                    max_per_img=cfg['max_per_img'])
    run()
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < budget_s and n < 64:
        run()
        n += 1
    el = time.perf_counter() - t0
    return dict(value=round(n / el, 4), unit='images/sec', cores=threads, kind='port',
                sample=f'{n} single-image {size}x{size} forward+decode+NMS runs of the CPU oracle (YOLOv3) '
                       f'({el:.1f} s, {threads} torch threads = cgroup CPU quota), same weights as the GPU run')


# image 0's pred maps of the timed step vs the CPU oracle, |diff| / (1 + |ref|): fp32 is anchored on the float64 oracle
# (oracle_check; the 'f32' entry below is no longer a bound, only the 16-bit ones are); 16-bit operands: one rounding per fused
# layer through ~110 layers (measured mean 5e-3 fp16 / 4e-2 bf16) -- bounds that a skipped MFMA, a missing
# slice or a stale buffer exceed by orders of magnitude
ORACLE_BOUNDS = {'f32': (5e-5, 2e-3), 'f16': (3e-2, 1.0), 'bf16': (2e-1, 4.0)}


def oracle_check(det, img0, pred0, dets0, dtype):
    """The checker leg of the bench: the oracle (test infrastructure) evaluates image 0 of the timed batch on the CPU in
    fp32; the timed plan's pred maps must agree within ORACLE_BOUNDS[dtype] and, in fp32, the detection count with the
    oracle's own post-processing (+-2: near-ties at the max_per_img cut)."""
    from oracle import yolov4_oracle as O
    sd = {k: v.detach().cpu().clone() for k, v in det.state_dict().items()}
    stages, reps = O.ARCH[det_scale(det)]
    outs = list(det.backbone.out_indices) if hasattr(det.backbone, 'out_indices') else [3, 4, 5]
    neck = 'v5' if type(det.neck).__name__ == 'YOLOV5Neck' else 'v4'
    with torch.no_grad():
        ref, _ = O.forward_pred_maps(img0, sd, stages, reps, outs, neck=neck)
    mean_b, max_b = ORACLE_BOUNDS[dtype]
    worst_mean = worst_max = 0.0
    if dtype == 'f32':
        # fp32: anchored on the oracle evaluated in FLOAT64, as tests/test_gpu_fullsize.py does -- 115 layers deep two
        # correct fp32 evaluations differ by the amplified rounding of their summation orders, so the statement is "the
        # HIP maps are as close to the truth as the fp32 CPU oracle (the reference's own arithmetic) is": per level
        # mean <= 1.5 x and max <= 2.5 x the fp32 oracle's own distance from float64 (a loose constant would have to
        # be re-fitted whenever a kernel's summation order changes: round 4's 7.7e-4 -> 1.04e-3 against "2e-3")
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        with torch.no_grad():
            ref64, _ = O.forward_pred_maps(img0.double(), sd64, stages, reps, outs, neck=neck)
        parts = []
        ok = True
        for lvl, (got, r, t) in enumerate(zip(pred0, ref, ref64)):
            r, t = r[0], t[0]
            if tuple(got.shape) != tuple(r.shape):
                return False, f'pred map shape {tuple(got.shape)} != oracle {tuple(r.shape)}'
            e_gpu = (got.double() - t).abs() / (1 + t.abs())
            e_cpu = (r.double() - t).abs() / (1 + t.abs())
            if not bool(torch.isfinite(e_gpu).all()):
                return False, 'non-finite pred map'
            gm, gx, cm, cx = float(e_gpu.mean()), float(e_gpu.max()), float(e_cpu.mean()), float(e_cpu.max())
            ok = ok and gm <= 1.5 * cm + 1e-6 and gx <= 2.5 * cx + 1e-5
            parts.append(f'L{lvl} {gm:.1e}/{gx:.1e} vs {cm:.1e}/{cx:.1e}')
            e = (got - r).abs() / (1 + r.abs())
            worst_mean, worst_max = max(worst_mean, float(e.mean())), max(worst_max, float(e.max()))
        msg = ('image 0 pred maps of the timed step vs the CPU oracle in float64, mean/max of |d| / (1 + |logit|) per level, '
               'HIP vs fp32 CPU oracle: ' + ', '.join(parts) + ' (bound: mean <= 1.5 x, max <= 2.5 x the fp32 oracle\'s own); '
               f'HIP vs fp32 oracle directly: mean {worst_mean:.2e} / max {worst_max:.2e}')
    else:
        for got, r in zip(pred0, ref):
            r = r[0]
            if tuple(got.shape) != tuple(r.shape):
                return False, f'pred map shape {tuple(got.shape)} != oracle {tuple(r.shape)}'
            e = (got - r).abs() / (1 + r.abs())
            if not bool(torch.isfinite(e).all()):
                return False, 'non-finite pred map'
            worst_mean, worst_max = max(worst_mean, float(e.mean())), max(worst_max, float(e.max()))
        msg = (f'image 0 pred maps of the timed step vs the CPU oracle: mean {worst_mean:.2e} / max {worst_max:.2e} of 1 + |logit| '
               f'(bounds {mean_b:g} / {max_b:g})')
        ok = worst_mean <= mean_b and worst_max <= max_b
    if dtype == 'f32' and ok:
        res = O.get_bboxes(ref, [[1.0, 1.0, 1.0, 1.0]], 80, rescale=True)[0]
        k = int(res[0].shape[0])
        msg += f'; detections {dets0[0]} vs oracle {k}'
        ok = abs(k - dets0[0]) <= 2
    return ok, msg


def pin_check_plan(plan, small):
    import mmdet_yolov4_amd as pkg
    """fp32 only: the wide-tile kernels (16x16x4 MFMAs) group the K sum differently from the 32x32x2 tiles a batch-2 plan
    would pick by itself, so a check plan is PINNED to the timed plan's tile ids layer by layer (yv4_conv_pick_tile
    reports the pinned form; every tile kernel is batch-invariant).  The 16-bit tiles are all bit-identical to each
    other (tests/test_gpu_h16.py::test_*_matches_generic_bitwise) and need no pinning.  Returns '' or a note when the
    two plans' launch lists do not line up.  Used by the output check below and by tests/test_gpu_fullsize.py."""
    import ctypes
    big_convs = [o for o in plan.ops if o.kind == 'conv' and 'desc' in o.info]
    small_convs = [o for o in small.ops if o.kind == 'conv' and 'desc' in o.info]
    if len(big_convs) != len(small_convs):
        return (f'; NOTE: the timed plan has {len(big_convs)} conv launches, the batch-2 plan {len(small_convs)}: '
                'tile ids NOT pinned layer by layer')
    pick = pkg._lib.lib().yv4_conv_pick_tile
    for ob, os_ in zip(big_convs, small_convs):
        db, ds = ob.info['desc'], os_.info['desc']
        if ob.info.get('fused') or ob.info.get('stem32') or os_.info.get('fused') or os_.info.get('stem32'):
            continue
        t = db.tile if db.tile else pick(ctypes.byref(db))
        ts = ds.tile if ds.tile else pick(ctypes.byref(ds))
        # either side on a wide-tile form (the timed plan's fill rule depends on M: a batch-2 layer can take a wide tile the
        # batch-N plan rejected, and the other way round): the check plan runs the TIMED plan's resolved tile id.  The
        # 32x32x2 tiles (ids 1-9) give the same bits as one another.
        if t != ts and (t >= 10 or ts >= 10):
            ds.tile = t
    return ''


def vs_published(args, value):
    """BASELINE.md holds published numbers only for upstream YOLOv3-DarkNet53 at batch 1 (fwd + post-processing,
    one V100, configs/yolo/README.md:22-24); every other configuration has none."""
    pub = {320: 63.9, 416: 61.2, 608: 48.1}
    if MODELS[args.model].get('v3') and args.batch == 1 and args.gpus == 1 and args.dtype == 'f32' and args.size in pub:
        return round(value / pub[args.size], 3)
    return None


def train_step_leg(args, rank, local_rank, world):
    """The train-step half of BASELINE.json's metric (configs[2]: bf16, batch 64/GPU, data-parallel with the RCCL
    all-reduce of ``dist.GradReducer`` when WORLD_SIZE > 1), measured by ``tools/train_bench.py`` in a CHILD process of
    every rank after this process has left its own process group: a fault or a stuck collective in the training path
    then costs the ``train_step`` object, not the inference line.  The children rendezvous on their own port."""
    import subprocess
    env = dict(os.environ)
    port = int(env.get('MASTER_PORT', '29500'))
    env['MASTER_PORT'] = str(port + 7 if port < 65000 else port - 7)
    env.setdefault('MASTER_ADDR', '127.0.0.1')
    env['RANK'], env['LOCAL_RANK'], env['WORLD_SIZE'] = str(rank), str(local_rank), str(world)
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'train_bench.py'),
           '--batch', str(args.train_batch), '--size', str(args.size), '--steps', str(args.steps),
           '--warmup', str(args.warmup), '--dtype', args.train_dtype, '--model', args.model]
    try:
        r = subprocess.run(cmd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=args.train_timeout, text=True)
    except subprocess.TimeoutExpired:
        return dict(error=f'train_bench.py still running after {args.train_timeout} s; killed')
    if rank != 0:
        return None
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    if r.returncode != 0 or not lines:
        return dict(error=f'train_bench.py exit {r.returncode}: ' + r.stderr.strip()[-400:])
    t = json.loads(lines[-1])
    t['unit'] = 'images/sec'
    t['steps'], t['warmup'] = args.steps, args.warmup
    t['config'] = dict(workload=f'{args.model} {args.size}x{args.size} {args.train_dtype} train step (forward, fused loss, '
                                f'backward, gradient all-reduce, SGD-Nesterov + EMA through the recipe hooks), batch '
                                f'{args.train_batch}/GPU (BASELINE.json configs[2])',
                       global_batch=args.train_batch * world,
                       parallelism=f'dp{world}: replicated weights, ' + str(t.get('grad_exchange'))
                       if world > 1 else 'one rank, no collective')
    return t


def det_scale(det):
    return det._bench_scale


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def launch_ranks(n, argv, script=None, python=None, timeout=None):
    """``python bench.py --gpus N`` without a launcher: start the N ranks as CHILD processes (one per GPU, RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their environment -- the contract of
    ``torch.distributed.run``, tools/dist_train.sh:8-10), relay rank 0's output (the one JSON line) and return the worst
    exit code.  The parent never initialises the GPU and never exec()s: it only waits.  A rank that dies takes the
    others with it after a grace period (they would otherwise sit in a collective until its timeout)."""
    import subprocess
    import threading
    script = script or os.path.abspath(__file__)
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: what RCCL needs on this driver
        env.setdefault('OMP_NUM_THREADS', str(max(1, host_cpu_budget() // n)))
        procs.append(subprocess.Popen([python or sys.executable, script] + list(argv), env=env, stdin=subprocess.DEVNULL,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=None, text=True))

    def relay():
        for line in procs[0].stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
    t = threading.Thread(target=relay, daemon=True)
    t.start()
    t0 = time.time()
    rcs = [None] * n
    killed = set()                                             # ranks the launcher itself took down
    seen_at = [None] * n                                       # the poll in which a rank's exit was first seen
    failed_at = None
    polls = 0
    while any(rc is None for rc in rcs):
        polls += 1
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
                if rcs[i] is not None:
                    seen_at[i] = polls
        bad = [rc for rc in rcs if rc not in (None, 0)]
        if bad and failed_at is None:
            failed_at = time.time()
        if (failed_at is not None and time.time() - failed_at > 30) or (timeout and time.time() - t0 > timeout):
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    p.kill()                                   # exactly the PIDs started here
                    rcs[i] = p.wait()
                    killed.add(i)
            break
        time.sleep(0.2)
    t.join(timeout=5)
    # the exit code of the run = the non-zero code of the rank that died FIRST by itself (the ranks that follow abort in
    # their collectives with whatever the backend exits with; a rank this launcher killed returns -9, which must not mask
    # the real failure); the larger code among ranks seen dead in the same poll; 124 (timeout's convention) when only
    # launcher kills happened
    own = sorted((seen_at[i], -abs(rc), rc) for i, rc in enumerate(rcs) if i not in killed and rc not in (None, 0))
    code = 0
    if own:
        rc0 = own[0][2]
        code = rc0 if 0 < rc0 < 256 else 128 + min(abs(rc0), 127)              # a signal: the shell's 128 + n
    elif killed:
        code = 124
    if code:
        print(f'bench.py launcher: rank exit codes {rcs} (killed by the launcher: {sorted(killed)})', file=sys.stderr)
    return code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32, help='images per GPU per step')
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--model', default='yolov4l', choices=sorted(MODELS))
    ap.add_argument('--candidates', type=float, default=2000.0, help='target NMS candidates per image')
    ap.add_argument('--full', action='store_true',
                    help='also measure and check what the headline figure does not need: per-conv HIP events in the timed '
                         'region (roofline), the batch-2 output check, the CPU baseline with the oracle check, the train step')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='write the detections of the last timed step to DIR/{dets,labels,count}.npy (float32; rows past '
                         'an image\'s count are 0 in dets and -1 in labels)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-output-check', action='store_true',
                    help='skip the batch-2 plan of the output check (profiling runs: every profiled conv launch is then a '
                         'launch of the timed configuration, so rocprofv3 averages are per-step averages)')
    ap.add_argument('--layers', default='', help='write a per-conv timing table (JSON) to this path (instruments the '
                                                 'conv launches as --full does)')
    ap.add_argument('--autotune', action='store_true',
                    help='re-decide the conv tile of every layer by timing the candidates on this box (default: the static '
                         'choice of pick_tile, which measures the same images/s; see DESIGN.md 2.3)')
    ap.add_argument('--no-autotune', action='store_true', help='accepted for old command lines: the default now')
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f16', 'bf16'],
                    help='operand type of the convs (f32 = the headline / parity configuration)')
    ap.add_argument('--no-train', action='store_true', help='skip the train-step leg (the "train_step" object)')
    ap.add_argument('--train-batch', type=int, default=64, help='images per GPU per training step (configs[2])')
    ap.add_argument('--train-dtype', default='bf16', choices=['f32', 'f16', 'bf16'])
    ap.add_argument('--train-timeout', type=float, default=420.0, help='seconds the train-step child may take')
    ap.add_argument('--graph', action='store_true',
                    help='replay the launch list as ONE hipGraph per step (the batch-1 protocol of '
                         'tools/analysis_tools/benchmark.py:83-109 is launch-bound otherwise); the per-conv HIP events of '
                         'the roofline block then come from extra eager steps after the timed region')
    ap.add_argument('--streams', type=int, default=1,
                    help='run the step as this many part-batch plans on as many HIP streams (default 1; 2: every conv launch has a '
                         'compute phase that leaves HBM idle and a memory phase that leaves the matrix pipe idle, and one '
                         'persistent workgroup per CU keeps all CUs in the same phase; two independent half-batch plans fill each '
                         'other\'s phases and kernel boundaries.  Measured (profiles/r06_two_stream_probe.txt, r06_ab_streams.txt): fp32 +0.9-2.2 %%, '
                         'configs[3] -1 to +8 %%, bf16 0, and the batch-16 launches fill the chip worse (dominant tile 0.79 -> 0.71 of its '
                         'roof) -- not the default')
    ap.add_argument('--event-every', type=int, default=10,
                    help='bracket the conv launches with HIP events in every n-th timed step.  The two event records around a '
                         'launch keep it from overlapping its neighbours: ~0.6 ms per instrumented step, i.e. with every 4th step '
                         'instrumented 0.5 %% of the fp32 rate, 3 %% of the bf16 rate and 1.5 %% of configs[3]\'s '
                         '(profiles/r06_ab_events.txt)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher (it never touches the GPU) and the N
        # ranks are its children -- what tools/dist_train.sh:8-10 does with torch.distributed.launch
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import dist as D
    rank, local_rank, world = D.env_world()
    if world != args.gpus:
        sys.exit(f'bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}; start it as `python bench.py --gpus N` '
                 '(self-launching) or under torch.distributed.run with --nproc-per-node N')
    dev = torch.device('cuda', local_rank)
    torch.cuda.set_device(dev)
    D.init(backend='nccl', device=dev)              # RCCL; a no-op for a single process

    from mmdet_yolov4_amd.calibrate import calibrate_bn
    pkg._lib.lib()                                  # fail loudly if the HIP extension is missing

    torch.manual_seed(0)                            # identical weights on every rank
    det = pkg.build_detector(model_cfg(args.model))
    det.init_weights()
    det._bench_scale = MODELS[args.model]['scale']
    det.eval().to(dev)
    img = synthetic_images(args.batch, args.size, 1000 + rank, dev)

    plan = det.compile(args.batch, args.size, args.size, device=dev, rescale=True)
    calibrate_bn(plan, img)
    ncand = init_head(det, plan, img, args.candidates)
    h16 = args.dtype != 'f32'
    if h16:
        # BN statistics and the head were fitted through the fp32 plan (they live in the modules);
        # rebuild the plan on 16-bit operands
        del plan
        det._engines.clear()
        torch.cuda.empty_cache()
        plan = det.compile(args.batch, args.size, args.size, device=dev, rescale=True,
                           dtype=torch.float16 if args.dtype == 'f16' else torch.bfloat16)
        plan.run(img)
        torch.cuda.synchronize()
        ncand = float(plan.post['counts'].float().mean())
    if args.autotune and not args.no_autotune:
        plan.autotune()

    # ---- the step as NS part-batch plans on NS streams (default 2; --streams 1: one plan on the current stream) ----------
    NS = args.streams if (args.streams > 1 and not args.graph and not args.autotune and args.batch % args.streams == 0
                          and args.batch // args.streams >= 2) else 1
    tdt = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    stream = torch.cuda.current_stream()
    ctypes_ = __import__('ctypes')
    if NS > 1:
        nb = args.batch // NS
        del plan
        torch.cuda.empty_cache()
        plans = []
        for _ in range(NS):
            det._engines.clear()                        # distinct plan instances (own buffers) for the same geometry
            plans.append(det.compile(nb, args.size, args.size, device=dev, rescale=True, dtype=tdt))
        streams_ = [stream] + [torch.cuda.Stream(device=dev) for _ in range(NS - 1)]
        plan = plans[0]                                 # (image 0 lives here: output check, oracle leg, tile ids)
    else:
        nb = args.batch
        plans, streams_ = [plan], [stream]
    sptrs = [ctypes_.c_void_p(s_.cuda_stream) for s_ in streams_]
    conv_ops = [o for pl in plans for o in pl.ops if o.kind == 'conv']
    post = plan.post
    host_dets = torch.empty((args.batch,) + tuple(post['dets'].shape[1:]), dtype=torch.float32, pin_memory=True)
    host_labels = torch.empty((args.batch,) + tuple(post['labels'].shape[1:]), dtype=torch.int32, pin_memory=True)
    host_count = torch.empty((args.batch,) + tuple(post['count'].shape[1:]), dtype=torch.int32, pin_memory=True)
    for i, pl in enumerate(plans):
        pl.inputs[0]['src'] = img[i * nb:(i + 1) * nb]
    if args.graph:
        plan.capture()                                  # static input buffer + one graph of the whole launch list
        plan.inputs[0]['src'].copy_(img)
        torch.cuda.synchronize()
    step_done = [torch.cuda.Event() for _ in range(NS)]

    def copy_out(i):
        pl, sl = plans[i], slice(i * nb, (i + 1) * nb)
        with torch.cuda.stream(streams_[i]):
            host_dets[sl].copy_(pl.post['dets'], non_blocking=True)
            host_labels[sl].copy_(pl.post['labels'], non_blocking=True)
            host_count[sl].copy_(pl.post['count'], non_blocking=True)
    # (The copies on a stream of their own, ordered behind the step's last kernel by an event and ahead of the next step's
    # post-processing by another, so that the next step's convs do not wait for three PCIe round trips: built and measured,
    # bf16 -5 to -8 %, configs[3] -3.6 / +0.4 %, fp32 -0.3 % -- the cross-stream event waits cost more than the copies.
    # profiles/r06_ab_copystream_dropped.txt)

    def step(events=None):
        if args.graph and events is None:
            plan.graph.replay()
            copy_out(0)
            return
        if events is not None:
            # instrumented step: one part at a time, so that every bracketed launch has the chip to itself.  Events come from a
            # pool created before the timed region: creating two per launch inside it made the instrumented 16-bit steps
            # host-bound, and the gap where the GPU caught up read as one slow kernel
            for i, pl in enumerate(plans):
                if NS > 1:
                    torch.cuda.synchronize()
                for op in pl.ops:
                    if op.kind == 'conv':
                        e0, e1 = ev_pool.pop() if ev_pool else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                        e0.record(streams_[i])
                        op.fn(sptrs[i])
                        e1.record(streams_[i])
                        events.append((op, e0, e1))
                    else:
                        op.fn(sptrs[i])
                copy_out(i)
            return
        if NS > 1:                                      # a step is one batch: every stream starts it behind the whole last step
            for i in range(NS):
                for j in range(NS):
                    if j != i:
                        streams_[i].wait_event(step_done[j])
            for ops in zip(*[pl.ops for pl in plans]):  # launch lists interleaved: both streams stay fed by one host thread
                for i, op in enumerate(ops):
                    op.fn(sptrs[i])
        else:
            for op in plan.ops:
                op.fn(sptrs[0])
        for i in range(NS):
            copy_out(i)
            if NS > 1:
                step_done[i].record(streams_[i])

    # per-conv HIP events (--full, --layers): with one stream, every n-th step INSIDE the timed region is instrumented; with
    # several streams (and under --graph) instrumented steps run after it -- a launch bracketed while the other stream's kernels
    # share the chip would time the mixture, not the kernel.  A plain run brackets nothing.
    instrument = args.full or bool(args.layers)
    events_inside = instrument and NS == 1 and not args.graph
    n_instr = (args.steps + max(args.event_every, 1) - 1) // max(args.event_every, 1) + 2
    ev_pool = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(n_instr * len(conv_ops) if instrument else 0)]
    for _ in range(args.warmup):
        step()
    # no garbage collection inside the timed region: an instrumented step allocates ~230 event objects, and a
    # generation-0 pass of the collector between a start event and its launch showed up as a 170 us "kernel" at the
    # same layer of every such step (profiles/r02_layers_bf16.json before this line)
    import gc
    gc.collect()
    gc.disable()
    D.barrier()
    events = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(events if (i % max(args.event_every, 1) == 0 and events_inside) else None)
    D.barrier()
    my_elapsed = time.perf_counter() - t0
    elapsed = D.max_over_ranks(my_elapsed, device=dev)
    # what every rank saw: its world size (the RCCL group's, not the launcher's word for it), device and own rate
    import torch.distributed as tdist
    mine = dict(rank=rank, world_size=tdist.get_world_size() if tdist.is_available() and tdist.is_initialized() else 1,
                backend=D.backend_name() if hasattr(D, 'backend_name') else None, device=str(dev),
                images_per_sec=round(args.batch * args.steps / my_elapsed, 2))
    if tdist.is_available() and tdist.is_initialized() and world > 1:
        per_rank = [None] * world
        tdist.all_gather_object(per_rank, mine)
    else:
        per_rank = [mine]
    gc.enable()
    torch.cuda.synchronize()
    assert int(host_count.min()) >= 0, 'an image took the split NMS path; lower --candidates'
    if args.dump_outputs:                               # the last timed step's detections, before any further step
        dump_outputs(args.dump_outputs, host_dets, host_labels, host_count, '' if world == 1 else f'_rank{rank}')
    if instrument and not events_inside:                # per-conv events: instrumented steps outside the timed region
        for _ in range(max(2, args.steps // max(args.event_every, 1))):
            step(events)
        torch.cuda.synchronize()

    # ---- roofline of the dominant kernel (the fused MFMA conv), from the timed region ------
    roofline = per_layer = None
    if instrument:
        roofline, per_layer = roofline_block(args, events, events_inside, conv_ops, h16, nb, NS, elapsed)
    if args.layers and rank == 0:
        rows = []
        for op, tsum, n, tile in per_layer.values():
            i = op.info
            rows.append(dict(name=op.name, Cin=i['Cin'], Cout=i['Cout'], k=i['k'], stride=i['stride'], H=i['H'],
                             W=i['W'], tile=tile, us=round(tsum / n * 1e6, 1),
                             tflops=round(op.flops / (tsum / n) / 1e12, 1), gflop=round(op.flops / 1e9, 2),
                             mbytes=round(op.bytes / 1e6, 2), residual=i['launch']['res'] is not None))
        with open(args.layers, 'w') as f:
            json.dump(rows, f, indent=1)

    # the timed batch's output is the real thing: image 0 (and 1) of the batch-N step must equal, bit for bit, what a
    # batch-2 plan computes for the same two images (per-image NMS, eval-mode BN, every conv tile walks K in the same
    # order -- the wide-tile 3x3 kernel's 16x16x32 MFMAs included: tests/test_gpu_h16.py::test_wide3x3_matches_generic_bitwise)
    # -- a wrong fast path (cached outputs, skipped images) cannot pass this
    torch.cuda.synchronize()
    check_failed = None
    output_check = None
    if args.full and args.batch >= 2 and not args.no_output_check:
        small = det.compile(2, args.size, args.size, device=dev, rescale=True,
                            dtype={'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype])
        pin_note = '' if h16 else pin_check_plan(plan, small)
        if pin_note:
            print('bench.py: output check' + pin_note[2:], file=sys.stderr)
        small.run(img[:2])
        torch.cuda.synchronize()
        for n in range(2):
            k = int(host_count[n])
            if int(small.post['count'][n]) != k:
                check_failed = f'image {n}: batch-{args.batch} step kept {k} detections, batch-2 plan {int(small.post["count"][n])}'
            elif not (torch.equal(small.post['dets'][n, :k].cpu(), host_dets[n, :k]) and
                      torch.equal(small.post['labels'][n, :k].cpu().to(torch.int32), host_labels[n, :k])):
                check_failed = f'image {n} of the batch-{args.batch} step differs from the batch-2 plan'
        del small
        output_check = f'images 0-1 of the timed batch-{args.batch} step == a batch-2 plan on the same images (bit-exact; ' \
                       f'{int(host_count[0])} + {int(host_count[1])} detections)' + pin_note
        if check_failed:
            output_check = 'FAILED: ' + check_failed
    # image 0's pred maps of the TIMED plan, kept for the oracle leg below (the CPU oracle runs on this box anyway for
    # cpu_baseline): the batch-2 comparison above goes through the same library, so a library that is wrong in a
    # self-consistent way would pass it; the oracle is independent of the library
    pred0 = [v.buf.tensor.view(v.N, v.H, v.W, v.C)[0].permute(2, 0, 1).float().cpu() for v in plan.pred_views] \
        if args.full and getattr(plan, 'pred_views', None) and rank == 0 else None
    dets0 = (int(host_count[0]), host_dets[0].clone(), host_labels[0].clone())

    # the inference numbers are final here: leave the group, free the plan, then let a child measure the train step
    D.finalize()
    train = None
    if args.full and not args.no_train:
        del plan, plans, conv_ops, events, per_layer, post
        det._engines.clear()
        torch.cuda.empty_cache()
        train = train_step_leg(args, rank, local_rank, world)

    if rank == 0:
        total_images = args.batch * world * args.steps
        out = dict(
            metric=f'images/sec (inference) {"YOLOv3" if MODELS[args.model].get("v3") else "YOLOv4"} {args.size}x{args.size}', value=round(total_images / elapsed, 2),
            unit='images/sec', n_gpus=world, steps=args.steps, warmup=args.warmup,
            ms_per_step=round(elapsed / args.steps * 1e3, 3), higher_is_better=True, scaling='weak',
            vs_baseline=vs_published(args, total_images / elapsed), dtype=args.dtype, data='synthetic',
            config=dict(workload=(f'{args.model} (Darknet-53 + YOLOV3Neck + YOLOV3Head, 80 classes) '
                                  if MODELS[args.model].get('v3') else
                                  f'{args.model} (DarknetCSP {MODELS[args.model]["scale"]} + '
                                  f'{MODELS[args.model].get("neck", "YOLOV4Neck")} + YOLOCSPHead, 80 classes) ') +
                                 f'{args.size}x{args.size} {dict(f32="fp32", f16="fp16", bf16="bf16")[args.dtype]} inference, batch {args.batch}/GPU: image -> '
                                 'fused conv path -> decode -> per-class NMS -> detections on host ' +
                                 ('[one hipGraph replay per step] ' if args.graph else '') +
                                 (f'[the step runs as {NS} batch-{nb} plans on {NS} HIP streams, joined at every step] ' if NS > 1 else '') +
                                 ('(BASELINE.json configs[1])' if (args.model, args.size, args.batch, args.dtype) == ('yolov4l', 608, 32, 'f32')
                                  else '(not the headline configuration)'),
                        global_batch=args.batch * world, per_gpu_batch=args.batch, input=f'{args.size}x{args.size}',
                        weights='random init (seed 0), BN statistics fitted on the batch, head bias set for '
                                f'~{ncand:.0f} NMS candidates/image', parallelism=f'replicated weights, batch '
                                f'sharded over {world} rank(s), no collective'),
            full=args.full, ranks=per_rank)
        if roofline is not None:
            out['roofline'] = roofline
        if args.full:
            out.update(output_check=output_check, train_step=train)
            if world == 1 and not args.no_cpu_baseline:
                out['cpu_baseline'] = cpu_baseline(det, args.size)
                if pred0 is not None and not MODELS[args.model].get('v3'):
                    ok, msg = oracle_check(det, img[:1].cpu(), pred0, dets0, args.dtype)
                    out['output_check_oracle'] = ('' if ok else 'FAILED: ') + msg
                    check_failed = check_failed or (None if ok else msg)
            else:
                out['cpu_baseline'] = None
        print(json.dumps(out), flush=True)
        if check_failed:            # the metric line is out; a wrong result still fails the run
            sys.exit(3)


def dump_outputs(path, host_dets, host_labels, host_count, suffix=''):
    """What a caller of the timed path receives for the batch, as float32 arrays: dets (N, max_per_img, 5: x1 y1 x2 y2
    score), labels (N, max_per_img) and count (N).  Rows at and past an image's count are 0 in dets and -1 in labels:
    the NMS kernel leaves them unspecified.  7.2 KB per image."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    count = host_count.numpy().astype(np.int64).reshape(-1)
    valid = np.arange(host_dets.shape[1])[None, :] < count[:, None]
    dets = np.where(valid[:, :, None], host_dets.numpy(), 0).astype(np.float32)
    labels = np.where(valid, host_labels.numpy(), -1).astype(np.float32)
    for name, a in (('dets', dets), ('labels', labels), ('count', count.astype(np.float32))):
        np.save(os.path.join(path, f'{name}{suffix}.npy'), a)


def roofline_block(args, events, events_inside, conv_ops, h16, nb, NS, elapsed):
    """The roofline of the dominant conv tile class from the HIP events of the instrumented steps, and the per-layer sums
    behind --layers."""
    import mmdet_yolov4_amd as pkg
    per_tile = {}
    per_layer = {}

    def tile_of(op):
        d = op.info['desc']
        if op.info.get('fused'):
            return op.info['fused']
        if op.info.get('stem32'):
            return 'stem3x3'
        if h16:
            t = d.tile if d.tile else pkg._lib.lib().yv4_conv_h16_pick_tile(__import__('ctypes').byref(d))
            return pkg._lib.HTILE_NAMES[t]
        t = d.tile if d.tile else pkg._lib.lib().yv4_conv_pick_tile(__import__('ctypes').byref(d))
        return pkg._lib.TILE_NAMES[t]

    for op, e0, e1 in events:
        ms = e0.elapsed_time(e1)
        tile = tile_of(op)
        a = per_tile.setdefault(tile, [0.0, 0.0, 0])
        a[0] += op.flops
        a[1] += ms * 1e-3
        a[2] += 1
        b = per_layer.setdefault(id(op), [op, 0.0, 0, tile])
        b[1] += ms * 1e-3
        b[2] += 1
    conv_flops = sum(v[0] for v in per_tile.values())
    conv_time = sum(v[1] for v in per_tile.values())
    dom = max(per_tile, key=lambda k: per_tile[k][1])
    dflops, dtime, dn = per_tile[dom]
    peak = PEAK_H16_MFMA_TFLOPS if h16 else PEAK_FP32_MFMA_TFLOPS
    dbytes = sum(o.bytes for o, _, _ in events if tile_of(o) == dom)
    n_instr_steps = max(len(events) // len(conv_ops), 1)
    tiles_block = {}
    for tname, (tf, tt, tn) in per_tile.items():
        tb = sum(o.bytes for o, _, _ in events if tile_of(o) == tname)
        tiles_block[tname] = dict(launches_per_step=tn // n_instr_steps, avg_launch_us=round(tt / tn * 1e6, 2),
                                  gflop_per_launch=round(tf / tn / 1e9, 3), algorithmic_bytes_per_launch=round(tb / tn),
                                  tflops=round(tf / tt / 1e12, 1), gbps=round(tb / tt / 1e9, 1),
                                  share_of_conv_time=round(tt / conv_time, 4))
    run_key = f'{args.model}_{args.size}_b{args.batch}_{args.dtype}' + (f'_s{NS}' if NS > 1 else '')
    traffic, traffic_src = pmc_traffic(dom, run_key, dbytes / dn, dn // n_instr_steps)
    kname = {'w3x3': 'conv3x3_wide_f32_kernel', 'wide': 'conv_wide_f32_kernel', 'h16_w3x3': 'conv3x3_wide_h16_kernel', 'h16_wide': 'conv_wide_h16_kernel',
             'h16_pp3x3': 'conv3x3_pp_h16_kernel'}.get(dom, f'conv_mfma_{"h16" if h16 else "f32"}_kernel<{dom}>')
    roofline = dict(bound='mfma', kernel=kname,
                    achieved=round(dflops / dtime / 1e12, 2), peak=peak, unit='TFLOP/s',
                    frac=round(dflops / dtime / 1e12 / peak, 4), traffic=traffic,
                    traffic_source=traffic_src,
                    algorithmic_bytes_per_launch=round(dbytes / dn),
                    launches=dn, avg_launch_us=round(dtime / dn * 1e6, 2),
                    gflop_per_launch=round(dflops / dn / 1e9, 3),
                    all_convs_tflops=round(conv_flops / conv_time / 1e12, 2),
                    all_convs_frac=round(conv_flops / conv_time / 1e12 / peak, 4),
                    conv_share_of_step=round(conv_time / max(len(events) // len(conv_ops), 1) /
                                             (elapsed / args.steps), 4),
                    instrumented_steps=len(events) // len(conv_ops), run_key=run_key, tiles=tiles_block,
                    launch_batch=nb, streams=NS,
                    measured=('HIP events around every conv launch in every %d-th step of the timed region' % max(args.event_every, 1))
                    if events_inside else 'HIP events around every conv launch in instrumented steps AFTER the timed region, one '
                    'part-batch plan at a time (a launch bracketed while another stream\'s kernels share the chip would time the '
                    'mixture); the launches are those of the timed region')
    # which roof bounds the dominant kernel: the higher of its two floors (FLOPs / matrix peak, algorithmic bytes /
    # HBM peak).  fp32: the matrix core by 14x; the 16-bit operands move the small-model / batch-256 configurations
    # (BASELINE.json configs[3]) and most tile classes of YOLOv4-L under the HBM roof
    if dbytes / (PEAK_HBM_GBPS * 1e9) > dflops / (peak * 1e12):
        roofline.update(bound='hbm', achieved=round(dbytes / dtime / 1e9, 1), peak=PEAK_HBM_GBPS, unit='GB/s',
                        frac=round(dbytes / dtime / 1e9 / PEAK_HBM_GBPS, 4),
                        mfma_tflops=round(dflops / dtime / 1e12, 2), mfma_frac=round(dflops / dtime / 1e12 / peak, 4))
    return roofline, per_layer


if __name__ == '__main__':
    main()
