"""Fixture: the route table of the convolution front end (tests/test_conv_routes_host.py).

For every descriptor of a sweep, the ten values the library's pure host functions answer: the tile
yv4_conv_pick_tile / yv4_conv_h16_pick_tile / yv4_conv_f8_pick_tile resolve AUTO to, (bytes, ksplit) of
yv4_conv_splitk_workspace and yv4_conv_h16_splitk_workspace, and yv4_conv_wgrad_workspace for f32, f16 and bf16.
None of them launches anything: the library loads, and this script runs, without a GPU.

The sweep:
  * every conv of every model config the repository ships -- the 12 configs of tests/golden/configs_n1.json, bench.py's
    MODELS -- as the descriptors of its fp32 and of its bf16 inference plan (Plan on the CPU device: emitted, never
    finalized), at batch 1, 2, 32 and 64;
  * a grid: Cin x Cout x square map x (1x1 s1, 3x3 s1 p1, 3x3 s2 p1) x batch, dense views.

Run it against the library whose routes are to be pinned -- to check a change of the front end, a build of the commit
BEFORE the change (YV4_LIB_PATH=<that build's libyv4_hip.so>):
    python tests/golden/make_golden_conv_routes.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

DESC_FIELDS = ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad', 'x_cstride', 'x_coff', 'y_cstride',
               'y_coff', 'r_cstride', 'r_coff', 'act1', 'act2', 'flags')
VALUES = ('pick_f32', 'pick_h16', 'pick_f8', 'splitk_f32_bytes', 'splitk_f32_ways', 'splitk_h16_bytes', 'splitk_h16_ways',
          'wgrad_ws_f32', 'wgrad_ws_f16', 'wgrad_ws_bf16')
BATCHES = (1, 2, 32, 64)
GRID_CIN = (4, 16, 32, 64, 128, 256, 512, 1024)
GRID_COUT = (18, 32, 64, 128, 255, 256, 512, 1024)
GRID_MAP = (19, 38, 76, 152, 304, 608)
GRID_KSP = ((1, 1, 0), (3, 1, 1), (3, 2, 1))      # kernel, stride, pad


def routes(L, lib, rows):
    """The table of VALUES (int64, one row per descriptor row) from `lib`."""
    out = np.zeros((len(rows), len(VALUES)), np.int64)
    d = L.ConvDesc()
    ks = C.c_int(0)
    for i, row in enumerate(rows):
        for f, v in zip(DESC_FIELDS, row):
            setattr(d, f, int(v))
        p = C.byref(d)
        v = [lib.yv4_conv_pick_tile(p), lib.yv4_conv_h16_pick_tile(p), lib.yv4_conv_f8_pick_tile(p)]
        for fn in (lib.yv4_conv_splitk_workspace, lib.yv4_conv_h16_splitk_workspace):
            ks.value = -7
            v += [fn(p, C.byref(ks)), ks.value]
        v += [lib.yv4_conv_wgrad_workspace(p, dt) for dt in (L.F32, L.F16, L.BF16)]
        out[i] = v
    return out


def model_rows(pkg):
    import torch
    import bench
    from mmdet_yolov4_amd.plan import Plan
    with open(os.path.join(HERE, 'configs_n1.json')) as f:
        cfgs = {k: (v['model'], 640 if 'yolov5' in k else 608) for k, v in json.load(f).items()}
    for name, size in (('yolov4l', 608), ('yolov4s', 416), ('yolov3', 608), ('yolov5l', 640)):
        cfgs[f'bench:{name}@{size}'] = (bench.model_cfg(name), size)
    rows = []
    for name, (model, size) in cfgs.items():
        det = pkg.build_detector(model).eval()
        for dtype in (torch.float32, torch.bfloat16):
            for n in BATCHES:
                plan = Plan('cpu', dtype)
                det.emit(plan, det._add_image(plan, n, size, size, 'img'))
                for op in plan.ops:
                    if op.kind == 'conv':
                        rows.append([getattr(op.info['desc'], f) for f in DESC_FIELDS])
        print(f'{name}: {len(rows)} rows so far', flush=True)
    return rows


def grid_rows():
    rows = []
    for cin in GRID_CIN:
        for cout in GRID_COUT:
            for hw in GRID_MAP:
                for k, s, p in GRID_KSP:
                    ho = (hw + 2 * p - k) // s + 1
                    for n in BATCHES:
                        rows.append([n, hw, hw, cin, ho, ho, cout, k, k, s, p, cin, 0, cout, 0, 0, 0, 1, 0, 0])
    return rows


def main():
    import mmdet_yolov4_amd as pkg
    L = pkg._lib
    lib = L.lib()
    rows = np.unique(np.asarray(model_rows(pkg), np.int32), axis=0)
    grid = np.asarray(grid_rows(), np.int32)
    desc = np.concatenate([rows, grid])
    table = routes(L, lib, desc)
    path = os.path.join(HERE, 'conv_routes.npz')
    np.savez_compressed(path, desc=desc, routes=table, desc_fields=np.array(DESC_FIELDS), values=np.array(VALUES),
                        n_model_rows=np.int64(len(rows)))
    print(f'{path}: {len(rows)} model rows + {len(grid)} grid rows from {L.LIB_PATH}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
