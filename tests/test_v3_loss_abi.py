"""ABI 8: the YOLOv3 loss entry points (include/yv4.h yv4_yolov3_loss_fwd / _bwd) are exported, bound, and their
descriptor has the header's layout.  No GPU needed."""
import ctypes

import torch

import mmdet_yolov4_amd as pkg

import _abi_probe

# gcc on include/yv4.h: sizeof(yv4_v3_loss_level), sizeof(yv4_v3_loss_desc), then offsetof of the fields below
LEVEL_SIZE, DESC_SIZE = 192, 1128
OFFSETS = dict(num_levels=960, gt_max_assign_all=980, gt=984, pos_iou_thr=1008, eps=1024, loss_weight=1040,
               reduce_mean=1056, img_off=1072, assigned=1104, sums=1112, losses=1120)


def test_v3_loss_symbols_exported_and_bound():
    lib = pkg._lib.lib()
    assert pkg._lib.ABI_VERSION == 8 and lib.yv4_abi_version() == 8
    for name in ('yv4_yolov3_loss_fwd', 'yv4_yolov3_loss_bwd'):
        assert name in pkg._lib.SIGNATURES and name in pkg._lib.FEATURES['v3_loss'].symbols
        assert getattr(lib, name).argtypes == pkg._lib.SIGNATURES[name][1]
    assert pkg._lib.has('v3_loss')


def test_v3_loss_desc_layout_matches_header():
    D, Lv = pkg._lib.V3LossDesc, pkg._lib.V3LossLevel
    assert ctypes.sizeof(Lv) == LEVEL_SIZE and ctypes.sizeof(D) == DESC_SIZE
    assert Lv.sn.offset == 16 and Lv.H.offset == 48 and Lv.base_anchors.offset == 64
    for k, v in OFFSETS.items():
        assert getattr(D, k).offset == v, k


def test_v3_loss_desc_layout_matches_a_c_compiler():
    """The same numbers from a C compiler on the header itself, where one is installed."""
    p = _abi_probe.probe()                                      # skips without a C compiler
    got = [p.sizeof['yv4_v3_loss_level'], p.sizeof['yv4_v3_loss_desc']] + [p.fields['yv4_v3_loss_desc', k][0] for k in OFFSETS]
    assert got == [LEVEL_SIZE, DESC_SIZE] + list(OFFSETS.values())


def test_v3_loss_rejects_bad_descriptors_without_gpu():
    lib = pkg._lib.lib()
    assert lib.yv4_yolov3_loss_fwd(None, None) == -1
    assert b'null' in lib.yv4_last_error()
    d = pkg._lib.V3LossDesc()
    d.num_levels = 6
    assert lib.yv4_yolov3_loss_fwd(ctypes.byref(d), None) == -1
    d.num_levels, d.N, d.A, d.num_classes = 3, 2, 3, 80
    assert lib.yv4_yolov3_loss_bwd(ctypes.byref(d), None, None) == -1
    assert b'work buffers' in lib.yv4_last_error()


def test_v3_fused_loss_gate_on_the_host():
    """CPU maps and a head without train_cfg keep the tensor-op path."""
    cfg = dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0))
    head = pkg.YOLOV3Head(num_classes=4, in_channels=[8, 8, 8], out_channels=[8, 8, 8], train_cfg=cfg)
    maps = [torch.zeros(1, 27, s, s) for s in (2, 4, 8)]
    assert not head._fused_loss_ok(maps)
    assert not pkg.YOLOV3Head(num_classes=4, in_channels=[8, 8, 8], out_channels=[8, 8, 8])._fused_loss_ok(maps)
