"""Host side of the IoU / DIoU / CIoU box losses and SoftFocalLoss in the fused YOLOCSPHead loss: no GPU.

  * the registry entries and heads build from config dicts;
  * the torch restatements (losses.py) against tests/golden/loss_variants.npz, which the reference's classes produced:
    outputs and autograd gradients bit for bit, in float32 and in float64;
  * header, binding and library agree on ``yv4_yolo_loss_fwd_ex`` / ``_bwd_ex`` and on ``yv4_loss_opts``;
  * the ``_ex`` calls reject bad options before a device is touched;
  * ``_fused_loss_ok`` on every supported combination;
  * the coverage conditions of the GPU cases (tests/_loss_variants_ref.py) and the reference's own fp32 error ``e32``.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd import losses as Ls
from mmdet_yolov4_amd.registry import build_loss
from mmdet_yolov4_amd.yolocsp_head import RawPredMap, loss_options

import _abi_probe
import _loss_ref as R
import _loss_variants_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = dict(iou_linear=dict(type='IoULoss', linear=True), iou_log=dict(type='IoULoss', linear=False),
               diou=dict(type='DIoULoss'), ciou=dict(type='CIoULoss'))
# cc on include/yv4.h: sizeof(yv4_loss_opts), then offsetof of its fields in declaration order
OPTS_SIZE = 64
OPTS_OFFSETS = dict(box_kind=0, conf_focal=4, conf_gamma=8, conf_alpha=12, cls_focal=16, cls_gamma=20, cls_alpha=24,
                    reserved=28)
BCE = dict(type='CrossEntropyLoss', use_sigmoid=True)


def focal(weight, gamma=1.5, alpha=0.25, **raw):
    return dict(type='SoftFocalLoss', raw_loss=dict(BCE, loss_weight=weight, **raw), gamma=gamma, alpha=alpha)


def make_head(**kw):
    return pkg.YOLOCSPHead(num_classes=5, in_channels=[8, 8, 8], **kw)


# ---------------------------------------------------------------------------------------------------------------------
def test_box_losses_build_from_config_dicts():
    for cfg, cls in ((dict(type='IoULoss'), Ls.IoULoss), (dict(type='IoULoss', linear=True, eps=1e-5), Ls.IoULoss),
                     (dict(type='DIoULoss', loss_weight=2.0), Ls.DIoULoss), (dict(type='CIoULoss', reduction='sum'), Ls.CIoULoss)):
        loss = build_loss(cfg)
        assert type(loss) is cls
    d = build_loss(dict(type='IoULoss'))
    assert (d.linear, d.eps, d.reduction, d.loss_weight) == (False, 1e-6, 'mean', 1.0)      # the reference's defaults
    for name in ('DIoULoss', 'CIoULoss'):
        d = build_loss(dict(type=name))
        assert (d.eps, d.reduction, d.loss_weight) == (1e-6, 'mean', 1.0)
    with pytest.raises(AssertionError):
        build_loss(dict(type='CIoULoss'))(torch.zeros(1, 4), torch.zeros(1, 4), weight=torch.ones(1))


@pytest.mark.parametrize('cfg', list(V.BOX_CFG.values()), ids=list(V.BOX_CFG))
def test_head_builds_with_every_box_loss(cfg):
    head = make_head(loss_bbox=dict(cfg, loss_weight=3.2))
    assert head.loss_bbox_weight == 3.2 and head.loss_bbox.loss_weight == 1.


def test_head_builds_with_soft_focal_loss():
    head = make_head(loss_conf=focal(64.), loss_cls=focal(32., gamma=2.0), loss_bbox=dict(type='CIoULoss', loss_weight=3.2))
    assert type(head.loss_conf) is Ls.SoftFocalLoss and type(head.loss_cls) is Ls.SoftFocalLoss
    o = loss_options(head)
    assert (o.box_kind, o.conf_focal, o.cls_focal) == (_lib.BOX_CIOU, 1, 1)
    assert (o.conf_gamma, o.conf_alpha, o.cls_gamma, o.cls_alpha) == (1.5, 0.25, 2.0, 0.25)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,sfx', [(torch.float32, ''), (torch.float64, '64')], ids=['float32', 'float64'])
@pytest.mark.parametrize('kind', list(FIXTURE))
def test_restatements_reproduce_the_reference_fixture(kind, dtype, sfx, golden):
    """Outputs AND autograd gradients equal the reference classes' bit for bit (nan where the reference gives nan: CIoU
    on identical boxes is 0 / 0); the restatements keep the reference's expression and slicing order, so no bound is
    needed for the gradients either."""
    g = golden('loss_variants')
    pred = torch.from_numpy(g['pred']).to(dtype).requires_grad_(True)
    target = torch.from_numpy(g['target']).to(dtype)
    assert pred.shape[0] >= 300 and set(np.unique(g['group'])) == {0, 1, 2, 3, 4, 5}
    loss = build_loss(dict(FIXTURE[kind], reduction='none'))(pred, target)
    (grad,) = torch.autograd.grad(loss.sum(), pred)
    np.testing.assert_array_equal(loss.detach().numpy(), g[f'{kind}/loss{sfx}'])
    np.testing.assert_array_equal(grad.numpy(), g[f'{kind}/grad{sfx}'])
    # the fixture holds what it was built to hold
    iou_lin = g['iou_linear/loss']
    assert np.all(iou_lin[g['group'] == 1] == np.float32(1 - 1e-6)) and np.all(iou_lin[g['group'] == 5] == np.float32(1 - 1e-6))
    assert np.all(iou_lin[g['group'] == 2] == 0) and np.isnan(g['ciou/loss'][g['group'] == 2]).sum() >= 1
    mean = build_loss(dict(FIXTURE[kind], loss_weight=2.0))(pred.detach(), target)
    ref = 2.0 * torch.from_numpy(g[f'{kind}/loss{sfx}']).mean()
    assert torch.equal(mean, ref) or (torch.isnan(mean) and torch.isnan(ref))


def test_helper_focal_expression_is_the_soft_focal_loss(golden):
    """The helper's inline SoftFocalLoss expression (used in float64) against the registered class in float32, and the
    class against the reference's fixture."""
    g = golden('softfocal')
    gen = torch.Generator().manual_seed(5)
    x, t = torch.randn(64, 7, generator=gen) * 3, torch.rand(64, 7, generator=gen)
    for gamma in (1.0, 1.5, 2.0):
        m = build_loss(dict(type='SoftFocalLoss', raw_loss=dict(BCE, reduction='none'), gamma=gamma, alpha=0.25))
        assert torch.equal(m(x, t), V.bce_or_focal(x, t, (gamma, 0.25)))
    assert set(g.files) and torch.equal(V.bce_or_focal(x, t, None), torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none'))


# ---------------------------------------------------------------------------------------------------------------------
def test_loss_ex_symbols_exported_and_bound():
    lib = _lib.lib()
    assert _lib.ABI_VERSION == 8 and lib.yv4_abi_version() == 8
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    for name in ('yv4_yolo_loss_fwd_ex', 'yv4_yolo_loss_bwd_ex'):
        assert name in _lib.SIGNATURES and name in _lib.FEATURES['loss_ex'].symbols and f'int {name}(' in text
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.has('loss_ex')
    assert ctypes.sizeof(_lib.LossDesc) == 1016
    for i, k in enumerate(('GIOU', 'IOU_LINEAR', 'IOU_LOG', 'DIOU', 'CIOU')):
        assert f'#define YV4_BOX_{k} {i}' in text and getattr(_lib, 'BOX_' + k) == i


def test_loss_opts_layout_matches_a_c_compiler():
    O_ = _lib.LossOpts
    assert ctypes.sizeof(O_) == OPTS_SIZE
    for k, v in OPTS_OFFSETS.items():
        assert getattr(O_, k).offset == v, k
    assert [f[0] for f in O_._fields_] == list(OPTS_OFFSETS)
    p = _abi_probe.probe()                                      # skips without a C compiler
    got = [p.sizeof['yv4_loss_opts'], p.sizeof['yv4_loss_desc']] + [p.fields['yv4_loss_opts', k][0] for k in OPTS_OFFSETS]
    assert got == [OPTS_SIZE, 1016] + list(OPTS_OFFSETS.values())


def test_loss_ex_rejects_bad_options_without_gpu():
    lib = _lib.lib()
    d = _lib.LossDesc()
    d.num_levels, d.N, d.A, d.num_classes = 3, 2, 3, 80
    assert lib.yv4_yolo_loss_fwd_ex(ctypes.byref(d), None, None) == -1
    assert b'null options' in lib.yv4_last_error()
    assert lib.yv4_yolo_loss_bwd_ex(ctypes.byref(d), None, None, None) == -1
    assert lib.yv4_yolo_loss_fwd_ex(None, ctypes.byref(_lib.LossOpts()), None) == -1
    assert b'null' in lib.yv4_last_error()

    def rejected(what, **kw):
        o = _lib.LossOpts()
        for k, v in kw.items():
            setattr(o, k, v)
        for rc in (lib.yv4_yolo_loss_fwd_ex(ctypes.byref(d), ctypes.byref(o), None),
                   lib.yv4_yolo_loss_bwd_ex(ctypes.byref(d), ctypes.byref(o), None, None)):
            assert rc == -1 and what in lib.yv4_last_error(), (kw, lib.yv4_last_error())

    rejected(b'box_kind', box_kind=5)
    rejected(b'box_kind', box_kind=-1)
    rejected(b'gamma', conf_focal=1, conf_gamma=0.5, conf_alpha=0.25)
    rejected(b'gamma', cls_focal=1, cls_gamma=0.99, cls_alpha=0.25)
    rejected(b'gamma', cls_focal=1, cls_gamma=float('nan'), cls_alpha=0.25)
    rejected(b'alpha', conf_focal=1, conf_gamma=1.5, conf_alpha=1.5)
    rejected(b'alpha', cls_focal=1, cls_gamma=2.0, cls_alpha=-0.1)
    # valid options get past the option checks: the descriptor (no work buffers) is what is refused then
    o = _lib.LossOpts()
    o.box_kind, o.conf_focal, o.conf_gamma, o.conf_alpha = _lib.BOX_CIOU, 1, 1.0, 0.0
    assert lib.yv4_yolo_loss_fwd_ex(ctypes.byref(d), ctypes.byref(o), None) == -1
    assert b'work buffers' in lib.yv4_last_error()
    o = _lib.LossOpts()                      # a switched-off focal term's gamma / alpha are not looked at
    o.conf_gamma = 0.25
    assert lib.yv4_yolo_loss_fwd_ex(ctypes.byref(d), ctypes.byref(o), None) == -1
    assert b'work buffers' in lib.yv4_last_error()


# ---------------------------------------------------------------------------------------------------------------------
def _raw_maps(head):
    return [RawPredMap(torch.zeros(1, 32, s, s).contiguous(memory_format=torch.channels_last), torch.zeros(30), 3, 10)
            for s in (8, 4, 2)]


def test_fused_gate_accepts_every_supported_combination():
    kinds = {}
    for name, box in V.BOX_CFG.items():
        for conf in (dict(BCE, loss_weight=64.), focal(64.), focal(64., gamma=1.0), focal(64., gamma=2.0)):
            for cls in (dict(BCE, loss_weight=32.), focal(32.), focal(32., gamma=2.0, alpha=0.5)):
                head = make_head(loss_bbox=dict(box, loss_weight=3.2), loss_conf=conf, loss_cls=cls)
                assert head._fused_loss_ok(_raw_maps(head)), (name, conf, cls)
                kinds[name] = loss_options(head).box_kind
                assert not head._fused_loss_ok([torch.zeros(1, 30, 8, 8)] * 3)          # dense maps: tensor-op path
    assert kinds == dict(giou=0, iou_linear=1, iou_log=2, diou=3, ciou=4)
    agn = pkg.YOLOCSPHead(num_classes=5, in_channels=[8, 8, 8], class_agnostic=True, loss_conf=focal(64.),
                          loss_bbox=dict(type='DIoULoss', loss_weight=3.2))
    maps = [RawPredMap(torch.zeros(1, 16, s, s).contiguous(memory_format=torch.channels_last), torch.zeros(15), 3, 5)
            for s in (8, 4, 2)]
    assert agn._fused_loss_ok(maps) and loss_options(agn).cls_focal == 0


def test_fused_gate_refuses_what_the_kernels_do_not_cover(monkeypatch):
    for kw in (dict(loss_conf=focal(64., gamma=0.5)), dict(loss_cls=focal(32., gamma=0.5)),
               dict(loss_conf=focal(64., class_weight=[2.0])), dict(loss_cls=dict(BCE, class_weight=[1.0] * 5)),
               dict(loss_cls=focal(32., reduction='sum')), dict(loss_bbox=dict(type='CIoULoss', reduction='sum'))):
        head = make_head(**kw)
        assert not head._fused_loss_ok(_raw_maps(head)), kw
    head = make_head(loss_bbox=dict(type='CIoULoss'), loss_conf=focal(64.))
    assert head._fused_loss_ok(_raw_maps(head))
    monkeypatch.setenv('YV4_FUSED_LOSS', '0')
    assert not head._fused_loss_ok(_raw_maps(head))


def test_tensor_op_path_runs_every_variant_on_the_cpu():
    """What a configuration off the fused kernels computes: ``head.loss`` on dense CPU maps equals the helper's
    float32 reference (same expression order) for CIoU + SoftFocalLoss, to fp32 accuracy."""
    case, inputs, r64, e32 = V.references('v_dups', 'ciou-conf1.5-cls1.5')
    head = pkg.YOLOCSPHead(num_classes=case.C, in_channels=[8] * 3, featmap_strides=case.strides,
                           anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=case.base_sizes, strides=case.strides),
                           loss_bbox=dict(type='CIoULoss', loss_weight=V.W_BBOX), loss_conf=focal(V.W_CONF),
                           loss_cls=focal(V.W_CLS)).train()
    out = head.loss(R.dense_maps(case, inputs), case.boxes, case.labels, None)
    for l in range(case.L):
        bal = float(head.conf_level_balance_weight[l])
        got = torch.stack([out['loss_cls'][l].reshape(()), out['loss_conf'][l].reshape(()) / bal, out['loss_bbox'][l].reshape(())])
        assert R.err(got, r64.losses[l]) <= 1e-5, (l, got, r64.losses[l])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(V.CASES) + ['v_dups'])
def test_gpu_case_coverage(name):
    """No case can pass by being empty: positives on every level, an anchor box with two positives (the winner row),
    the intended branches of the hand-built case in float64, CIoU away from its 0 / 0 point.  Nothing is filtered."""
    case = V.check_coverage(name)
    if name == 'v_coco':
        assert case.C == 80 and case.L == 3 and case.N >= 8
    if name == 'v_nonsquare_agnostic':
        assert case.H != case.W and case.C == 0 and case.attr == 5
    if name == 'v_dups':             # positives sharing an anchor box are copies of one box
        gtb = torch.cat(case.boxes)
        for l, asg in enumerate(case.assign):
            key = asg.img * 10 ** 6 + asg.anchor
            for k in key.unique():
                boxes = gtb[asg.g[key == k]]
                assert bool((boxes == boxes[0]).all()), f'{name} level {l}: different boxes share an anchor box'
    print(name, 'G', case.G, 'positives per level', [a.slot.numel() for a in case.assign])


@pytest.mark.parametrize('tag', list(V.CONFIGS))
@pytest.mark.parametrize('name', list(V.CASES))
def test_reference_float32_against_float64(name, tag):
    """``e32`` per case, configuration and tensor: finite and of fp32 size."""
    case, inputs, r64, e32 = V.references(name, tag)
    assert r64.losses.dtype == torch.float64 and all(d.dtype == torch.float64 for d in r64.draw)
    assert bool(torch.isfinite(r64.losses).all()) and all(bool(torch.isfinite(d).all()) for d in r64.draw)
    print(f'{name} {tag}: e32 losses', [[f'{v:.2e}' for v in row] for row in e32.losses.tolist()])
    print(f'{name} {tag}: e32 conf_t {[f"{v:.2e}" for v in e32.conf_t]} draw {[f"{v:.2e}" for v in e32.draw]} '
          f'dbias {[f"{v:.2e}" for v in e32.dbias]}')
    every = e32.losses.reshape(-1).tolist() + e32.conf_t + e32.draw + e32.dbias
    assert all(math.isfinite(v) and v < 1e-3 for v in every), every
    assert max(e32.draw) > 0
    c = V.CONFIGS[tag]
    if c.conf or c.cls:              # the focal terms change the numbers they are meant to change
        _, _, plain, _ = V.references(name, c.kind) if c.kind != 'giou' else (None, None, None, None)
        if plain is not None:
            col = 1 if c.conf else 0
            if col == 1 or case.C > 0:
                assert float((plain.losses[:, col] - r64.losses[:, col]).abs().min()) > 0
