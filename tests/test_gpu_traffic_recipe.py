"""The traffic-sign recipe (``configs/tencent/tencent_traffic_sign_yolov4l.py``, parsed into
tests/golden/custom_sets_recipe.json) end to end at toy width: its keys -- ``TrafficSignDataset`` over a ``.circle``
folder, the mosaic pipeline with ``RandomScale(scale_limit=(-0.5, 0))``, ``out_indices=[2, 3, 4, 5]``, a four-level neck,
four strides with one anchor each, ``class_agnostic=True``, ``num_classes=1``, ``evaluation=dict(metric='mAP')`` -- with
the widths cut to ``[4, 8, 16, 32, 64, 64]``, the sizes to 64-pixel tiles and ``score_thr`` to 0.001, fp32.  Two epochs through
``train_detector(validate=True)`` in deterministic mode, twice (the flat and the list validation loop), then
``tools/test.py --eval mAP`` as a child; and the head's inference and loss on that four-level, one-anchor, class-agnostic
shape against the CPU oracle, within the bounds the three-level tests use (tests/test_gpu_fused_loss.py: 2e-5;
tests/test_gpu_parity.py: labels exactly, boxes and scores 1e-5)."""
import copy
import json
import os
import pickle
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd.registry import Config
from mmdet_yolov4_amd.yolocsp_head import RawPredMap
from oracle import yolov4_oracle as O
from conftest import GOLDEN
from _custom_sets_data import jpgs_of, write_tree
from test_gpu_fused_loss import flat, random_gts, run_pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
STRIDES = [4, 8, 16, 32]
BASE = [[(8, 8)], [(16, 16)], [(32, 32)], [(64, 64)]]
BALANCE = [4.0, 4.0, 1.0, 0.4]


@pytest.fixture(scope='module')
def recipe():
    with open(os.path.join(GOLDEN, 'custom_sets_recipe.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def root(tmp_path_factory, golden):
    return write_tree(str(tmp_path_factory.mktemp('traffic_recipe') / 'sets'), jpgs_of(golden('custom_sets')))


@pytest.fixture(scope='module', autouse=True)
def _deterministic_mode(gpu_device):
    was = pkg.deterministic()
    yield
    pkg.set_deterministic(was)


def _toy(recipe, root):
    """The recipe's blocks with the widths and the sizes replaced, nothing else."""
    model = copy.deepcopy(recipe['model'])
    assert model['backbone']['out_indices'] == [2, 3, 4, 5] and model['backbone']['scale'][2] == [16, 32, 64, 128, 256, 256]
    model['backbone']['scale'] = [model['backbone']['scale'][0], [None, 1, 1, 1, 1, 1], [4, 8, 16, 32, 64, 64]]
    model['neck'].update(in_channels=[16, 32, 64, 64], out_channels=[16, 32, 64, 128])
    model['bbox_head']['in_channels'] = [16, 32, 64, 128]
    head = model['bbox_head']
    assert head['class_agnostic'] is True and head['num_classes'] == 1 and head['featmap_strides'] == STRIDES
    assert [[tuple(a) for a in lv] for lv in head['anchor_generator']['base_sizes']] == BASE
    assert model['train_cfg']['conf_level_balance_weight'] == BALANCE
    # six iterations from fresh weights leave every objectness below the recipe's score_thr=0.3 (no detection, mAP 0 on
    # both sides of every comparison below): the toy scores from 0.001, so that the validation loops have rows to score
    assert model['test_cfg']['score_thr'] == 0.3
    model['test_cfg']['score_thr'] = 0.001

    def sized(t):
        t = copy.deepcopy(t)
        if t['type'] == 'MosaicPipeline':
            for s in t['individual_pipeline']:
                if s['type'] == 'Resize':
                    s['img_scale'] = (64, 64)
        if t['type'] == 'Albu':
            for a in t['transforms']:
                a.update({'PadIfNeeded': dict(min_height=192, min_width=192), 'RandomCrop': dict(width=128, height=128),
                          'CenterCrop': dict(width=64, height=64)}.get(a['type'], {}))
                assert a['type'] != 'RandomScale' or list(a['scale_limit']) == [-0.5, 0]
        if t['type'] == 'MultiScaleFlipAug':
            t['img_scale'] = (96, 64)
        return t
    data = dict(samples_per_gpu=2, workers_per_gpu=2)
    for part in ('train', 'val', 'test'):
        block = copy.deepcopy(recipe['data'][part])
        assert block['type'] == 'TrafficSignDataset'
        block.update(ann_file=os.path.join(root, 'circle'), img_prefix=os.path.join(root, 'circle_img'),
                     pipeline=[sized(t) for t in block['pipeline']])
        data[part] = block
    return model, data


def _config(path, recipe, root, **over):
    model, data = _toy(recipe, root)
    cfg = dict(model=model, data=data,
               optimizer=dict(type='SGD', lr=0.01, momentum=0.937, weight_decay=0.0005, nesterov=True,
                              paramwise_cfg=dict(bias_decay_mult=0., norm_decay_mult=0.)),
               optimizer_config=dict(type='Fp16GradAccumulateOptimizerHook', nominal_batch_size=2,
                                     grad_clip=dict(max_norm=35, norm_type=2), loss_scale='dynamic'),
               lr_config=dict(policy='CosineAnnealing', min_lr_ratio=0.2), checkpoint_config=dict(interval=1),
               log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
               evaluation=dict(interval=1, metric=recipe['evaluation']['metric']),
               runner=dict(type='EpochBasedRunner', max_epochs=2), workflow=[('train', 1)], load_from=None, resume_from=None,
               log_level='INFO', seed=0, work_dir=None)
    cfg.update(over)
    Config(cfg).dump(str(path))
    return str(path)


def _train(cfg_path, work, gpu_device, flat_loop):
    cfg = Config.fromfile(cfg_path)
    cfg.work_dir = work
    cfg.evaluation['flat'] = flat_loop
    pkg.set_random_seed(0, deterministic=True)
    det = pkg.build_detector(cfg.model)
    det.init_weights()
    runner = pkg.train_detector(det.to(gpu_device), cfg.data.train, cfg, validate=True, timestamp='t0', meta=dict(seed=0))
    assert runner.epoch == 2 and len(runner.data_loader) == 3 and runner.iter == 6
    assert isinstance(runner.data_loader.dataset, pkg.TrafficSignDataset)
    with open(os.path.join(work, 't0.log.json')) as f:
        lines = [json.loads(ln) for ln in f]
    return {k: v.detach().cpu().clone() for k, v in runner.model.state_dict().items()}, lines[1:]


@pytest.fixture(scope='module')
def runs(tmp_path_factory, recipe, root, gpu_device):
    d = tmp_path_factory.mktemp('traffic_runs')
    cfg_path = _config(d / 'traffic_toy.py', recipe, root)
    out = []
    for name, flat_loop in (('flat', True), ('lists', False)):
        work = str(d / name)
        os.makedirs(work)
        out.append((work,) + _train(cfg_path, work, gpu_device, flat_loop))
    return cfg_path, out


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_recipe_trains_validates_and_repeats(runs):
    _, ((work, state, lines), (work_b, state_b, lines_b)) = runs
    assert {'epoch_1.pth', 'epoch_2.pth', 'latest.pth', 't0.log.json'} <= set(os.listdir(work))
    train = [ln for ln in lines if ln['mode'] == 'train']
    assert [(ln['epoch'], ln['iter']) for ln in train] == [(e, i) for e in (1, 2) for i in (1, 2, 3)]
    for ln in train:
        assert {'loss_conf', 'loss_bbox', 'loss', 'grad_norm'} <= set(ln) and 'loss_cls' not in ln      # class-agnostic
        assert all(np.isfinite(ln[k]) for k in ('loss_conf', 'loss_bbox', 'loss'))
    val = [ln for ln in lines if ln['mode'] == 'val']
    assert [ln['epoch'] for ln in val] == [1, 2] and all({'AP50', 'mAP'} <= set(ln) for ln in val)
    assert all(0.0 <= ln['mAP'] <= 1.0 for ln in val)
    print('val', [(ln['AP50'], ln['mAP']) for ln in val])
    # two runs, identical final weights; the flat and the list validation loop, equal metrics
    assert list(state) == list(state_b)
    for k in state:
        assert torch.equal(state[k], state_b[k]), k
    val_b = [ln for ln in lines_b if ln['mode'] == 'val']
    assert [(ln['AP50'], ln['mAP']) for ln in val] == [(ln['AP50'], ln['mAP']) for ln in val_b]
    ck = torch.load(os.path.join(work, 'epoch_2.pth'), map_location='cpu', weights_only=False)
    name = 'bbox_head.convs_pred.0.weight'
    assert tuple(ck['state_dict'][name].shape)[:2] == (5, 16) and len([k for k in state if 'convs_pred' in k]) == 8
    assert torch.equal(ck['state_dict'][name], state[name])


def test_tools_test_reproduces_the_last_logged_map(runs):
    cfg_path, ((work, _, lines), _) = runs
    out_file = os.path.join(work, 'results.pkl')            # (--out: the child runs the list loop; the log's value is the flat one's)
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfg_path, os.path.join(work, 'epoch_2.pth'),
                          '--eval', 'mAP', '--out', out_file], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    try:
        out, _ = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        p.kill()
        raise
    assert p.returncode == 0, out[-4000:]
    printed = [ln for ln in out.splitlines() if ln.startswith('OrderedDict(')]
    assert len(printed) == 1
    got = eval(printed[0], dict(OrderedDict=OrderedDict, nan=float('nan')))
    last = [ln for ln in lines if ln['mode'] == 'val' and ln['epoch'] == 2][0]
    assert {k: round(float(v), 5) for k, v in got.items()} == {k: last[k] for k in ('AP50', 'mAP')}
    with open(out_file, 'rb') as f:
        lists = pickle.load(f)
    assert len(lists) == 8 and all(len(r) == 1 for r in lists) and sum(len(r[0]) for r in lists) > 0


def test_flat_and_list_loops_score_alike_on_the_trained_weights(runs, gpu_device):
    """Six iterations give no true positive at IoU 0.5 (the logged mAP is 0 on every side), so the two validation loops
    are also compared where rows do match: the final checkpoint scored at IoU 0.05 and 0.25."""
    cfg_path, ((work, _, _), _) = runs
    cfg = Config.fromfile(cfg_path)
    model = pkg.init_detector(cfg, os.path.join(work, 'epoch_2.pth'), device=gpu_device)
    loader = pkg.build_test_loader(cfg.data.val, device=gpu_device)
    ds = loader.dataset
    assert isinstance(ds, pkg.TrafficSignDataset) and len(ds) == 8 and ds.accepts_flat
    lists = pkg.single_gpu_test(model, loader)
    table = pkg.single_gpu_test(model, loader, flat=True)
    assert all(t.is_cuda for t in table) and int(table[0].shape[0]) == sum(len(r[0]) for r in lists) > 0
    a = ds.evaluate(lists, metric='mAP', iou_thr=[0.05, 0.25], logger='silent')
    b = ds.evaluate(table, metric='mAP', iou_thr=[0.05, 0.25], logger='silent')
    print('lists', dict(a), 'flat', dict(b))
    assert list(a) == ['AP05', 'AP25', 'mAP'] and dict(a) == dict(b)
    loader.close()


# ---- the head on this shape against the CPU oracle -----------------------------------------------------------------------
def _head(dev, **kw):
    return pkg.YOLOCSPHead(num_classes=1, in_channels=[8, 8, 8, 8], featmap_strides=STRIDES, class_agnostic=True,
                           anchor_generator=dict(type='YOLOV4AnchorGenerator', base_sizes=BASE, strides=STRIDES),
                           loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                           train_cfg=dict(num_obj_per_image=3, conf_level_balance_weight=BALANCE), **kw).to(dev)


def test_four_level_one_anchor_agnostic_loss_matches_oracle(gpu_device):
    """As tests/test_gpu_fused_loss.py::test_fused_loss_matches_oracle_fp32, on four levels of one 5-attribute anchor
    (pixel stride 8: three channels of padding) at 96 pixels: 24, 12, 6 and 3 cells."""
    N, img = 3, 96
    head = _head(gpu_device).train()
    assert head.num_attrib == 5 and head.num_anchors == [1, 1, 1, 1] and not hasattr(head, 'loss_cls')
    g = torch.Generator().manual_seed(21)
    maps, leaves = [], []
    for s in STRIDES:
        raw = (torch.randn(N, 8, img // s, img // s, generator=g) * 1.5).to(gpu_device).contiguous(
            memory_format=torch.channels_last).requires_grad_(True)
        bias = (torch.randn(5, generator=g) * 0.5).to(gpu_device).requires_grad_(True)
        maps.append(RawPredMap(raw, bias, 1, 5))
        leaves.append((raw, bias))
    gts, labels = random_gts(N, img, 1, 22)
    gts[0] = torch.tensor([[20., 20., 44., 44.], [21., 21., 45., 43.], [0., 0., 14., 12.], [24., 40., 40., 56.]])
    labels[0] = torch.zeros(4, dtype=torch.long)
    weights = dict(loss_conf=[0.9, 1.1, 1.0, 0.8], loss_bbox=[1.2, 1.0, 0.8, 1.1])
    dense = [(raw.detach()[:, :5].float().cpu() + bias.detach().cpu().view(1, -1, 1, 1)).requires_grad_(True)
             for raw, bias in leaves]
    ref = O.head_loss(dense, gts, labels, num_classes=0, base_sizes=BASE, strides=STRIDES, loss_conf_weight=1.0,
                      conf_level_balance_weight=BALANCE)
    sum(w * v.sum() for key in weights for w, v in zip(weights[key], ref[key])).backward()
    out, grads = run_pkg(head, maps, leaves, [b.to(gpu_device) for b in gts], [l.to(gpu_device) for l in labels], weights,
                         fused=True)
    assert 'loss_cls' not in out and float(out['num_gts']) == float(ref['num_gts'])
    for key in weights:
        assert len(out[key]) == 4
        print(key, flat(out, key).tolist(), flat(ref, key).tolist())
        np.testing.assert_allclose(flat(out, key), flat(ref, key), rtol=2e-5, atol=1e-7)
    for (draw, dbias), d in zip(grads, dense):
        dref = d.grad
        assert float((draw[:, :5].float().cpu() - dref).abs().max()) <= 2e-5 * float(dref.abs().max())
        assert float(draw[:, 5:].abs().max()) == 0
        bref = dref.sum((0, 2, 3))
        assert float((dbias.cpu() - bref).abs().max()) <= 2e-5 * float(bref.abs().max()) + 1e-7


def test_four_level_one_anchor_agnostic_inference_matches_oracle(gpu_device, recipe):
    test_cfg = recipe['model']['test_cfg']
    assert test_cfg['nms']['iou_threshold'] == 0.1 and test_cfg['score_thr'] == 0.3
    head = _head(gpu_device, test_cfg=test_cfg).eval()
    g = torch.Generator().manual_seed(23)
    preds = [(torch.randn(2, 5, 64 // s, 96 // s, generator=g) * 1.5).to(gpu_device) for s in STRIDES]
    sf = np.array([[1, 1, 1, 1], [1.5, 1.25, 1.5, 1.25]], np.float32)
    res = head.get_bboxes(preds, [dict(scale_factor=sf[i]) for i in range(2)], rescale=True)
    ores = O.get_bboxes([p.cpu() for p in preds], sf, 1, score_thr=0.3, iou_threshold=0.1, max_per_img=300, rescale=True,
                        base_sizes=BASE, strides=STRIDES, nms_pre=-1, class_agnostic=True)
    for n in range(2):
        assert len(ores[n][1]) > 3 and set(ores[n][1].tolist()) == {0}
        np.testing.assert_array_equal(res[n][1].cpu().numpy(), ores[n][1].numpy())
        np.testing.assert_allclose(res[n][0].cpu().numpy(), ores[n][0].numpy(), rtol=1e-5, atol=1e-5)
