"""Training and testing from a config file, on the GPU: ``train_detector`` against the same run assembled by hand,
bit for bit; the artefacts ``tools/train.py`` leaves; no device synchronisation per iteration; resume; the YOLOv3 recipe's
``lr_config``; ``tools/test.py`` as a child; ``init_detector`` + ``inference_detector``; two ranks on one GPU.

The data set is tests/golden/coco_train_set.json + .npz written into a temporary directory (as
tests/test_gpu_train_loader.py does), the detector the tiny YOLOv4 of tests/golden/train_v4 with its 80-class head cut to
the set's three classes (the first three class rows of every anchor), the recipes those of that file at 64 pixels.  Every
test writes its own config file, so ``Config.fromfile`` is on the path."""
import glob
import json
import os
import pickle
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd.optim import build_optimizer
from mmdet_yolov4_amd.registry import Config
from conftest import GOLDEN, arch_from, state_dict_from

import _eval_hook_data as DATA
from test_gpu_train_loader import MOSAIC, V3
from test_gpu_test_loader import TEST

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ('cat', 'dog', 'bird')
BATCH = 3
CHILD_TIMEOUT = 240


# ---- what the runs share ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def data_root(tmp_path_factory, golden):
    g = golden('coco_train_set')
    root = str(tmp_path_factory.mktemp('coco_api_set'))
    os.makedirs(os.path.join(root, 'img'))
    with open(os.path.join(GOLDEN, 'coco_train_set.json')) as f:
        d = json.load(f)
    with open(os.path.join(root, 'ann.json'), 'w') as f:
        json.dump(d, f)
    for im in d['images']:
        with open(os.path.join(root, 'img', im['file_name']), 'wb') as f:
            f.write(g[f"jpg_{im['id']}"].tobytes())
    return root


@pytest.fixture(scope='module')
def start(tmp_path_factory, golden):
    """(model block, path of the checkpoint every run loads): train_v4's weights with a three-class head."""
    g = golden('train_v4')
    stages, reps, chans = arch_from(g)
    sd = state_dict_from(g)
    for k in list(sd):
        if k.startswith('bbox_head.convs_pred.'):
            t = sd[k]
            sd[k] = t.reshape(3, 85, *t.shape[1:])[:, :5 + len(CLASSES)].reshape(3 * (5 + len(CLASSES)), *t.shape[1:]).clone()
    model = dict(type='SingleStageDetector',
                 backbone=dict(type='DarknetCSP', scale=[stages, reps, chans], out_indices=[3, 4, 5]),
                 neck=dict(type='YOLOV4Neck', in_channels=[32, 64, 64], out_channels=[32, 64, 128], csp_repetition=1),
                 bbox_head=dict(type='YOLOCSPHead', num_classes=len(CLASSES), in_channels=[32, 64, 128]), train_cfg=None,
                 test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=300))
    path = str(tmp_path_factory.mktemp('start') / 'start.pth')
    torch.save(dict(meta=dict(), state_dict=sd), path)
    return model, path


OPTIMIZER = dict(type='SGD', lr=0.01, momentum=0.937, weight_decay=0.0005, nesterov=True,
                 paramwise_cfg=dict(bias_decay_mult=0., norm_decay_mult=0.))
OPT_HOOK = dict(type='Fp16GradAccumulateOptimizerHook', nominal_batch_size=BATCH, grad_clip=dict(max_norm=35, norm_type=2),
                loss_scale='dynamic')
EMA = dict(type='StateEMAHook', momentum=0.9, nominal_batch_size=BATCH, warm_up=2, priority='HIGH')
WARMUP = dict(type='DetailedLinearWarmUpHook', warmup_iters=8, priority='NORMAL')      # ends inside the second epoch


def _config(path, data_root, start, **over):
    """The YOLOv4 mosaic recipe at 64 pixels as a config file -> the ``Config`` read back from it."""
    model, ckpt = start

    def block(pipeline, **kw):
        return dict(type='CocoDataset', ann_file='ann.json', data_root=data_root, img_prefix='img/', classes=CLASSES,
                    pipeline=pipeline, **kw)
    cfg = dict(model=model,
               data=dict(samples_per_gpu=BATCH, workers_per_gpu=2, train=block(MOSAIC), val=block(TEST, samples_per_gpu=4),
                         test=block(TEST, samples_per_gpu=4)),
               optimizer=OPTIMIZER, optimizer_config=OPT_HOOK, lr_config=dict(policy='CosineAnnealing', min_lr_ratio=0.2),
               custom_hooks=[EMA, WARMUP], checkpoint_config=None, log_config=None,
               evaluation=dict(interval=1, metric='bbox', save_best='bbox_mAP'),
               runner=dict(type='EpochBasedRunner', max_epochs=2), workflow=[('train', 1)], load_from=ckpt, resume_from=None,
               log_level='INFO', seed=0, work_dir=None, cudnn_benchmark=True, dist_params=dict(backend='nccl'))
    cfg.update(over)
    Config(cfg).dump(str(path))
    return Config.fromfile(str(path))


def _detector(cfg, dev):
    det = pkg.build_detector(cfg.model)
    det.init_weights()
    return det.to(dev)


@pytest.fixture(scope='module', autouse=True)
def _deterministic_mode(gpu_device):
    was = pkg.deterministic()
    yield
    pkg.set_deterministic(was)


def _state(runner):
    """Everything a run leaves: parameters and buffers (``ema_*`` included), momentum buffers, the groups' hyper-parameters."""
    sd = {k: v.detach().clone() for k, v in runner.model.state_dict().items()}
    groups = [{k: v for k, v in g.items() if k != 'params'} for g in runner.optimizer.param_groups]
    return sd, runner.optimizer.momentum_buf.clone(), groups


def _assert_same_state(a, b):
    assert list(a[0]) == list(b[0]) and any(k.startswith('ema_') for k in a[0])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and float(a[1].abs().sum()) > 0
    assert a[2] == b[2]


@pytest.fixture(scope='module')
def straight(tmp_path_factory, data_root, start, gpu_device):
    """Two epochs through ``train_detector`` from a config file, seed 0, deterministic: compared by tests 1 and 4."""
    cfg = _config(tmp_path_factory.mktemp('straight') / 'v4_mosaic.py', data_root, start)
    pkg.set_random_seed(0, deterministic=True)
    runner = pkg.train_detector(_detector(cfg, gpu_device), cfg.data.train, cfg, validate=False)
    assert runner.epoch == 2 and runner.iter == 2 * len(runner.data_loader) and len(runner.data_loader) >= 4
    return cfg, _state(runner), runner.iter


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_train_detector_is_the_hand_assembly(straight, gpu_device):
    cfg, state, _ = straight
    pkg.set_random_seed(0, deterministic=True)
    det = _detector(cfg, gpu_device)
    opt = build_optimizer(det, OPTIMIZER)
    loader = pkg.build_train_loader(cfg.data.train.to_dict(), BATCH, seed=0, device=gpu_device)
    runner = H.Runner(det, opt, max_epochs=2)
    runner.load_checkpoint(cfg.load_from)
    runner.register_hook(H.CosineAnnealingLrUpdaterHook(min_lr_ratio=0.2), 'VERY_HIGH')
    runner.register_hook_from_cfg(WARMUP)
    runner.register_hook_from_cfg(EMA)
    runner.register_hook(H.Fp16GradAccumulateOptimizerHook(nominal_batch_size=BATCH, grad_clip=dict(max_norm=35, norm_type=2),
                                                           loss_scale='dynamic'), 'ABOVE_NORMAL')
    runner.run(loader)
    _assert_same_state(state, _state(runner))
    start_sd = torch.load(cfg.load_from, weights_only=False)['state_dict']
    name = 'backbone.conv0.conv.weight'
    assert not torch.equal(state[0][name].cpu(), start_sd[name])              # and it trained


# ---- 3 and the first half of 4 -----------------------------------------------------------------------------------------------
@H.HOOKS.register_module()
class RecordPendingThenStop(H.Hook):
    """LOWEST: at the epoch's last iteration, after every other hook, which of the stored log variables still wait for
    their copies; then ends the run after its first epoch (the schedules have seen ``max_epochs=2``)."""
    seen = None

    def after_train_iter(self, runner):
        if runner.inner_iter + 1 == len(runner.data_loader):
            deferred = [e for e, _ in runner.log_buffer.history if isinstance(e, pkg.deferred.DeferredLogVars)]
            type(self).seen = dict(pending=[e.pending for e in deferred], iters=runner.inner_iter + 1,
                                   names=[list(OrderedDict.keys(e)) for e in deferred])

    def after_train_epoch(self, runner):
        runner.max_epochs = runner.epoch + 1


@pytest.fixture(scope='module')
def first_epoch(tmp_path_factory, data_root, start, gpu_device):
    work = tmp_path_factory.mktemp('first_epoch')
    cfg = _config(work / 'v4_mosaic.py', data_root, start, work_dir=str(work), checkpoint_config=dict(interval=1),
                  log_config=dict(interval=1000, hooks=[dict(type='TextLoggerHook')]),
                  custom_hooks=[EMA, WARMUP, dict(type='RecordPendingThenStop', priority='LOWEST')])
    pkg.set_random_seed(0, deterministic=True)
    RecordPendingThenStop.seen = None
    runner = pkg.train_detector(_detector(cfg, gpu_device), cfg.data.train, cfg, validate=False, timestamp='t0',
                                meta=dict(config=cfg.pretty_text, seed=0))
    assert runner.epoch == 1
    return cfg, str(work), RecordPendingThenStop.seen, len(runner.data_loader)


def test_no_synchronisation_per_iteration(first_epoch):
    """``interval`` is larger than the epoch: nothing read the log variables, so every one the runner and the optimizer
    hook stored -- the losses and the gradient norm of every iteration -- still waits for its copy when the last
    iteration's hooks have run."""
    _, work, seen, per_epoch = first_epoch
    assert seen['iters'] == per_epoch
    assert len(seen['pending']) == 2 * per_epoch and all(seen['pending'])
    assert sum('loss' in n for n in seen['names']) == per_epoch and sum('grad_norm' in n for n in seen['names']) == per_epoch
    lines = [json.loads(ln) for ln in open(os.path.join(work, 't0.log.json'))]
    assert len(lines) == 1 and lines[0]['seed'] == 0                          # the meta line and no other


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_for_bit(first_epoch, straight, tmp_path, data_root, start, gpu_device):
    _, work, _, per_epoch = first_epoch
    latest = os.path.join(work, 'latest.pth')
    ck = torch.load(latest, map_location='cpu', weights_only=False)
    assert ck['meta']['epoch'] == 1 and ck['meta']['iter'] == per_epoch
    assert len(ck['meta']['detailed_warmup_base']['lr']) == len(ck['optimizer']['param_groups'])
    assert per_epoch < WARMUP['warmup_iters']                                  # resumed INSIDE the warm-up window
    cfg = _config(tmp_path / 'v4_mosaic.py', data_root, start, resume_from=latest, work_dir=str(tmp_path))
    pkg.set_random_seed(0, deterministic=True)
    # (the config text in the meta is where StateEMAHook finds resume_from, as with tools/train.py)
    runner = pkg.train_detector(_detector(cfg, gpu_device), cfg.data.train, cfg, validate=False,
                                meta=dict(config=cfg.pretty_text))
    assert runner.epoch == 2 and runner.iter == straight[2]
    _assert_same_state(straight[1], _state(runner))


# ---- 2, 6, 7: one run of tools/train.py, then tools/test.py, as children ---------------------------------------------------
def _child(args, env=None, **kw):
    return subprocess.Popen([sys.executable] + args, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True, **kw)


def _finish(procs):
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-4000:]
    return outs


@pytest.fixture(scope='module')
def tool_run(tmp_path_factory, data_root, start, gpu_device):
    work = tmp_path_factory.mktemp('tool_run')
    cfg_path = work / 'v4_mosaic.py'
    _config(cfg_path, data_root, start, checkpoint_config=dict(interval=1),
            log_config=dict(interval=2, hooks=[dict(type='TextLoggerHook')]))
    out_dir = str(work / 'out')
    _finish([_child([os.path.join(ROOT, 'tools', 'train.py'), str(cfg_path), '--work-dir', out_dir, '--seed', '0',
                     '--deterministic'])])
    return str(cfg_path), out_dir


def _json_lines(out_dir):
    files = glob.glob(os.path.join(out_dir, '*.log.json'))
    assert len(files) == 1
    return files[0], [json.loads(ln) for ln in open(files[0])]


def _metrics(line):
    return {k: v for k, v in line.items() if k not in ('mode', 'epoch', 'iter', 'lr')}


def test_artefacts_of_a_run(tool_run, gpu_device):
    cfg_path, out_dir = tool_run
    names = set(os.listdir(out_dir))
    assert {'epoch_1.pth', 'epoch_2.pth', 'latest.pth', 'best_bbox_mAP.pth', 'v4_mosaic.py'} <= names
    log_json, lines = _json_lines(out_dir)
    log = log_json[:-len('.json')]
    assert os.path.isfile(log) and len(names) == 7
    text = open(log).read()
    assert 'Epoch [1][2/' in text and 'Epoch(val) [2][' in text and 'Environment info' in text and 'Config:' in text
    dumped = Config.fromfile(os.path.join(out_dir, 'v4_mosaic.py'))
    assert dumped.work_dir == out_dir and dumped.data.samples_per_gpu == BATCH and dumped.resume_from is None
    assert set(lines[0]) >= {'env_info', 'config', 'seed', 'exp_name'} and lines[0]['exp_name'] == 'v4_mosaic.py'
    per_epoch = len(pkg.build_train_loader(dumped.data.train.to_dict(), BATCH, seed=0, device=gpu_device))
    for epoch in (1, 2):
        train = [ln for ln in lines[1:] if ln['mode'] == 'train' and ln['epoch'] == epoch]
        assert [ln['iter'] for ln in train] == list(range(2, per_epoch + 1, 2))
        for ln in train:
            assert list(ln)[:6] == ['mode', 'epoch', 'iter', 'lr', 'memory', 'data_time'] and list(ln)[-1] == 'time'
            assert {'loss_cls', 'loss_conf', 'loss_bbox', 'loss', 'grad_norm'} <= set(ln) and np.isfinite(ln['loss'])
            assert ln['memory'] > 0
        val = [ln for ln in lines[1:] if ln['mode'] == 'val' and ln['epoch'] == epoch]
        assert len(val) == 1
        # the same checkpoint, scored by hand at the loader's batch
        model = pkg.init_detector(dumped, os.path.join(out_dir, f'epoch_{epoch}.pth'), device=gpu_device)
        loader = pkg.build_test_loader(dumped.data.val, device=gpu_device)
        assert loader.samples_per_gpu == 4
        want = loader.dataset.evaluate(pkg.single_gpu_test(model, loader), metric='bbox', logger='silent')
        print('epoch', epoch, 'val line', val[0], 'by hand', dict(want))
        assert _metrics(val[0]) == {k: (round(v, 5) if isinstance(v, float) else v) for k, v in want.items()}
    ck = torch.load(os.path.join(out_dir, 'latest.pth'), map_location='cpu', weights_only=False)
    meta = ck['meta']
    assert tuple(meta['CLASSES']) == CLASSES and meta['epoch'] == 2 and meta['iter'] == 2 * per_epoch
    assert meta['mmdet_yolov4_amd_version'] == pkg.__version__ and meta['seed'] == 0
    scope = {}
    exec(meta['config'], scope)
    assert scope['work_dir'] == out_dir and scope['optimizer']['lr'] == 0.01
    assert os.path.realpath(os.path.join(out_dir, 'latest.pth')) == os.path.realpath(os.path.join(out_dir, 'epoch_2.pth'))
    assert os.path.basename(meta['hook_msgs']['best_ckpt']) in ('epoch_1.pth', 'epoch_2.pth')


@pytest.fixture(scope='module')
def test_children(tool_run, tmp_path_factory):
    """Two children of tools/test.py on ``latest.pth``, side by side: ``--eval bbox --out`` at the config's batch of 4, and
    ``--format-only`` + ``--show-dir`` + ``--out`` at a batch of 1."""
    cfg_path, out_dir = tool_run
    d = tmp_path_factory.mktemp('test_children')
    tool, latest = os.path.join(ROOT, 'tools', 'test.py'), os.path.join(out_dir, 'latest.pth')
    a = _child([tool, cfg_path, latest, '--eval', 'bbox', '--out', str(d / 'r.pkl')])
    b = _child([tool, cfg_path, latest, '--format-only', '--eval-options', f"jsonfile_prefix={d / 'res'}", '--show-dir',
                str(d / 'painted'), '--show-score-thr', '0.001', '--out', str(d / 'r1.pickle'), '--cfg-options',
                'data.test.samples_per_gpu=1'])
    outs = _finish([a, b])
    return str(d), outs


def test_tools_test_as_a_child(tool_run, test_children, gpu_device):
    cfg_path, out_dir = tool_run
    d, outs = test_children
    printed = [ln for ln in outs[0].splitlines() if ln.startswith('OrderedDict(')]
    assert len(printed) == 1
    got = eval(printed[0], dict(OrderedDict=OrderedDict, nan=float('nan')))
    _, lines = _json_lines(out_dir)
    val = [ln for ln in lines[1:] if ln['mode'] == 'val' and ln['epoch'] == 2][0]
    assert {k: (round(v, 5) if isinstance(v, float) else v) for k, v in got.items()} == _metrics(val)
    with open(os.path.join(d, 'r.pkl'), 'rb') as f:
        lists = pickle.load(f)
    assert len(lists) == 17 and all(len(r) == len(CLASSES) for r in lists)
    assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5 for r in lists for a in r)
    assert sum(len(a) for r in lists for a in r) > 0
    # the second child: the result file equals format_results of ITS pickle (a batch of 1: plans of different batch sizes
    # may choose different tiles, so results are compared at equal batch only), from the lists and from the flat table
    with open(os.path.join(d, 'r1.pickle'), 'rb') as f:
        lists1 = pickle.load(f)
    cfg = Config.fromfile(cfg_path)
    cfg.merge_from_dict({'data.test.samples_per_gpu': 1})
    loader = pkg.build_test_loader(cfg.data.test, device=gpu_device)
    ds = loader.dataset
    with open(os.path.join(d, 'res.bbox.json')) as f:
        text = f.read()
    files, tmp_dir = ds.format_results(lists1)
    with open(files['bbox']) as f:
        assert f.read() == text
    tmp_dir.cleanup()
    assert len(json.loads(text)) == sum(len(a) for r in lists1 for a in r) > 0
    model = pkg.init_detector(cfg, os.path.join(out_dir, 'latest.pth'), device=gpu_device)
    flat = pkg.single_gpu_test(model, loader, flat=True)
    assert all(t.is_cuda for t in flat)
    files, tmp_dir = ds.format_results(flat)
    with open(files['bbox']) as f:
        assert f.read() == text
    tmp_dir.cleanup()
    painted = sorted(os.listdir(os.path.join(d, 'painted')))
    assert painted == sorted(i['filename'] for i in ds.data_infos) and len(painted) == 17
    for name, info in zip(painted, sorted(ds.data_infos, key=lambda i: i['filename'])):
        img = pkg.imread(os.path.join(d, 'painted', name), device=gpu_device)
        assert tuple(img.shape) == (info['height'], info['width'], 3)


def test_init_detector_and_inference_detector(tool_run, test_children, gpu_device):
    cfg_path, out_dir = tool_run
    d, _ = test_children
    with open(os.path.join(d, 'r1.pickle'), 'rb') as f:
        lists1 = pickle.load(f)
    latest = os.path.join(out_dir, 'latest.pth')
    model = pkg.init_detector(cfg_path, latest, device='cuda:0', cfg_options={'data.test.samples_per_gpu': 1})
    assert tuple(model.CLASSES) == CLASSES and not model.training and model.cfg.data.test.samples_per_gpu == 1
    assert model.cfg.model.train_cfg is None and next(model.parameters()).is_cuda
    ds = pkg.build_test_loader(model.cfg.data.test).dataset
    pos = max(range(len(lists1)), key=lambda i: sum(len(a) for a in lists1[i]))
    path = os.path.join(ds.img_prefix, ds.data_infos[pos]['filename'])
    got = pkg.inference_detector(model, path)                                # model.cfg.data.test.pipeline
    assert len(got) == len(CLASSES) and sum(len(a) for a in got) > 0
    for a, b in zip(got, lists1[pos]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    explicit = pkg.inference_detector(model, path, test_pipeline=TEST)       # the explicit argument, as before
    assert all(np.array_equal(a, b) for a, b in zip(explicit, got))
    with pytest.warns(UserWarning, match='Class names are not saved'):
        plain = pkg.init_detector(cfg_path, Config.fromfile(cfg_path).load_from)
    assert len(plain.CLASSES) == 80


def test_init_detector_in_bf16(tmp_path, golden, data_root, gpu_device):
    """``dtype=torch.bfloat16`` builds and runs, from a ``Config`` object.  The 16-bit plans want channel counts that are
    multiples of 8, which train_v4's 4-channel stem is not: the tiny YOLOv5 of tests/test_gpu_h16.py, whose checkpoint
    carries no class names."""
    g = golden('tiny_v5')
    stages, reps, chans = arch_from(g)
    ckpt = str(tmp_path / 'v5.pth')
    torch.save(dict(state_dict={'module.' + k: v for k, v in state_dict_from(g).items()}), ckpt)     # a DDP checkpoint
    Config(dict(
        model=dict(type='SingleStageDetector', pretrained='somewhere/backbone.pth',
                   backbone=dict(type='DarknetCSP', scale=[stages, reps, chans], out_indices=[2, 3, 4]),
                   neck=dict(type='YOLOV5Neck', in_channels=[32, 64, 128], out_channels=[32, 64, 128], csp_repetition=1),
                   bbox_head=dict(type='YOLOCSPHead', num_classes=80, in_channels=[32, 64, 128]), train_cfg=None,
                   test_cfg=dict(min_bbox_size=0, nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65),
                                 max_per_img=300)),
        data=dict(test=dict(type='CocoDataset', ann_file='ann.json', data_root=data_root, img_prefix='img/',
                            pipeline=TEST)))).dump(str(tmp_path / 'v5.py'))
    cfg = Config.fromfile(str(tmp_path / 'v5.py'))
    with pytest.warns(UserWarning, match='Class names are not saved'):
        model = pkg.init_detector(cfg, ckpt, dtype=torch.bfloat16)
    assert model.bbox_head.fp16_enabled and model.cfg is cfg and cfg.model.pretrained is None and len(model.CLASSES) == 80
    name, want = next(iter(state_dict_from(g).items()))
    assert torch.equal(model.state_dict()[name].cpu(), want)                  # 'module.' was stripped
    paths = [os.path.join(data_root, 'img', f'{i:06d}.jpg') for i in (1, 2)]
    res = pkg.inference_detector(model, paths)
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5 for r in res for a in r)
    with pytest.raises(ValueError, match='dtype'):
        pkg.init_detector(cfg, None, dtype=torch.int8)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@H.HOOKS.register_module()
class RecordLr(H.Hook):
    """LOWEST: the lr of two groups and the loss as every iteration's optimizer step saw them."""
    rows = []

    def after_train_iter(self, runner):
        groups = runner.optimizer.param_groups
        type(self).rows.append((groups[0]['lr'], groups[-1]['lr'], float(runner.outputs['log_vars']['loss'])))


def test_yolov3_recipe_step_lr_with_warmup(tmp_path, data_root, gpu_device):
    det = DATA.tiny_v3(DATA.make_test_cfg(v3=True), gpu_device)
    sd = det.state_dict()
    det.bbox_head = pkg.YOLOV3Head(
        num_classes=len(CLASSES), in_channels=[64, 32, 16], out_channels=[96, 64, 32],
        loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_conf=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0, reduction='sum'),
        loss_xy=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=2.0, reduction='sum'),
        loss_wh=dict(type='MSELoss', loss_weight=2.0, reduction='sum'),
        train_cfg=dict(assigner=dict(type='GridAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0)),
        test_cfg=DATA.make_test_cfg(v3=True))
    det.load_state_dict(sd)
    det.to(gpu_device)
    base = 0.001
    cfg = Config(dict(
        data=dict(samples_per_gpu=2, workers_per_gpu=2,
                  train=dict(type='CocoDataset', ann_file='ann.json', data_root=data_root, img_prefix='img/',
                             classes=CLASSES, pipeline=V3)),
        optimizer=dict(type='SGD', lr=base, momentum=0.9, weight_decay=0.0005),
        optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=3, warmup_ratio=0.1, step=[1]),
        checkpoint_config=None, log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        custom_hooks=[dict(type='RecordLr', priority='LOWEST')], runner=dict(type='EpochBasedRunner', max_epochs=2),
        workflow=[('train', 1)], load_from=None, resume_from=None, seed=1, work_dir=str(tmp_path)))
    cfg.dump(str(tmp_path / 'v3.py'))
    cfg = Config.fromfile(str(tmp_path / 'v3.py'))
    RecordLr.rows = []
    runner = pkg.train_detector(det, cfg.data.train, cfg, validate=False, timestamp='v3')
    per_epoch = len(runner.data_loader)
    rows = RecordLr.rows
    assert len(rows) == 2 * per_epoch and per_epoch > 3 and all(np.isfinite(r[2]) for r in rows)
    assert type(runner._hooks[1]).__name__ == 'OptimizerHook' and runner.optimizer.param_groups[0]['initial_lr'] == base

    def closed_form(it):
        lr = base * 0.1 ** (1 if it // per_epoch >= 1 else 0)
        return lr * (1 - (1 - it / 3) * (1 - 0.1)) if it < 3 else lr
    for it, (first, last, _) in enumerate(rows):
        assert first == last == pytest.approx(closed_form(it), rel=1e-15), it
    lines = [json.loads(ln) for ln in open(tmp_path / 'v3.log.json')]
    train = [ln for ln in lines if ln.get('mode') == 'train']
    assert [ln['lr'] for ln in train] == [round(closed_form(it), 5) for it in range(2 * per_epoch)]
    assert all('grad_norm' in ln and 'loss_cls' in ln and 'loss_wh' in ln for ln in train)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_gpu(tmp_path, data_root, start):
    cfg_path = tmp_path / 'v4_mosaic.py'
    _config(cfg_path, data_root, start, checkpoint_config=dict(interval=1),
            log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]))
    out_dir = str(tmp_path / 'out')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1', YV4_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(_child([os.path.join(ROOT, 'tools', 'train.py'), str(cfg_path), '--work-dir', out_dir, '--seed', '0',
                             '--launcher', 'pytorch', '--cfg-options', 'runner.max_epochs=1'], env=env))
    outs = _finish(procs)
    names = sorted(os.listdir(out_dir))
    assert len(names) == 6 and {'epoch_1.pth', 'latest.pth', 'best_bbox_mAP.pth', 'v4_mosaic.py'} <= set(names)
    assert sum(n.endswith('.log') for n in names) == 1 and sum(n.endswith('.log.json') for n in names) == 1
    _, lines = _json_lines(out_dir)
    val = [ln for ln in lines[1:] if ln['mode'] == 'val']
    assert len(val) == 1 and val[0]['epoch'] == 1 and 'bbox_mAP' in val[0]
    train = [ln for ln in lines[1:] if ln['mode'] == 'train']
    assert len(train) >= 2 and all(np.isfinite(ln['loss']) for ln in train)
    # rank 1 logs errors only: the run's lines come from one rank
    assert sum('Epoch [1][1/' in out for out in outs) == 1


# ---- ranks that initialise their weights differently train ONE model ----------------------------------------------------------
SEED_WORKER = '''
import hashlib, json, os, sys
sys.path.insert(0, %r)
import torch
import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import dist as D
from mmdet_yolov4_amd.flat_state import FlatState
from mmdet_yolov4_amd.registry import Config
rank, _, world = D.env_world()
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
D.init('nccl', dev)                                   # YV4_DIST_BACKEND=gloo: both ranks on cuda:0
cfg = Config.fromfile(%r)
pkg.set_random_seed(100 + rank, deterministic=True)   # every rank its own random stream, as without --seed
det = pkg.build_detector(cfg.model)
det.init_weights()
det.to(dev)
flat = FlatState.of(det)

def digest():
    return hashlib.sha1(flat.values[:flat.n_param].cpu().numpy().tobytes()).hexdigest()
before = digest()
runner = pkg.train_detector(det, cfg.data.train, cfg, distributed=True, validate=False)
print('RESULT ' + json.dumps(dict(rank=rank, before=before, after=digest(), iters=runner.iter)), flush=True)
D.finalize()
'''


def test_two_ranks_with_different_seeds_train_one_model(tmp_path, data_root, start):
    """No ``load_from``, a different seed on each rank: the ranks' ``init_weights()`` differ, ``train_detector`` hands
    every rank rank 0's parameters and buffers before the run (the reference's DDP wrapper does), and since the exchanged
    gradients are the same on both ranks the parameters are still equal, bit for bit, after the epoch."""
    cfg_path = tmp_path / 'v4_mosaic.py'
    _config(cfg_path, data_root, start, load_from=None, runner=dict(type='EpochBasedRunner', max_epochs=1))
    script = tmp_path / 'worker.py'
    script.write_text(SEED_WORKER % (ROOT, str(cfg_path)))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1', YV4_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(_child([str(script)], env=env))
    outs = [json.loads([ln for ln in out.splitlines() if ln.startswith('RESULT ')][0][7:]) for out in _finish(procs)]
    outs.sort(key=lambda o: o['rank'])
    assert outs[0]['before'] != outs[1]['before']                             # they did start apart
    assert outs[0]['after'] == outs[1]['after'] and outs[0]['after'] != outs[0]['before']
    assert outs[0]['iters'] == outs[1]['iters'] == 3
