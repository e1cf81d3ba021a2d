"""The host side of training and testing from a config file: the lr schedules against their closed forms, the hook
order of ``register_training_hooks``, ``TextLoggerHook`` + ``LogBuffer`` on a fake runner, ``Config.pretty_text``, the
``key=value`` option parser, the argument checks of ``tools/train.py`` / ``tools/test.py``, ``format_results`` on the
per-image lists, and ``set_random_seed``.  No GPU."""
import importlib.util
import json
import logging
import math
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd.registry import Config, parse_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'yv4_tool_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # (defines main() and does nothing else)
    return mod


class _Opt:
    def __init__(self, lrs):
        self.param_groups = [dict(lr=lr, momentum=0.9) for lr in lrs]


class _Stub:
    """What a hook touches of a runner, driven by hand."""

    def __init__(self, lrs=(0.01,), iters_per_epoch=3, max_epochs=5):
        self.optimizer = _Opt(lrs)
        self.data_loader = [None] * iters_per_epoch
        self.max_epochs, self.epoch, self.iter, self.inner_iter = max_epochs, 0, 0, 0

    @property
    def max_iters(self):
        return self.max_epochs * len(self.data_loader)


def _schedule(hook, lrs=(0.01, 0.002), iters_per_epoch=3, max_epochs=5):
    """The lr of every group at every iteration (as the optimizer hook would see it)."""
    r = _Stub(lrs, iters_per_epoch, max_epochs)
    hook.before_run(r)
    seen = []
    for e in range(max_epochs):
        r.epoch = e
        hook.before_train_epoch(r)
        for i in range(iters_per_epoch):
            r.inner_iter = i
            hook.before_train_iter(r)
            seen.append([g['lr'] for g in r.optimizer.param_groups])
            r.iter += 1
    return seen


def _step_closed_form(base, it, ipe, step, gamma, warmup, warmup_iters, ratio):
    """float64: ``base * gamma**k`` with ``k`` the steps reached at the iteration's epoch; during the first
    ``warmup_iters`` iterations the warm-up form of it."""
    epoch = it // ipe
    k = epoch // step if isinstance(step, int) else sum(epoch >= s for s in step)
    lr = base * gamma ** k
    if warmup is None or it >= warmup_iters:
        return lr
    if warmup == 'constant':
        return lr * ratio
    if warmup == 'linear':
        return lr * (1 - (1 - it / warmup_iters) * (1 - ratio))
    return lr * ratio ** (1 - it / warmup_iters)


@pytest.mark.parametrize('step,warmup,by_epoch_warmup', [([2, 4], 'linear', False), ([2, 4], 'constant', False),
                                                         ([2, 4], 'exp', False), ([2, 4], 'linear', True),
                                                         (3, 'linear', False), ([2, 4], None, False)])
def test_step_lr_equals_the_closed_form(step, warmup, by_epoch_warmup):
    ipe, epochs, bases = 3, 5, (0.01, 0.002)
    kw = dict(warmup=warmup, warmup_iters=2 if by_epoch_warmup else 5, warmup_ratio=0.1,
              warmup_by_epoch=by_epoch_warmup) if warmup else {}
    got = _schedule(H.StepLrUpdaterHook(step=step, gamma=0.1, **kw), bases, ipe, epochs)
    wi = 2 * ipe if by_epoch_warmup else 5
    assert len(got) == ipe * epochs
    for it, lrs in enumerate(got):
        for base, lr in zip(bases, lrs):
            want = _step_closed_form(base, it, ipe, step, 0.1, warmup, wi, 0.1)
            assert lr == pytest.approx(want, rel=1e-15, abs=0), (it, base)
    # the warm-up ends ON the regular lr, and the steps are taken
    assert got[wi][0] == pytest.approx(_step_closed_form(0.01, wi, ipe, step, 0.1, None, 0, 0.1), rel=1e-15)
    assert got[-1][0] < got[wi][0]


def test_step_min_lr_and_bad_arguments():
    r = _Stub()
    r.epoch = 4
    assert H.StepLrUpdaterHook(step=[1, 2], min_lr=0.005).get_lr(r, 0.01) == 0.005
    assert H.StepLrUpdaterHook(step=2, by_epoch=False).get_lr(r, 0.01) == 0.01       # by iteration: none reached
    with pytest.raises(TypeError):
        H.StepLrUpdaterHook(step=1.5)
    with pytest.raises(ValueError, match='cubic'):
        H.StepLrUpdaterHook(step=1, warmup='cubic', warmup_iters=2)
    with pytest.raises(AssertionError):
        H.StepLrUpdaterHook(step=1, warmup='linear', warmup_iters=0)


def test_cosine_without_warmup_is_unchanged_and_takes_the_shared_warmup():
    """Without warm-up: ``min + 0.5 (base - min)(1 + cos(pi * epoch / max_epochs))`` with ``min = base * min_lr_ratio``,
    written at the start of each epoch and nowhere else -- the values of the hook before it had a base class."""
    ipe, epochs, bases = 3, 5, (0.01, 0.002)
    got = _schedule(H.CosineAnnealingLrUpdaterHook(min_lr_ratio=0.2), bases, ipe, epochs)

    def cos(base, e):
        end = base * 0.2
        return end + 0.5 * (base - end) * (math.cos(math.pi * (e / epochs)) + 1)
    for it, lrs in enumerate(got):
        assert lrs == [cos(b, it // ipe) for b in bases]                  # bit for bit: the same expression
    # no write inside the epoch: a value another hook puts into a group survives the iteration
    hook, r = H.CosineAnnealingLrUpdaterHook(min_lr=0.001), _Stub(bases)
    hook.before_run(r)
    hook.before_train_epoch(r)
    r.optimizer.param_groups[0]['lr'] = 123.0
    hook.before_train_iter(r)
    assert r.optimizer.param_groups[0]['lr'] == 123.0
    # by iteration, and with the warm-up of the shared base
    by_iter = _schedule(H.CosineAnnealingLrUpdaterHook(min_lr=0.0, by_epoch=False), (0.01,), ipe, epochs)
    assert by_iter[7][0] == 0.5 * 0.01 * (math.cos(math.pi * (7 / 15)) + 1)
    warm = _schedule(H.CosineAnnealingLrUpdaterHook(min_lr_ratio=0.2, warmup='linear', warmup_iters=4, warmup_ratio=0.5),
                     bases, ipe, epochs)
    for it in range(4):
        e = it // ipe
        assert warm[it][0] == pytest.approx(cos(0.01, e) * (1 - (1 - it / 4) * 0.5), rel=1e-15)
    assert warm[4:] == got[4:]


# ---- register_training_hooks --------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 1)


class _Loader:
    dataset = object()

    def __iter__(self):
        return iter(())


RECIPE = dict(
    lr_config=dict(policy='CosineAnnealing', min_lr_ratio=0.2),
    optimizer_config=dict(type='Fp16GradAccumulateOptimizerHook', nominal_batch_size=64,
                          grad_clip=dict(max_norm=35, norm_type=2), loss_scale='dynamic'),
    checkpoint_config=dict(interval=1),
    log_config=dict(interval=50, hooks=[dict(type='TextLoggerHook')]),
    custom_hooks=[dict(type='StateEMAHook', momentum=0.9999, nominal_batch_size=64, warm_up=10000, priority='HIGH'),
                  dict(type='DetailedLinearWarmUpHook', warmup_iters=10000, priority='NORMAL')])


def _recipe_runner():
    model = _Model()
    r = H.EpochBasedRunner(model, _Opt((0.01,)), max_epochs=2)
    r.register_training_hooks(RECIPE['lr_config'], RECIPE['optimizer_config'], RECIPE['checkpoint_config'],
                              RECIPE['log_config'], None)
    r.register_hook(H.DistSamplerSeedHook())
    r.register_hook(H.EvalHook(_Loader(), interval=1, metric='bbox'))
    for hook_cfg in RECIPE['custom_hooks']:
        r.register_hook_from_cfg(hook_cfg)
    return r


def test_training_hooks_run_in_the_documented_order():
    r = _recipe_runner()
    names = [type(h).__name__ for h in r._hooks]
    # DESIGN 26.2
    assert names == ['CosineAnnealingLrUpdaterHook', 'StateEMAHook', 'Fp16GradAccumulateOptimizerHook', 'CheckpointHook',
                     'DistSamplerSeedHook', 'EvalHook', 'DetailedLinearWarmUpHook', 'IterTimerHook', 'TextLoggerHook']
    assert [h.priority for h in r._hooks] == [10, 30, 40, 50, 50, 50, 50, 70, 90]
    pos = {n: i for i, n in enumerate(names)}
    assert pos['CosineAnnealingLrUpdaterHook'] < pos['Fp16GradAccumulateOptimizerHook']       # lr before the step
    assert pos['CheckpointHook'] < pos['EvalHook']                                            # save_best's last_ckpt
    assert pos['TextLoggerHook'] == len(names) - 1                                            # the loggers run last
    assert r._hooks[-1].interval == 50                                # log_config.interval reaches the logger hook
    assert r._hooks[2].accumulation is None and r._hooks[2].nominal_batch_size == 64
    # a plain optimizer_config block is mmcv's OptimizerHook; 'step' resolves by name
    r2 = H.EpochBasedRunner(_Model(), _Opt((0.01,)), max_epochs=1)
    r2.register_training_hooks(dict(policy='step', step=[8, 11], warmup='linear', warmup_iters=500, warmup_ratio=0.001),
                               dict(grad_clip=dict(max_norm=35, norm_type=2)), dict(interval=1), None)
    assert [type(h).__name__ for h in r2._hooks] == ['StepLrUpdaterHook', 'OptimizerHook', 'CheckpointHook',
                                                     'IterTimerHook']
    assert r2._hooks[0].step == [8, 11] and r2._hooks[0].warmup_iters == 500


def test_what_is_not_built_is_refused_by_name():
    r = H.EpochBasedRunner(_Model(), _Opt((0.01,)), max_epochs=1)
    with pytest.raises(NotImplementedError, match='CyclicLrUpdaterHook'):
        r.register_training_hooks(dict(policy='cyclic'))
    with pytest.raises(NotImplementedError, match='TensorboardLoggerHook'):
        r.register_training_hooks(None, log_config=dict(interval=10, hooks=[dict(type='TensorboardLoggerHook')]))
    with pytest.raises(NotImplementedError, match='momentum_config'):
        r.register_training_hooks(None, momentum_config=dict(policy='cyclic'))
    with pytest.raises(NotImplementedError, match='IterBasedRunner'):
        H.build_runner(dict(type='IterBasedRunner', max_iters=10), default_args=dict(model=_Model()))
    with pytest.raises(NotImplementedError, match='workflow'):
        r.run([], workflow=[('train', 1), ('val', 1)])
    built = H.build_runner(dict(type='EpochBasedRunner', max_epochs=7), default_args=dict(model=_Model(), optimizer=None))
    assert isinstance(built, H.EpochBasedRunner) and built.max_epochs == 7


# ---- LogBuffer, IterTimerHook, TextLoggerHook -------------------------------------------------------------------------------
def test_log_buffer_average_and_clear():
    buf = H.LogBuffer()
    buf.update(dict(loss=1.0, acc=10.0), 1)
    buf.update(dict(loss=2.0), 3)
    buf.update(dict(loss=4.0, acc=20.0), 4)
    buf.average(2)
    assert buf.ready and list(buf.output) == ['loss', 'acc']
    assert buf.output['loss'] == (2.0 * 3 + 4.0 * 4) / 7                 # the last two entries OF THE VARIABLE
    assert buf.output['acc'] == (10.0 * 1 + 20.0 * 4) / 5
    buf.average()
    assert buf.output['loss'] == (1.0 + 6.0 + 16.0) / 8
    buf.clear_output()
    assert not buf.ready and not buf.output and len(buf.history) == 3
    buf.clear()
    assert buf.history == []


class _FakeRunner(_Stub):
    def __init__(self, work_dir, logger, meta, iters_per_epoch=5):
        super().__init__((0.01, 0.5), iters_per_epoch, 2)
        self.work_dir, self.logger, self.meta, self.timestamp = work_dir, logger, meta, '20260101_000000'
        self.model = _Model()
        self.log_buffer = H.LogBuffer()
        self.rank = 0

    def current_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]


def _load_json_logs(path):
    """The reader of the reference's ``tools/analysis_tools/analyze_logs.py`` (``load_json_logs``), restated: every line a
    JSON object; lines without ``epoch`` are skipped; per epoch, per key, the list of values."""
    log_dict = dict()
    with open(path) as f:
        for line in f:
            log = json.loads(line.strip())
            if 'epoch' not in log:
                continue
            epoch = log.pop('epoch')
            for k, v in log.items():
                log_dict.setdefault(epoch, dict()).setdefault(k, []).append(v)
    return log_dict


def _drive(runner, hooks, feed, evaluate=None):
    """Two epochs of the stages a runner calls, ``feed(epoch, i)`` -> (log_vars, num_samples) per iteration."""
    runner._hooks = hooks
    for h in hooks:
        h.before_run(runner)
    for e in range(2):
        runner.epoch = e
        for h in hooks:
            h.before_train_epoch(runner)
        for i in range(len(runner.data_loader)):
            runner.inner_iter = i
            for h in hooks:
                h.before_train_iter(runner)
            runner.log_buffer.update(*feed(e, i))
            for h in hooks:
                h.after_train_iter(runner)
            runner.iter += 1
        if evaluate is not None:
            evaluate(runner)
        for h in hooks:
            h.after_train_epoch(runner)


@pytest.mark.parametrize('ignore_last', [True, False])
def test_text_logger_lines_and_json(tmp_path, caplog, ignore_last):
    logger = logging.getLogger(f'yv4_test_text_logger_{ignore_last}')
    logger.setLevel(logging.INFO)
    meta = dict(env_info='a: b', seed=3, exp_name='tiny.py')
    runner = _FakeRunner(str(tmp_path), logger, meta)
    samples = [2, 3, 1, 2, 2]

    def feed(e, i):
        return OrderedDict(loss_cls=float(i + 1), loss=float(10 * e + i)), samples[i]

    def evaluate(r):                         # what EvalHook.evaluate leaves behind
        r.log_buffer.output['bbox_mAP'] = 0.25 + r.epoch
        r.log_buffer.output['bbox_mAP_copypaste'] = '0.250 0.500'
        r.log_buffer.ready = True
    timer, text = H.IterTimerHook(), H.TextLoggerHook(interval=2, ignore_last=ignore_last)
    with caplog.at_level(logging.INFO, logger=logger.name):
        _drive(runner, [timer, text], feed, evaluate)
    lines = [json.loads(ln) for ln in open(tmp_path / '20260101_000000.log.json')]
    assert lines[0] == meta                                                  # the first line is the run's meta
    train = [ln for ln in lines[1:] if ln['mode'] == 'train']
    val = [ln for ln in lines[1:] if ln['mode'] == 'val']
    per_epoch = 2 + (0 if ignore_last else 1)
    assert len(train) == 2 * per_epoch and len(val) == 2 and len(lines) == 1 + len(train) + len(val)
    first = train[0]
    assert list(first)[:4] == ['mode', 'epoch', 'iter', 'lr'] and list(first)[-1] == 'time'
    assert list(first)[-4:] == ['data_time', 'loss_cls', 'loss', 'time'] or list(first)[-5] == 'memory'
    assert first['epoch'] == 1 and first['iter'] == 2 and first['lr'] == 0.01          # the first group's lr
    assert first['loss_cls'] == round((1.0 * 2 + 2.0 * 3) / 5, 5)            # weighted by num_samples
    assert first['loss'] == round((0.0 * 2 + 1.0 * 3) / 5, 5)
    second = train[1]
    assert second['iter'] == 4 and second['loss_cls'] == round((3.0 * 1 + 4.0 * 2) / 3, 5)
    if not ignore_last:                                                      # the ragged tail: its last two entries
        assert train[2]['iter'] == 5 and train[2]['loss_cls'] == round((4.0 * 2 + 5.0 * 2) / 4, 5)
    assert train[per_epoch]['epoch'] == 2 and train[per_epoch]['loss'] == round((10.0 * 2 + 11.0 * 3) / 5, 5)
    assert [v['epoch'] for v in val] == [1, 2] and [v['bbox_mAP'] for v in val] == [0.25, 1.25]
    assert val[0]['bbox_mAP_copypaste'] == '0.250 0.500' and 'time' not in val[0] and val[0]['iter'] == 5
    # the text lines, in mmcv's layout
    text_lines = [r.getMessage() for r in caplog.records]
    t0 = [ln for ln in text_lines if ln.startswith('Epoch [1][2/5]\t')]
    assert len(t0) == 1
    assert t0[0].startswith('Epoch [1][2/5]\tlr: 1.000e-02, eta: 0:00:00, time: 0.000, data_time: 0.000, ')
    assert t0[0].endswith('loss_cls: 1.6000, loss: 0.6000')
    assert any(ln.startswith('Epoch(val) [2][5]\t') and 'bbox_mAP: 1.2500' in ln for ln in text_lines)
    assert 'Exp name: tiny.py' in text_lines
    # the reference's log analysis reads it
    logs = _load_json_logs(tmp_path / '20260101_000000.log.json')
    assert sorted(logs) == [1, 2]
    assert logs[1]['loss_cls'] == [ln['loss_cls'] for ln in train[:per_epoch]]
    assert logs[2]['bbox_mAP'] == [1.25] and logs[1]['mode'] == ['train'] * per_epoch + ['val']
    assert len(logs[1]['time']) == per_epoch and all(t >= 0 for t in logs[1]['time'])


@pytest.mark.parametrize('rank', ['1', '0'])
def test_text_logger_writes_nothing_on_rank_1(tmp_path, caplog, monkeypatch, rank):
    """The runner ``build_runner`` returns, its own ``rank`` on the path: the launcher's ``RANK``, patched."""
    monkeypatch.setenv('RANK', rank)
    logger = logging.getLogger(f'yv4_test_text_logger_rank{rank}')
    logger.setLevel(logging.INFO)
    runner = H.build_runner(dict(type='EpochBasedRunner', max_epochs=2),
                            default_args=dict(model=_Model(), optimizer=_Opt((0.01,)), work_dir=str(tmp_path), logger=logger,
                                              meta=dict(seed=0)))
    assert runner.rank == int(rank)
    runner.timestamp = 'stamp'
    runner.data_loader = [None] * 3
    with caplog.at_level(logging.INFO, logger=logger.name):
        _drive(runner, [H.IterTimerHook(), H.TextLoggerHook(interval=1), H.CheckpointHook(interval=-1)],
               lambda e, i: (dict(loss=1.0), 1))
    if rank == '1':
        assert os.listdir(tmp_path) == [] and not caplog.records
    else:
        assert os.listdir(tmp_path) == ['stamp.log.json'] and len(caplog.records) == 6


def test_root_logger_is_rank_aware(tmp_path, monkeypatch):
    from mmdet_yolov4_amd import apis
    for rank in ('1', '0'):
        monkeypatch.setenv('RANK', rank)
        logger = logging.getLogger('mmdet')
        for h in list(logger.handlers):
            logger.removeHandler(h)
        logger._yv4_initialised = False
        log_file = tmp_path / f'r{rank}.log'
        got = apis.get_root_logger(str(log_file), 'INFO')
        assert got is logger and got is apis.get_root_logger()
        kinds = [type(h).__name__ for h in got.handlers]
        if rank == '0':
            assert kinds == ['StreamHandler', 'FileHandler'] and got.level == logging.INFO
            got.info('hello')
            got.handlers[1].flush()
            assert 'mmdet - INFO - hello' in log_file.read_text()
        else:
            assert kinds == ['StreamHandler'] and got.level == logging.ERROR and not log_file.exists()
    for h in list(logger.handlers):
        h.close()
        logger.removeHandler(h)
    logger._yv4_initialised = False


# ---- Config.pretty_text / dump ------------------------------------------------------------------------------------------------
def test_config_pretty_text_round_trip(tmp_path):
    src = dict(
        model=dict(type='SingleStageDetector', backbone=dict(type='DarknetCSP', scale=[['conv', 'csp'], [None, 1], [8, 16]],
                                                             out_indices=(3, 4, 5)), train_cfg=None),
        data=dict(samples_per_gpu=8, train=dict(pipeline=[dict(type='Resize', img_scale=[(64, 64), (96, 96)]),
                                                          dict(type='Normalize', mean=[0, 0, 0], to_rgb=True)])),
        note='it\'s a "quoted" \\ string\nwith a second line', lr=1e-3, big=float('inf'), one=(1,), empty=[], nothing={},
        resume_from=None, odd={'not-an-identifier': 1, 'class': 2})
    cfg = Config(src)
    text = cfg.pretty_text
    scope = {}
    exec(text, scope)                                                        # valid Python (StateEMAHook execs it)
    assert scope['resume_from'] is None and scope['one'] == (1,)
    path = tmp_path / 'dumped.py'
    cfg.dump(str(path))
    back = Config.fromfile(str(path))
    assert back.to_dict() == cfg.to_dict() == src
    assert isinstance(back.model.backbone.out_indices, tuple) and back.data.train.pipeline[0].img_scale[1] == (96, 96)
    assert back.pretty_text == text                                          # a fixed point
    back.merge_from_dict({'data.samples_per_gpu': 2, 'model.backbone.out_indices': [1, 2], 'new.key': 'x'})
    assert back.data.samples_per_gpu == 2 and back.model.backbone.out_indices == [1, 2] and back.new.key == 'x'
    assert back.model.type == 'SingleStageDetector' and back.data.train.pipeline[1].to_rgb is True
    assert Config.fromfile(str(path)).data.samples_per_gpu == 8
    with pytest.raises(NotImplementedError):
        cfg.dump(str(tmp_path / 'x.yaml'))


def test_cfg_options_parsing_table():
    table = {'a=1': 1, 'a=-2': -2, 'a=1.5': 1.5, 'a=1e-3': 1e-3, 'a=true': True, 'a=False': False, 'a=None': None,
             'a=none': 'none', 'a=x,y': ['x', 'y'], 'a=1,2.5': [1, 2.5], 'a=[1,2]': [1, 2], 'a=[x]': ['x'], 'a=(1,2)': (1, 2),
             'a=[(1,2),(3,4)]': [(1, 2), (3, 4)], 'a="[a,b]"': ['a', 'b'], 'a=bbox_mAP': 'bbox_mAP', 'a=out/r': 'out/r',
             'a=k=v': 'k=v', 'a=[1, 2]': [1, 2]}
    for word, want in table.items():
        got = parse_options([word])['a']
        assert got == want and type(got) is type(want), word
    assert parse_options(['x.y=1', 'z=q']) == {'x.y': 1, 'z': 'q'} and parse_options(None) == {}
    with pytest.raises(ValueError):
        parse_options(['novalue'])
    with pytest.raises(AssertionError):
        parse_options(['a=[(1,2]'])
    train = _tool('train')
    args = train.parse_args(['c.py', '--cfg-options', 'data.samples_per_gpu=4', 'lr_config.step=[8,11]', '--seed', '3'])
    assert args.cfg_options == {'data.samples_per_gpu': 4, 'lr_config.step': [8, 11]} and args.seed == 3
    assert args.dtype == 'fp32' and args.launcher == 'none' and not args.no_validate and args.work_dir is None


# ---- the tools' argument checks -----------------------------------------------------------------------------------------------
def test_tools_check_their_arguments_before_building_anything(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setenv('LOCAL_RANK', '0')
    test, train = _tool('test'), _tool('train')
    missing = str(tmp_path / 'does_not_exist.py')                            # never read: the checks come first
    with pytest.raises(AssertionError, match='at least one operation'):
        test.main([missing, 'x.pth'])
    with pytest.raises(ValueError, match='cannot be both'):
        test.main([missing, 'x.pth', '--eval', 'bbox', '--format-only'])
    with pytest.raises(ValueError, match='pkl'):
        test.main([missing, 'x.pth', '--out', 'results.json'])
    with pytest.raises(NotImplementedError, match='--show'):
        test.main([missing, 'x.pth', '--show'])
    for tool, rest in ((test, ['x.pth', '--eval', 'bbox']), (train, [])):
        for launcher in ('slurm', 'mpi'):
            with pytest.raises(NotImplementedError, match=launcher):
                tool.main([missing] + rest + ['--launcher', launcher])
        with pytest.raises(SystemExit) as e:
            tool.main([missing] + rest)
        assert 'no GPU' in str(e.value.code) and '\n' not in str(e.value.code)
    with pytest.raises(NotImplementedError, match='--gpus'):
        train.main([missing, '--gpus', '2'])
    with pytest.raises(NotImplementedError, match='--gpus'):
        train.main([missing, '--gpu-ids', '0', '1'])
    args = test.parse_args([missing, 'x.pth', '--format-only', '--eval-options', 'jsonfile_prefix=out/r', '--fuse-conv-bn',
                            '--show-dir', 'd', '--show-score-thr', '0.5', '--gpu-collect', '--tmpdir', 't', '--dtype', 'bf16'])
    assert args.eval_options == {'jsonfile_prefix': 'out/r'} and args.fuse_conv_bn and args.show_score_thr == 0.5


# ---- format_results on the per-image lists ------------------------------------------------------------------------------------
def _lists(num_images, num_classes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_images):
        per_class = []
        for c in range(num_classes):
            n = int(rng.integers(0, 4)) if i != 1 else 0                      # image 1 has no detection
            xy = rng.uniform(0, 50, (n, 2))
            wh = rng.uniform(1, 40, (n, 2))
            per_class.append(np.concatenate([xy, xy + wh, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
        out.append(per_class)
    return out


def _det2json_restated(results, img_ids, cat_ids):
    """``datasets/coco.py:175-225`` (``xyxy2xywh`` + ``_det2json``), restated."""
    json_results = []
    for idx in range(len(img_ids)):
        result = results[idx]
        for label in range(len(result)):
            bboxes = result[label]
            for i in range(bboxes.shape[0]):
                b = bboxes[i].tolist()
                json_results.append(dict(image_id=img_ids[idx], bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]],
                                         score=float(bboxes[i][4]), category_id=cat_ids[label]))
    return json_results


def test_format_results_writes_det2json(tmp_path):
    gt = pkg.CocoGt(dict(images=[dict(id=i) for i in (31, 7, 19, 4)],
                         categories=[dict(id=c, name=f'c{c}') for c in (5, 2, 9)], annotations=[]))
    ds = pkg.CocoBBoxDataset(gt, classes=['c5', 'c2', 'c9'])
    results = _lists(4, 3)
    assert sum(len(c) for r in results for c in r) > 8
    files, tmp_dir = ds.format_results(results, jsonfile_prefix=str(tmp_path / 'res'))
    assert tmp_dir is None and files == dict(bbox=str(tmp_path / 'res.bbox.json'), proposal=str(tmp_path / 'res.bbox.json'))
    want = _det2json_restated(results, ds.img_ids, ds.cat_ids)
    with open(files['bbox']) as f:
        text = f.read()
    assert text == json.dumps(want)                                          # the bytes mmcv.dump writes
    got = json.loads(text)
    assert got == want and [sorted(r) for r in got[:1]] == [['bbox', 'category_id', 'image_id', 'score']]
    assert got[0]['bbox'][2] == float(results[0][0][0][2]) - float(results[0][0][0][0])       # formed in double
    # the flat tuple (host arrays) gives the same bytes
    flat_files, _ = ds.format_results(pkg.flatten_results(results), jsonfile_prefix=str(tmp_path / 'flat'))
    with open(flat_files['bbox']) as f:
        assert f.read() == text
    # without a prefix: a temporary directory, handed back
    files, tmp_dir = ds.format_results(results)
    assert os.path.dirname(files['bbox']) == tmp_dir.name and os.path.basename(files['bbox']) == 'results.bbox.json'
    with open(files['bbox']) as f:
        assert f.read() == text
    tmp_dir.cleanup()
    with pytest.raises(AssertionError, match='length of results'):
        ds.format_results(results[:3])
    with pytest.raises(AssertionError, match='must be a list'):
        ds.format_results(dict())


def test_set_random_seed_repeats():
    def draws():
        return random.random(), float(np.random.rand()), torch.rand(3).tolist()
    pkg.set_random_seed(11)
    a = draws()
    b = draws()
    pkg.set_random_seed(11)
    assert draws() == a and a != b
    pkg.set_random_seed(12)
    assert draws() != a
    was = pkg.deterministic()
    try:
        pkg.set_random_seed(11, deterministic=True)
        assert pkg.deterministic() is True and draws() == a
    finally:
        pkg.set_deterministic(was)


def test_init_detector_refuses_other_config_types():
    with pytest.raises(TypeError, match='filename or Config'):
        pkg.init_detector(dict(model=dict()))


def test_imgs_per_gpu_is_taken_with_a_warning(caplog):
    from mmdet_yolov4_amd.apis import broadcast_model_state, samples_per_gpu
    logger = logging.getLogger('yv4_test_imgs_per_gpu')
    cfg = Config(dict(data=dict(imgs_per_gpu=6)))
    with caplog.at_level(logging.WARNING, logger=logger.name):
        assert samples_per_gpu(cfg, logger) == 6 and cfg.data.samples_per_gpu == 6
    assert any('deprecated' in r.getMessage() for r in caplog.records)
    assert samples_per_gpu(Config(dict(data=dict(imgs_per_gpu=6, samples_per_gpu=2))), logger) == 6
    assert samples_per_gpu(Config(dict(data=dict(samples_per_gpu=2))), logger) == 2
    assert broadcast_model_state(_Model()) == 0                              # no process group: nothing is sent


def test_show_dir_with_a_launcher_is_refused_before_anything_is_built(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setenv('LOCAL_RANK', '0')
    with pytest.raises(NotImplementedError, match='--show-dir with a launcher'):
        _tool('test').main([str(tmp_path / 'none.py'), 'x.pth', '--show-dir', 'd', '--launcher', 'pytorch'])


def test_log_buffer_reads_only_the_entries_it_averages():
    """``average(n)`` touches the last ``n`` entries of a variable and no older one (an older pending entry stays
    pending), and a buffer nobody will read keeps nothing."""
    class Lazy(dict):
        reads, pending = 0, True                     # (pending: the buffer keeps the object itself, as a DeferredLogVars)

        def __getitem__(self, k):
            type(self).reads += 1
            return dict.__getitem__(self, k)
    buf = H.LogBuffer()
    for i in range(1000):
        buf.update(Lazy(loss=float(i)), 1)
    buf.average(3)
    assert Lazy.reads == 3 and buf.output['loss'] == 998.0
    off = H.LogBuffer()
    off.keep = False
    off.update(dict(loss=1.0))
    assert off.history == [] and not off.by_name
