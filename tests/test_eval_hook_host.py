"""The evaluation hooks' host logic, without a GPU: the schedule of ``EvalHook`` (eval_hooks.py:115-158), ``_init_rule``,
``save_best`` with ``CheckpointHook``, the runner additions, ``dist.collect_flat`` under a 2-rank gloo group on the CPU,
and the corrected ``metric='proposal'`` message.  The model is a stand-in whose ``simple_test`` returns canned lists and
the dataset records what ``evaluate`` receives."""
import json
import os
import socket
import subprocess
import sys
import textwrap
import warnings

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import dist as D
from mmdet_yolov4_amd import hooks as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeModel(torch.nn.Module):
    """One parameter (the loops ask it for the device); image i's result is one box whose score is i / 10."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.modes = []

    def simple_test(self, img, img_metas, rescale=False):
        assert not self.training and rescale
        return [[np.array([[0, 0, 1, 1, m['i'] / 10]], np.float32), np.zeros((0, 5), np.float32)] for m in img_metas]

    def train_step(self, data, optimizer):
        self.modes.append(self.training)
        return dict(loss=self.w.sum(), log_vars=dict(loss=0.0), num_samples=1)


class FakeDataset:
    def __init__(self, runner_ref, scores=None, n=3):
        self.runner_ref, self.scores, self.n = runner_ref, list(scores or []), n
        self.calls = []          # (epoch + 1, iter + 1, results)

    def __len__(self):
        return self.n

    def evaluate(self, results, logger=None, **kwargs):
        r = self.runner_ref[0]
        self.calls.append((r.epoch + 1, r.iter + 1, results, kwargs))
        score = self.scores[len(self.calls) - 1] if self.scores else 0.5
        return {'bbox_mAP': score, 'loss_val': 1 - score}


class FakeLoader:
    def __init__(self, dataset):
        self.dataset = dataset

    def __iter__(self):
        for i in range(self.dataset.n):
            yield dict(img=[torch.zeros(1, 3, 4, 4)], img_metas=[[dict(i=i)]])


def _runner(tmp_path=None, max_epochs=8, **hook_kw):
    ref = []
    model = FakeModel()
    runner = H.Runner(model, None, max_epochs=max_epochs, work_dir=None if tmp_path is None else str(tmp_path))
    ref.append(runner)
    ds = FakeDataset(ref, scores=hook_kw.pop('scores', None))
    hook = H.EvalHook(FakeLoader(ds), **hook_kw)
    return runner, ds, hook


@pytest.mark.parametrize('start,interval,resumed,expected', [
    (None, 1, 0, [1, 2, 3, 4, 5, 6, 7, 8]),
    (None, 2, 0, [2, 4, 6, 8]),
    (None, 3, 0, [3, 6]),
    (3, 2, 0, [3, 5, 7]),
    (3, 1, 0, [3, 4, 5, 6, 7, 8]),
    (1, 2, 0, [1, 3, 5, 7]),
    (0, 4, 0, [4, 8]),                       # the early call at epoch 0 tests (0 + 1 - 0) % 4 and is refused
    (3, 1, 4, [5, 5, 6, 7, 8]),              # resumed at epoch 4 >= start: evaluated before the first epoch (shown as 5)
    (3, 2, 4, [5, 5, 7]),
    (4, 2, 4, [6, 8]),                       # resumed, but (4 + 1 - 4) % 2 != 0: the flag refuses the early evaluation
    (6, 1, 4, [6, 7, 8]),                    # resumed before start: nothing early
])
def test_epoch_schedule(start, interval, resumed, expected):
    runner, ds, hook = _runner(start=start, interval=interval)
    runner.epoch = resumed
    runner.register_hook(hook)
    runner.run(H.BatchSource([dict()] * 2, 1))
    assert [c[0] for c in ds.calls] == expected
    # the list loop: three images in loader order, the reference's per-class lists
    for c in ds.calls:
        assert len(c[2]) == 3 and [float(r[0][0, 4]) for r in c[2]] == [0.0, np.float32(0.1), np.float32(0.2)]
    assert runner.log_buffer.ready and runner.log_buffer.output['bbox_mAP'] == 0.5
    assert all(runner.model.modes)                    # every training step ran in train mode


def test_iteration_schedule_and_mode_restored():
    runner, ds, hook = _runner(max_epochs=2, interval=3, by_epoch=False, classwise=True)
    runner.register_hook(hook)
    runner.run(H.BatchSource([dict()] * 5, 1))
    assert [c[1] for c in ds.calls] == [3, 6, 9]
    assert ds.calls[0][3] == dict(classwise=True)     # eval_kwargs reach the dataset
    assert all(runner.model.modes) and runner.model.training
    # by_epoch=True ignores iterations and by_epoch=False ignores epochs
    runner, ds, hook = _runner(max_epochs=2, interval=1, by_epoch=False)
    hook.after_train_epoch(runner)
    assert ds.calls == []


def test_hook_helpers_and_runner_additions():
    h = H.Hook()
    r = H.Runner(FakeModel(), None)
    assert r.work_dir is None and r.rank == 0
    assert isinstance(r.log_buffer.output, dict) and r.log_buffer.ready is False
    r.epoch, r.iter = 3, 9
    assert h.every_n_epochs(r, 2) and h.every_n_epochs(r, 4) and not h.every_n_epochs(r, 3)
    assert h.every_n_iters(r, 5) and not h.every_n_iters(r, 3)
    assert not h.every_n_epochs(r, -1) and not h.every_n_iters(r, 0)
    for name in ('EvalHook', 'DistEvalHook', 'CheckpointHook'):
        assert H.HOOKS.get(name) is getattr(H, name)


def test_constructor_checks():
    _, ds, _ = _runner()
    with pytest.raises(ValueError, match='interval must be positive'):
        H.EvalHook(FakeLoader(ds), interval=0)
    with pytest.raises(TypeError, match='dataset'):
        H.EvalHook([1, 2, 3])
    with pytest.warns(UserWarning, match='smaller than 0'):
        hook = H.EvalHook(FakeLoader(ds), start=-2)
    assert hook.start == 0
    d = H.DistEvalHook(FakeLoader(ds), tmpdir='/nowhere', gpu_collect=True, broadcast_bn_buffer=False, metric='bbox')
    assert d.tmpdir == '/nowhere' and d.gpu_collect and not d.broadcast_bn_buffer and d.eval_kwargs == dict(metric='bbox')
    # result form: the dataset's accepts_flat decides, the argument overrides
    assert H.EvalHook(FakeLoader(ds)).use_flat() is False and H.EvalHook(FakeLoader(ds), flat=True).use_flat() is True
    ds.accepts_flat = True
    assert H.EvalHook(FakeLoader(ds)).use_flat() is True and H.EvalHook(FakeLoader(ds), flat=False).use_flat() is False


def test_init_rule_every_branch():
    _, ds, _ = _runner()
    mk = lambda **kw: H.EvalHook(FakeLoader(ds), **kw)      # noqa: E731
    assert mk(save_best='bbox_mAP').rule == 'greater' and mk(save_best='AR@100').rule == 'greater'
    assert mk(save_best='loss_val').rule == 'less'
    assert mk(save_best='loss_val', rule='greater').rule == 'greater'       # an explicit rule wins
    assert mk(save_best='accuracy', rule='less').rule == 'less'
    h = mk(save_best='auto')
    assert h.rule is None and h.key_indicator == 'auto' and not hasattr(h, 'compare_func')
    assert mk(save_best='auto', rule='less').rule == 'less'
    assert not hasattr(mk(), 'rule')                                       # no save_best: no rule at all
    with pytest.raises(KeyError, match='rule must be greater, less or None'):
        mk(save_best='bbox_mAP', rule='max')
    with pytest.raises(ValueError, match='Cannot infer the rule for key accuracy'):
        mk(save_best='accuracy')
    assert H.EvalHook.rule_map['greater'](2, 1) and H.EvalHook.rule_map['less'](1, 2)
    assert H.EvalHook.init_value_map == {'greater': -np.inf, 'less': np.inf}


@pytest.mark.parametrize('save_best,rule,scores,best_epochs', [
    ('bbox_mAP', None, [0.2, 0.1, 0.3], [1, 1, 3]),           # greater: the worse epoch 2 leaves best_ckpt alone
    ('loss_val', None, [0.2, 0.1, 0.3], [1, 1, 3]),           # less on 1 - score: the same epochs win
    ('bbox_mAP', 'less', [0.2, 0.1, 0.3], [1, 2, 2]),
    ('auto', None, [0.2, 0.3, 0.3], [1, 2, 2]),               # auto -> the first key, bbox_mAP -> greater; a tie is no win
])
def test_save_best_and_checkpoint_hook(tmp_path, save_best, rule, scores, best_epochs):
    runner, ds, hook = _runner(tmp_path, max_epochs=3, save_best=save_best, rule=rule, scores=scores)
    seen = []

    class Probe(H.Hook):
        def after_train_epoch(self, r):
            msgs = r.meta['hook_msgs']
            seen.append((msgs['last_ckpt'], msgs['best_ckpt'], msgs['best_score']))
    runner.register_hook(H.CheckpointHook(interval=1, save_optimizer=False))
    runner.register_hook(hook)
    runner.register_hook(Probe(), 'LOW')
    runner.run(H.BatchSource([dict()], 1))
    key = 'bbox_mAP' if save_best == 'auto' else save_best
    assert hook.key_indicator == key
    for e, (last, best, score) in enumerate(seen):
        assert last == str(tmp_path / f'epoch_{e + 1}.pth') and os.path.isfile(last)
        assert best == str(tmp_path / f'epoch_{best_epochs[e]}.pth')
        want = scores[best_epochs[e] - 1]
        assert score == pytest.approx(1 - want if key == 'loss_val' else want)
    link = tmp_path / f'best_{key}.pth'
    assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(seen[-1][1])
    assert torch.load(str(link), weights_only=False)['meta']['epoch'] == best_epochs[-1]


def test_checkpoint_hook_interval_and_rank(tmp_path, monkeypatch):
    runner, _, _ = _runner(tmp_path, max_epochs=4)
    runner.register_hook(H.CheckpointHook(interval=2, save_optimizer=False))
    runner.run(H.BatchSource([dict()], 1))
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith('epoch_')) == ['epoch_2.pth', 'epoch_4.pth']
    assert runner.meta['hook_msgs']['last_ckpt'] == str(tmp_path / 'epoch_4.pth')
    # interval=-1 (the default) never saves; by_epoch=False counts iterations; other ranks write nothing
    out = tmp_path / 'b'
    runner, _, _ = _runner(out, max_epochs=1)
    runner.register_hook(H.CheckpointHook())
    runner.register_hook(H.CheckpointHook(interval=2, by_epoch=False, save_optimizer=False))
    runner.run(H.BatchSource([dict()] * 4, 1))
    assert sorted(os.listdir(out)) == ['iter_2.pth', 'iter_4.pth', 'latest.pth']
    r, _, _ = _runner(None, max_epochs=1)
    r.register_hook(H.CheckpointHook(interval=1))
    with pytest.raises(ValueError, match='work_dir'):
        r.run(H.BatchSource([dict()], 1))
    monkeypatch.setattr(H.Runner, 'rank', property(lambda self: 1))
    runner, _, _ = _runner(tmp_path / 'c', max_epochs=1)
    runner.register_hook(H.CheckpointHook(interval=1))
    runner.run(H.BatchSource([dict()], 1))
    assert not os.path.exists(tmp_path / 'c') and 'hook_msgs' not in runner.meta


def test_contiguous_runs_and_bn_segments():
    assert H.contiguous_runs([]) == []
    assert H.contiguous_runs([(8, 4), (0, 4), (4, 4)]) == [(0, 12)]
    assert H.contiguous_runs([(0, 4), (8, 4), (12, 8), (40, 4)]) == [(0, 4), (8, 20), (40, 44)]
    # a model whose float buffers are BN statistics except one in the middle: two runs, parameters / ints / ema_ left out
    from mmdet_yolov4_amd.flat_state import FlatState
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 1), torch.nn.BatchNorm2d(6), torch.nn.BatchNorm2d(6))
    net[1].register_buffer('other', torch.zeros(5))
    net.register_buffer('ema_x', torch.zeros(7))
    flat = FlatState(net)
    runs = H.bn_stat_runs(net, flat)
    seg = {s.name: s for s in flat.buffer_segments}
    assert set(seg) == {'1.running_mean', '1.running_var', '1.other', '2.running_mean', '2.running_var'}
    assert runs == [(seg['1.running_mean'].offset, seg['1.running_var'].offset + 8),
                    (seg['2.running_mean'].offset, seg['2.running_var'].offset + 8)]
    assert runs[0][0] >= flat.n_param and runs[1][1] <= flat.n_state
    net[2].track_running_stats = False
    assert H.bn_stat_runs(net, flat) == [runs[0]]
    plain = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 1), torch.nn.BatchNorm2d(6), torch.nn.BatchNorm2d(10))
    assert len(H.bn_stat_runs(plain, FlatState(plain))) == 1          # all of them touch: one collective


def test_collect_flat_single_process_drops_padding_and_orders():
    dets = torch.arange(30, dtype=torch.float32).view(6, 5)
    labels = torch.tensor([1, 0, 2, 2, 0, 1])
    pos = torch.tensor([2, 0, 0, 5, 1, 2])
    d, l, i = D.collect_flat(dets, labels, pos, size=5)
    assert i.tolist() == [0, 0, 1, 2, 2] and l.tolist() == [0, 2, 0, 1, 1]
    assert d[:, 0].tolist() == [5., 10., 20., 0., 25.]            # rows of one position keep their order
    assert D.rank_world() == (0, 1)


WORKER = textwrap.dedent('''
    import json, os, sys
    sys.path.insert(0, %r)
    import torch
    import torch.distributed as dist
    from mmdet_yolov4_amd import dist as D
    rank = int(os.environ['RANK'])
    dist.init_process_group('gloo', rank=rank, world_size=2)
    size = 5                                       # odd: rank 1's last image is the sampler's padding (image 0 again)
    mine = D.sampler_indices(size, rank, 2)
    rows_of = lambda image: (image * 2 + 1) %% 3   # 1, 0, 2, 1, 0 rows: the padding image has a row, others none
    dets, labels, pos = [], [], []
    for j, image in enumerate(mine):
        for k in range(rows_of(image)):
            dets.append([image, k, rank, j, 0.5])
            labels.append(k)
            pos.append(j * 2 + rank)
    dets = torch.tensor(dets, dtype=torch.float32).view(-1, 5)
    out = D.collect_flat(dets, torch.tensor(labels, dtype=torch.int64), torch.tensor(pos, dtype=torch.int64), size)
    res = dict(rank=rank, none=out is None, world=list(D.rank_world()))
    if out is not None:
        res.update(dets=out[0].tolist(), labels=out[1].tolist(), pos=out[2].tolist(), dtypes=[str(t.dtype) for t in out])
    print('RESULT ' + json.dumps(res), flush=True)
    dist.destroy_process_group()
''')


def test_collect_flat_two_ranks_gloo_cpu(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % ROOT)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdin=subprocess.DEVNULL,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=120)
        assert p.returncode == 0, out
        outs.append(json.loads([ln for ln in out.splitlines() if ln.startswith('RESULT ')][0][7:]))
    outs.sort(key=lambda o: o['rank'])
    assert outs[1]['none'] is True and outs[0]['none'] is False and outs[1]['world'] == [1, 2]
    r0 = outs[0]
    # images 0..4 with 1, 0, 2, 1, 0 rows; image 0's second visit (rank 1, position 5) has a row too, and it is dropped
    assert r0['pos'] == [0, 2, 2, 3] and r0['labels'] == [0, 0, 1, 0]
    assert [d[0] for d in r0['dets']] == [0, 2, 2, 3] and [d[2] for d in r0['dets']] == [0, 0, 0, 1]
    assert r0['dtypes'] == ['torch.float32', 'torch.int64', 'torch.int64']


def test_collect_flat_two_ranks_padding_rows_are_dropped():
    """The padding image with rows: what rank 0 does after the gather, on the gathered parts themselves."""
    size, world = 3, 2
    parts = []
    for rank in range(world):
        mine = D.sampler_indices(size, rank, world)        # rank 0: 0, 2; rank 1: 1, 0 (padding)
        pos = torch.tensor([j * world + rank for j, _ in enumerate(mine) for _ in range(2)])
        img = torch.tensor([im for im in mine for _ in range(2)], dtype=torch.float32)
        parts.append((img, pos))
    img = torch.cat([p[0] for p in parts])
    pos = torch.cat([p[1] for p in parts])
    d, l, i = D.collect_flat(img[:, None].repeat(1, 5), torch.zeros_like(pos), pos, size)
    assert i.tolist() == [0, 0, 1, 1, 2, 2] and d[:, 0].tolist() == [0., 0., 1., 1., 2., 2.]


def test_flat_loop_needs_the_gpu_and_says_so():
    model = FakeModel()                             # (its parameter lives on the CPU wherever the test runs)
    model.bbox_head = type('Head', (), dict(num_classes=2))()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.single_gpu_test(model, FakeLoader(FakeDataset([None])), flat=True)


def test_results_append_checks_its_arguments_without_a_gpu():
    """``yv4_results_append`` refuses bad arguments on the host, before any launch: the pointers below are never read."""
    import ctypes
    from mmdet_yolov4_amd import _lib
    L = _lib.lib()
    assert _lib.has('results_append') and _lib.RESULTS_MAX_PER_IMG == 4096
    keep = [(ctypes.c_int64 * 8)() for _ in range(7)]
    ptr = [ctypes.addressof(b) for b in keep]

    def call(N=1, M=4, C=3, base=0, capacity=8, hole=None):
        a = [None if i == hole else q for i, q in enumerate(ptr)]
        return L.yv4_results_append(*a[:4], N, M, C, base, capacity, *a[4:], None)
    assert call(N=-1) == -1 and b'negative batch' in L.yv4_last_error()
    assert call(M=_lib.RESULTS_MAX_PER_IMG + 1) == -2 and b'YV4_RESULTS_MAX_PER_IMG' in L.yv4_last_error()
    for hole in range(7):
        assert call(hole=hole) == -1 and b'null' in L.yv4_last_error()
    assert call(M=0) == -1 and call(C=0) == -1 and call(base=-1) == -1 and call(base=9) == -1
    assert L.yv4_results_append(None, None, None, None, 0, 4, 3, 0, 0, None, None, None, None) == 0    # an empty batch


def test_proposal_message_says_not_built_and_no_longer_blames_the_detectors():
    gt = pkg.CocoGt(dict(images=[dict(id=1)], categories=[dict(id=1, name='a')], annotations=[]))
    results = [[np.ones((1, 5), np.float32)]]
    for m in ('proposal', 'proposal_fast'):
        with pytest.raises(NotImplementedError) as e:
            pkg.evaluate_bbox(results, gt, metric=m)
        assert 'is not built' in str(e.value) and 'RPN' not in str(e.value) and "detector's own boxes" in str(e.value)
    ev = pkg.COCOeval(gt, results)
    ev.params.useCats = 0
    with pytest.raises(NotImplementedError) as e:
        ev.tables()
    assert 'useCats=0' in str(e.value) and 'is not built' in str(e.value) and 'RPN' not in str(e.value)


def test_coco_bbox_dataset_is_a_dataset_without_images():
    gt = dict(images=[dict(id=7), dict(id=3)], categories=[dict(id=5, name='a'), dict(id=2, name='b')], annotations=[])
    ds = pkg.CocoBBoxDataset(gt)
    assert len(ds) == 2 and ds.accepts_flat is True and ds.CLASSES == ('a', 'b') and ds.cat_ids == [5, 2]
    assert ds.img_ids == [7, 3]
    assert pkg.CocoBBoxDataset(pkg.CocoGt(gt), classes=['b']).cat_ids == [2]
    with pytest.raises(KeyError, match='metric mAP is not supported'):
        ds.evaluate([], metric='mAP')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert ds.evaluate([[np.zeros((0, 5), np.float32)] * 2] * 2, logger='silent') == {}
