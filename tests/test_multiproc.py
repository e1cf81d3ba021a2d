"""The N>1 launch path on CPU: 2 ranks, gloo backend, 127.0.0.1 rendezvous.

Covers what bench.py does around the timed region (join the group from the launcher's
environment, shard the work, barrier, MAX-reduce the elapsed time, rank 0 reports) and that the
ranks build identical weights while drawing different synthetic batches."""
import json
import os
import socket
import subprocess

import pytest
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = textwrap.dedent('''
    import json, os, sys, time
    sys.path.insert(0, %r)
    import torch
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import dist as D
    rank, local_rank, world = D.init(backend='gloo')
    torch.manual_seed(0)                                  # same recipe as bench.py
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[['conv', 'bottleneck', 'csp', 'sppv4'], [None, 1, 1, 1], [4, 8, 16, 16]],
                      out_indices=[1, 2, 3]),
        neck=dict(type='YOLOV4Neck', in_channels=[8, 16, 16], out_channels=[8, 16, 32], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=3, in_channels=[8, 16, 32], featmap_strides=[4, 8, 16],
                       anchor_generator=dict(type='YOLOV4AnchorGenerator', strides=[4, 8, 16],
                                             base_sizes=[[(4, 4)] * 3, [(8, 8)] * 3, [(16, 16)] * 3])),
        test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=10)))
    wsum = float(sum(p.double().sum() for p in det.parameters()))
    g = torch.Generator().manual_seed(1000 + rank)
    batch = torch.randint(0, 256, (2, 3, 8, 8), generator=g)
    lo, hi = D.shard(11, rank, world)
    D.barrier(sync_device=False)
    elapsed = 0.25 * (rank + 1)                           # pretend rank r took 0.25*(r+1) s
    worst = D.max_over_ranks(elapsed)
    D.barrier(sync_device=False)
    out = dict(rank=rank, world=world, wsum=wsum, bsum=int(batch.sum()), lo=lo, hi=hi, worst=worst)
    print('RESULT ' + json.dumps(out), flush=True)
    D.finalize()
''')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_gloo(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % ROOT)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out
        outs.append(json.loads([l for l in out.splitlines() if l.startswith('RESULT ')][0][7:]))
    outs.sort(key=lambda o: o['rank'])
    assert [o['world'] for o in outs] == [2, 2]
    assert outs[0]['wsum'] == outs[1]['wsum']             # replicated weights
    assert outs[0]['bsum'] != outs[1]['bsum']             # different shards of synthetic data
    assert (outs[0]['lo'], outs[0]['hi'], outs[1]['lo'], outs[1]['hi']) == (0, 6, 6, 11)
    assert outs[0]['worst'] == outs[1]['worst'] == 0.5    # max over ranks, seen by every rank


def test_shard_covers_everything():
    from mmdet_yolov4_amd import dist as D
    for n in (0, 1, 7, 32, 33):
        for world in (1, 2, 3, 8):
            spans = [D.shard(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


# ---- training exchange step: GradReducer over the flat gradient arena, 2 ranks ------------------
REDUCE_WORKER = textwrap.dedent('''
    import json, os, sys
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, 'tests', 'golden'))
    import torch
    from toy_model import Toy
    from mmdet_yolov4_amd import dist as D
    from mmdet_yolov4_amd.flat_state import FlatState
    rank, local_rank, world = D.init(backend='gloo')
    torch.manual_seed(0)
    class Odd(Toy):
        """Toy + a tail whose parameter counts (91, 7, 33, 3) are multiples of neither 4 nor 8: bucket sizes that
        the chunked exchange has to pad (dist.py _staging) and bucket tails that do not divide by the world size."""
        def __init__(self):
            super().__init__()
            self.fc1 = torch.nn.Linear(13, 7)
            self.fc2 = torch.nn.Linear(11, 3)
        def forward(self, x):
            y = super().forward(x)
            f = y.flatten(1)
            return y.mean() + self.fc1(f[:, :13]).square().mean() + self.fc2(f[:, 13:24]).square().mean()
    model = Odd() if os.environ.get('YV4_TEST_ODD') else Toy()   # identical weights on every rank
    fs = FlatState(model)
    red = D.GradReducer(fs, bucket_mb=float(os.environ.get('YV4_TEST_BUCKET_FLOATS', '200')) * 4 / (1 << 20),
                        mode=os.environ['YV4_TEST_MODE'])
    g = torch.Generator().manual_seed(100)
    xs = [torch.randn(2, 4, 6, 6, generator=g) for _ in range(2 * world)]   # world ranks x 2 micro-batches
    mine = xs[2 * rank: 2 * rank + 2]
    # accumulation window of 2 micro-batches: only the last one is exchanged
    fs.zero_grad()
    model(mine[0]).square().mean().backward()
    red.arm()
    model(mine[1]).square().mean().backward()
    launched_in_backward = all(red._launched)
    red.finish()
    # what the exchange must produce: mean over ranks of the per-rank SUM of micro-batch gradients
    ref = type(model)(); ref.load_state_dict({k: v for k, v in model.state_dict().items()})
    for r in range(world):
        for x in xs[2 * r: 2 * r + 2]:
            (ref(x).square().mean() / world).backward()
    err = max(float((p.grad - q.grad).abs().max()) for p, q in zip(model.parameters(), ref.parameters()))
    scale = max(float(q.grad.abs().max()) for q in ref.parameters())
    # a 16-bit wire format rounds every rank's LOCAL gradient sum: its error is relative to the largest local entry over
    # the ranks (per-rank gradients can cancel in the mean), cf. tests/test_gpu_ddp.py
    loc = type(model)(); loc.load_state_dict({k: v for k, v in ref.state_dict().items()})
    for x in mine:
        loc(x).square().mean().backward()
    lmax = torch.tensor(max(float(q.grad.abs().max()) for q in loc.parameters()))
    torch.distributed.all_reduce(lmax, op=torch.distributed.ReduceOp.MAX)
    scale = max(scale, float(lmax))
    out = dict(rank=rank, nb=len(red.buckets), launched=launched_in_backward, err=err, scale=scale,
               order=red.launch_order, gsum=float(fs.grads.double().sum()),
               sizes=[b[1] - b[0] for b in red.buckets], chunks=[st['chunk'] for st in red._stage.values()])
    print('RESULT ' + json.dumps(out), flush=True)
    D.finalize()
''')


def _run_reduce(tmp_path, mode, world, **extra):
    script = tmp_path / 'reduce_worker.py'
    script.write_text(REDUCE_WORKER % (ROOT, ROOT))
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1', YV4_TEST_MODE=mode, **extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=480)
        assert p.returncode == 0, out
        outs.append(json.loads([l for l in out.splitlines() if l.startswith('RESULT ')][0][7:]))
    outs.sort(key=lambda o: o['rank'])
    return outs


def _check_reduce(outs, mode):
    assert outs[0]['nb'] >= 2 and all(o['launched'] for o in outs)
    tol = 2.0 ** -8 * outs[0]['scale'] if mode == 'direct_bf16' else 1e-6
    assert all(o['err'] <= tol for o in outs), outs      # averaged sum of all ranks' gradients
    assert all(o['order'] == outs[0]['order'] for o in outs) and outs[0]['order'] == sorted(outs[0]['order'], reverse=True)
    assert all(o['gsum'] == outs[0]['gsum'] for o in outs)   # bit-identical arenas after the exchange


@pytest.mark.parametrize('mode', ['allreduce', 'direct', 'direct_bf16'])
def test_grad_reducer_two_ranks_gloo(tmp_path, mode):
    """The exchanged arena equals the mean over ranks of the per-rank gradient sums: exactly (1e-6) for the fp32 wire
    formats, within two bf16 roundings (2^-8 of the largest gradient) for 'direct_bf16'; both ranks end bit-identical and
    enqueue their collectives in the same (descending bucket) order."""
    _check_reduce(_run_reduce(tmp_path, mode, 2), mode)


@pytest.mark.parametrize('mode', ['allreduce', 'direct', 'direct_bf16'])
def test_grad_reducer_eight_ranks_gloo_ragged_buckets(tmp_path, mode):
    """The node's world size (8, mmdet/apis/train.py:74-82 + tools/dist_train.sh:8-10) over gloo on the CPU with an arena
    whose buckets are multiples of neither 8 floats nor the world size: every bucket's per-rank chunk is padded
    (dist.py _staging: ceil(n / 8) rounded up to 8 elements) and the pad must neither leak into the gradients nor
    desynchronise the ranks."""
    outs = _run_reduce(tmp_path, mode, 8, YV4_TEST_ODD='1', YV4_TEST_BUCKET_FLOATS='80')
    assert len(outs) == 8
    sizes = outs[0]['sizes']
    assert len(sizes) >= 3 and any(n % 8 for n in sizes), sizes
    if mode != 'allreduce':
        for n, c in zip(sorted(sizes), sorted(outs[0]['chunks'])):
            assert c % 8 == 0 and 8 * c >= n
        assert any(8 * c != n for n, c in zip(sorted(sizes), sorted(outs[0]['chunks'])))       # a padded tail was exchanged
    _check_reduce(outs, mode)


# ---- result gather of a distributed test run: ragged per-image results, 2 ranks -------------------
GATHER_WORKER = textwrap.dedent('''
    import json, os, sys
    sys.path.insert(0, %r)
    import numpy as np
    import torch
    from mmdet_yolov4_amd import dist as D
    rank, local_rank, world = D.init(backend='gloo')
    size = 7                                               # odd: the sampler pads rank 1 with image 0
    def result_of(i):                                      # per-image result: one (k_c, 5) array per class, ragged
        return [np.full((i + c, 5), 10 * i + c, dtype=np.float32) for c in range(3)]
    mine = D.sampler_indices(size, rank, world)
    merged = D.collect_results([result_of(i) for i in mine], size)
    ok = None
    if rank == 0:
        ok = len(merged) == size and all(
            len(m) == 3 and all(a.shape == b.shape and (a == b).all() for a, b in zip(m, result_of(i)))
            for i, m in enumerate(merged))
    empty = D.collect_results([], 0)
    print('RESULT ' + json.dumps(dict(rank=rank, mine=mine, ok=ok, none=merged is None, empty=empty)), flush=True)
    D.finalize()
''')


def test_collect_results_two_ranks_gloo(tmp_path):
    script = tmp_path / 'gather_worker.py'
    script.write_text(GATHER_WORKER % ROOT)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out
        outs.append(json.loads([l for l in out.splitlines() if l.startswith('RESULT ')][0][7:]))
    outs.sort(key=lambda o: o['rank'])
    assert outs[0]['mine'] == [0, 2, 4, 6] and outs[1]['mine'] == [1, 3, 5, 0]
    assert outs[0]['ok'] is True and outs[0]['none'] is False
    assert outs[1]['none'] is True                         # only rank 0 holds the merged list
    assert outs[0]['empty'] == [] and outs[1]['empty'] is None


def test_sampler_indices_match_torch_sampler():
    from torch.utils.data import DistributedSampler
    from mmdet_yolov4_amd import dist as D
    for n in (1, 2, 7, 16, 33):
        for world in (1, 2, 3, 8):
            for rank in range(world):
                ref = list(DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=False))
                assert D.sampler_indices(n, rank, world) == ref, (n, world, rank)
    assert D.sampler_indices(0, 0, 2) == []


def test_collect_results_single_process():
    from mmdet_yolov4_amd import dist as D
    assert D.collect_results([1, 2, 3], 2) == [1, 2]


# ---- bench.py's train-step leg: host logic around the child process (no GPU, the child is a stand-in) ----
def _leg_args(**kw):
    import argparse
    d = dict(train_batch=64, size=608, steps=3, warmup=1, train_dtype='bf16', model='yolov4l', train_timeout=5.0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_train_leg_child_gets_its_own_port_and_rank0_reports(monkeypatch):
    import subprocess
    import bench
    seen = {}

    def fake_run(cmd, env, **kw):
        seen['cmd'], seen['env'] = cmd, env
        line = json.dumps(dict(metric='images/sec (train step) yolov4l', value=123.4, n_gpus=2, ms_per_step=1.0))
        return subprocess.CompletedProcess(cmd, 0, stdout='noise\n' + line + '\n', stderr='')
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setenv('MASTER_PORT', '29500')
    out = bench.train_step_leg(_leg_args(), rank=0, local_rank=0, world=2)
    assert seen['env']['MASTER_PORT'] == '29507' and seen['env']['WORLD_SIZE'] == '2' and seen['env']['RANK'] == '0'
    assert seen['cmd'][1].endswith(os.path.join('tools', 'train_bench.py'))
    assert seen['cmd'][seen['cmd'].index('--batch') + 1] == '64' and seen['cmd'][seen['cmd'].index('--dtype') + 1] == 'bf16'
    assert out['value'] == 123.4 and out['steps'] == 3 and out['config']['global_batch'] == 128
    assert 'dp2' in out['config']['parallelism']
    # the other ranks run the child but report nothing
    assert bench.train_step_leg(_leg_args(), rank=1, local_rank=1, world=2) is None
    assert seen['env']['RANK'] == '1' and seen['env']['LOCAL_RANK'] == '1'


def test_train_leg_failure_costs_only_the_train_object(monkeypatch):
    import subprocess
    import bench

    def fails(cmd, env, **kw):
        return subprocess.CompletedProcess(cmd, 3, stdout='', stderr='RuntimeError: boom')
    monkeypatch.setattr(subprocess, 'run', fails)
    out = bench.train_step_leg(_leg_args(), 0, 0, 1)
    assert 'exit 3' in out['error'] and 'boom' in out['error']

    def hangs(cmd, env, timeout, **kw):
        raise subprocess.TimeoutExpired(cmd, timeout)
    monkeypatch.setattr(subprocess, 'run', hangs)
    assert 'killed' in bench.train_step_leg(_leg_args(), 0, 0, 1)['error']


LAUNCHED = textwrap.dedent('''
    import json, os, sys
    sys.path.insert(0, %r)
    import torch
    from mmdet_yolov4_amd import dist as D
    assert '--gpus' in sys.argv and sys.argv[sys.argv.index('--gpus') + 1] == os.environ['WORLD_SIZE']
    rank, local_rank, world = D.init(backend='gloo')          # the rendezvous the launcher's environment describes
    if '--die' in sys.argv and rank == 1:
        sys.exit(7)
    if '--hang' in sys.argv and rank == 0:
        import time
        time.sleep(600)                                       # a rank the launcher has to take down itself
    worst = D.max_over_ranks(0.5 * (rank + 1))
    D.barrier(sync_device=False)
    print('noise from rank %%d' %% rank, flush=True)
    if rank == 0:
        print(json.dumps(dict(metric='images/sec', n_gpus=world, worst=worst, local_rank=local_rank)), flush=True)
    D.finalize()
''')


def test_bench_launches_its_own_ranks(tmp_path, capfd):
    """`python bench.py --gpus N` with no launcher: the parent starts N children with the torch.distributed.run
    environment (tools/dist_train.sh:8-10), only rank 0's output is relayed, the worst exit code is returned."""
    import bench
    script = tmp_path / 'ranks.py'
    script.write_text(LAUNCHED % ROOT)
    rc = bench.launch_ranks(3, ['--gpus', '3', '--steps', '2'], script=str(script), timeout=120)
    out = capfd.readouterr().out
    assert rc == 0
    lines = [l for l in out.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and 'noise from rank 1' not in out and 'noise from rank 0' in out
    rec = json.loads(lines[0])
    assert rec == dict(metric='images/sec', n_gpus=3, worst=1.5, local_rank=0)


def test_bench_launcher_reports_the_worst_rank(tmp_path, capfd):
    import bench
    script = tmp_path / 'ranks.py'
    script.write_text(LAUNCHED % ROOT)
    rc = bench.launch_ranks(2, ['--gpus', '2', '--die'], script=str(script), timeout=60)
    assert rc == 7
    assert 'rank exit codes' in capfd.readouterr().err


def test_bench_launcher_kill_does_not_mask_the_failing_rank(tmp_path, capfd, monkeypatch):
    """rank 1 exits 7 by itself, rank 0 hangs and is killed by the launcher after the grace period (-9):
    the run's exit code is the rank's own 7, not 9; with only launcher kills (a timeout) it is 124."""
    import bench
    import time as _time
    script = tmp_path / 'ranks.py'
    script.write_text(LAUNCHED % ROOT)
    real = _time.time
    t0 = real()
    monkeypatch.setattr(bench.time, 'time', lambda: t0 + (real() - t0) * 20)      # the 30 s grace period in 1.5 s
    rc = bench.launch_ranks(2, ['--gpus', '2', '--die', '--hang'], script=str(script), timeout=2000)
    err = capfd.readouterr().err
    assert rc == 7, (rc, err)
    assert 'killed by the launcher: [0]' in err
    rc = bench.launch_ranks(2, ['--gpus', '2', '--hang'], script=str(script), timeout=300)   # 15 s of real time
    assert rc == 124


def test_bench_dump_outputs_writes_the_valid_detections(tmp_path):
    """--dump-outputs: float32 arrays of what the timed path hands its caller; rows past an image's count are masked."""
    import torch
    import numpy as np
    import bench
    dets = torch.arange(2 * 4 * 5, dtype=torch.float32).view(2, 4, 5)
    labels = torch.tensor([[3, 7, 9, 9], [1, 9, 9, 9]], dtype=torch.int32)
    count = torch.tensor([2, 1], dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / 'out'), dets, labels, count)
    d, l, c = (np.load(tmp_path / 'out' / f'{n}.npy') for n in ('dets', 'labels', 'count'))
    assert d.dtype == l.dtype == c.dtype == np.float32 and d.shape == (2, 4, 5) and l.shape == (2, 4)
    assert np.array_equal(c, [2, 1])
    assert np.array_equal(d[0, :2], dets[0, :2].numpy()) and np.array_equal(d[1, :1], dets[1, :1].numpy())
    assert not d[0, 2:].any() and not d[1, 1:].any()
    assert np.array_equal(l, [[3, 7, -1, -1], [1, -1, -1, -1]])
    bench.dump_outputs(str(tmp_path / 'out'), dets, labels, count, '_rank1')
    assert (tmp_path / 'out' / 'dets_rank1.npy').exists()


def test_bench_main_self_launches_only_without_a_launcher(monkeypatch):
    import bench
    called = {}
    monkeypatch.setattr(bench, 'launch_ranks', lambda n, argv, **kw: called.update(n=n, argv=list(argv)) or 0)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and called == dict(n=4, argv=['--gpus', '4', '--steps', '3'])
    # under a launcher whose world disagrees with --gpus: a message, not an AssertionError, and no GPU touched
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert 'WORLD_SIZE=2' in str(e.value.code)
