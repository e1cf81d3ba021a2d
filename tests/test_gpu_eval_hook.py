"""Validation in training, on the GPU: the flat test loops against the list loops (bit for bit, through the scoring),
``EvalHook`` / ``CheckpointHook`` in a ``Runner`` beside ``StateEMAHook``, and ``DistEvalHook`` with two ranks on one
card over gloo (the pattern of tests/test_gpu_dist_test.py).  Detectors, images and ground truth: tests/_eval_hook_data.py."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import hooks as H
from mmdet_yolov4_amd import yolocsp_head
from mmdet_yolov4_amd.coco_eval import flatten_results
from mmdet_yolov4_amd.optim import build_optimizer

import _eval_hook_data as DATA

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _setup(dev, kind='v4', batch=2, **cfg):
    det = (DATA.tiny_v3 if kind == 'v3' else DATA.tiny_v4)(DATA.make_test_cfg(v3=kind == 'v3', **cfg), dev)
    pipe = pkg.FusedTestPipeline(img_scale=(128, 128), device=dev)
    imgs = DATA.images()
    empty = DATA.lift_head(det, DATA.Loader(pipe, imgs, range(DATA.SIZE), batch=batch))
    return det, pipe, imgs, empty


def _spy_split(monkeypatch):
    calls = []
    real = yolocsp_head._run_split_path

    def spy(post, counts):
        calls.append(int((counts < 0).sum()))
        return real(post, counts)
    monkeypatch.setattr(yolocsp_head, '_run_split_path', spy)
    return calls


@pytest.mark.parametrize('kind,split_thr', [('v4', None), ('v4', 'some'), ('v3', None)])
def test_flat_loop_equals_the_list_loop_through_the_scoring(gpu_device, monkeypatch, kind, split_thr):
    cfg = {}
    if split_thr == 'some':
        # candidates per image are not known before the run: take the threshold from a first pass, between the two
        # largest candidate counts, so that some images take the split path and some do not
        det, pipe, imgs, _ = _setup(gpu_device, kind)
        cand = []
        for data in DATA.Loader(pipe, imgs, range(DATA.SIZE), batch=2):
            batch = data['img'][0]
            det.simple_test(batch, data['img_metas'][0], rescale=True)
            plan = det.compile(*[batch.shape[k] for k in (0, 2, 3)], device=gpu_device, rescale=True, graph=True)
            cand.extend(int(c) for c in plan.post['counts'][:batch.shape[0]].cpu())
        print('candidates per image', cand)
        top = sorted(set(cand))
        assert len(top) >= 3                                 # none, some, more: a threshold between the last two
        cfg['split_thr'] = (top[-2] + top[-1] + 1) // 2
    det, pipe, imgs, empty = _setup(gpu_device, kind, **cfg)
    calls = _spy_split(monkeypatch)
    loader = DATA.Loader(pipe, imgs, range(DATA.SIZE), batch=2)
    lists = pkg.single_gpu_test(det, loader)
    list_calls = list(calls)
    del calls[:]
    flat = pkg.single_gpu_test(det, loader, flat=True)
    per_image = [sum(len(c) for c in r) for r in lists]
    print(kind, split_thr, 'detections per image', per_image, 'split-path images per batch', list_calls)
    assert len(lists) == DATA.SIZE and per_image[empty] == 0 and sum(n > 0 for n in per_image) == DATA.SIZE - 1
    assert max(per_image) > DATA.NUM_CLASSES                 # enough rows for the class order to matter
    if split_thr == 'some':
        assert sum(list_calls) >= 1 and sum(list_calls) < sum(n > 0 for n in per_image)
    else:
        assert list_calls == []
    assert calls == list_calls                               # the flat loop takes the split path for the same images
    want = flatten_results(lists)
    assert all(t.is_cuda for t in flat)
    assert flat[0].dtype == torch.float32 and flat[1].dtype == torch.int64 and flat[2].dtype == torch.int64
    for got, ref in zip(flat, want):
        assert np.array_equal(got.cpu().numpy(), ref)
    assert len(np.unique(want[1])) > 1
    # the scoring: equal dicts, bit-equal tables
    gt = DATA.synthetic_gt(lists, imgs)
    ds = pkg.CocoBBoxDataset(gt, classes=[f'c{c}' for c in DATA.CAT_IDS])
    assert ds.cat_ids == DATA.CAT_IDS and ds.img_ids == DATA.IMG_IDS and len(ds) == DATA.SIZE
    a, b = ds.evaluate(lists, logger='silent'), ds.evaluate(flat, logger='silent')
    assert a == b and a['bbox_mAP'] > 0
    evs = []
    for res in (lists, flat):
        ev = pkg.COCOeval(gt, res, cat_ids=DATA.CAT_IDS, img_ids=DATA.IMG_IDS)
        ev.evaluate()
        ev.accumulate()
        evs.append(ev.eval)
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(np.asarray(evs[0][key]), np.asarray(evs[1][key])), key


class _Recording(pkg.CocoBBoxDataset):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.received = []

    def evaluate(self, results, **kw):
        self.received.append(tuple(t.clone() for t in results))
        return super().evaluate(results, **kw)


def test_hooks_evaluate_the_ema_weights_and_keep_the_best(gpu_device, tmp_path):
    det, pipe, imgs, _ = _setup(gpu_device)
    lists = pkg.single_gpu_test(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    ds = _Recording(DATA.synthetic_gt(lists, imgs), classes=[f'c{c}' for c in DATA.CAT_IDS])
    loader = DATA.Loader(pipe, imgs, range(DATA.SIZE), dataset=ds)
    rng = np.random.default_rng(5)
    data = dict(img=torch.from_numpy(rng.standard_normal((2, 3, 128, 128)).astype(np.float32)).to(gpu_device),
                img_metas=[dict(), dict()],
                gt_bboxes=[torch.tensor([[10., 12., 70., 90.], [40., 30., 100., 64.]], device=gpu_device),
                           torch.tensor([[5., 50., 60., 120.]], device=gpu_device)],
                gt_labels=[torch.tensor([0, 2], device=gpu_device), torch.tensor([1], device=gpu_device)])
    opt = build_optimizer(det, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005))
    runner = H.Runner(det, opt, max_epochs=2, work_dir=str(tmp_path))
    name = 'bbox_head.convs_pred.0.weight'
    ema_name = 'ema_' + name.replace('.', '_')
    param = dict(det.named_parameters())[name]
    seen = []

    class Probe(H.Hook):
        def before_train_epoch(self, r):
            if r.epoch > 0:                              # the EMA hook has swapped the trained weights back in
                seen[-1]['back'] = torch.equal(param.detach(), seen[-1]['trained'])

        def after_train_iter(self, r):                   # after the optimizer step and the EMA update
            self.trained = param.detach().clone()
            self.ema = getattr(det, ema_name).detach().clone()

        def after_train_epoch(self, r):                  # after the swap, the checkpoint and the evaluation
            was = det.training
            mine = pkg.single_gpu_test(det, loader, flat=True)
            det.train(was)
            seen.append(dict(trained=self.trained, ema=self.ema, now=param.detach().clone(), table=mine,
                             msgs=dict(r.meta['hook_msgs']), training=was))
    runner.register_hook(H.StateEMAHook(momentum=0.9, interval=1, warm_up=2), 'HIGH')
    runner.register_hook(H.Fp16GradAccumulateOptimizerHook(accumulation=1, loss_scale=512.), 'ABOVE_NORMAL')
    runner.register_hook(H.CheckpointHook(interval=1))
    runner.register_hook(H.EvalHook(loader, interval=1, save_best='bbox_mAP'))
    runner.register_hook(Probe(), 'LOW')
    det.train()
    runner.run(H.BatchSource([data] * 2, 2))
    assert len(seen) == 2 and len(ds.received) == 2
    for e, s in enumerate(seen):
        assert torch.equal(s['now'], s['ema'])                       # the weights in use are the EMA arena's ...
        assert not torch.equal(s['now'], s['trained'])               # ... not the trained ones
        assert s['training'] is True                                 # the hook left the model as it found it
        assert len(s['table'][0]) > 0
        for mine, theirs in zip(s['table'], ds.received[e]):         # the same table the dataset's evaluate received
            assert mine.is_cuda and torch.equal(mine, theirs)
        assert s['msgs']['last_ckpt'] == str(tmp_path / f'epoch_{e + 1}.pth')
    assert seen[0]['back'] is True                                   # epoch 2 trained on the trained weights
    out = runner.log_buffer.output
    assert runner.log_buffer.ready and 'bbox_mAP' in out and 'bbox_mAP_50' in out and 'bbox_mAP_copypaste' in out
    msgs = runner.meta['hook_msgs']
    assert os.path.isfile(msgs['best_ckpt']) and msgs['best_score'] == max(
        pkg.evaluate_bbox(r, ds.coco, cat_ids=ds.cat_ids, img_ids=ds.img_ids, logger='silent')['bbox_mAP']
        for r in ds.received)
    link = tmp_path / 'best_bbox_mAP.pth'
    assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(msgs['best_ckpt'])
    # the checkpoint was written after the swap: its weights are the EMA's, its ema_ entries the trained ones
    best_epoch = int(os.path.basename(msgs['best_ckpt'])[6:-4])
    sd = torch.load(msgs['best_ckpt'], weights_only=False)['state_dict']
    assert torch.equal(sd[name].to(gpu_device), seen[best_epoch - 1]['ema'])
    assert torch.equal(sd[ema_name].to(gpu_device), seen[best_epoch - 1]['trained'])
    # after the run: train mode; the last swap has no successor, so the trained weights of the last epoch are the
    # ema_ entries, as in the reference (ema_hooks.py:118-126) -- nothing of them is lost
    assert det.training
    assert torch.equal(getattr(det, ema_name), seen[-1]['trained'])


WORKER = textwrap.dedent('''
    import hashlib, json, os, sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import torch
    import torch.distributed as dist
    import mmdet_yolov4_amd as pkg
    from mmdet_yolov4_amd import dist as D
    from mmdet_yolov4_amd import hooks as H
    from mmdet_yolov4_amd.flat_state import FlatState
    import _eval_hook_data as DATA
    rank = int(os.environ['RANK'])
    dist.init_process_group('gloo', rank=rank, world_size=2)
    dev = torch.device('cuda', 0)
    det = DATA.tiny_v4(DATA.make_test_cfg(), dev)
    pipe = pkg.FusedTestPipeline(img_scale=(128, 128), device=dev)
    imgs = DATA.images()
    DATA.lift_head(det, DATA.Loader(pipe, imgs, range(DATA.SIZE), batch=1))
    # samples_per_gpu = 1, as in tests/test_gpu_dist_test.py: an image's canvas is then its own in both runs (in a batch
    # it is the batch's largest, and what the padding holds after the first layer reaches into the image)
    whole = pkg.single_gpu_test(det, DATA.Loader(pipe, imgs, range(DATA.SIZE), batch=1), flat=True)
    whole = [t.clone() for t in whole]

    class Recording(pkg.CocoBBoxDataset):
        received = None
        def evaluate(self, results, **kw):
            self.received = results
            return super().evaluate(results, **kw)
    lists = pkg.single_gpu_test(det, DATA.Loader(pipe, imgs, range(DATA.SIZE)))
    ds = Recording(DATA.synthetic_gt(lists, imgs), classes=['c%%d' %% c for c in DATA.CAT_IDS])
    flat = FlatState.of(det)
    runs = H.bn_stat_runs(det, flat)

    def digest():
        return hashlib.sha1(b''.join(flat.values[lo:hi].cpu().numpy().tobytes() for lo, hi in runs)).hexdigest()
    before = digest()
    ints_before = flat.ints.clone()
    if rank == 1:                          # this rank's running statistics drift, its parameters do not
        with torch.no_grad():
            for m in det.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.running_mean.add_(0.37)
                    m.running_var.mul_(1.9)
        flat.bump_versions()
        assert digest() != before
    params_before = flat.values[:flat.n_param].clone()
    hook = H.DistEvalHook(DATA.Loader(pipe, imgs, D.sampler_indices(DATA.SIZE, rank, 2), batch=1, dataset=ds), interval=1)
    runner = H.Runner(det, None, max_epochs=1)
    sent = []
    real = dist.broadcast
    dist.broadcast = lambda t, src, *a, **k: (sent.append(int(t.numel())), real(t, src, *a, **k))[1]
    hook.after_train_epoch(runner)
    dist.broadcast = real
    out = dict(rank=rank, before=before, after=digest(), evaluated=ds.received is not None, broadcasts=len(sent),
               runs=len(runs), sent=sum(sent), span=sum(hi - lo for lo, hi in runs),
               params_same=bool(torch.equal(params_before, flat.values[:flat.n_param])),
               ints_same=bool(torch.equal(ints_before, flat.ints)), mAP=runner.log_buffer.output.get('bbox_mAP'))
    if rank == 0:
        out['rows'] = int(whole[0].shape[0])
        out['same'] = all(bool(torch.equal(a, b)) and a.is_cuda for a, b in zip(ds.received, whole))
    print('RESULT ' + json.dumps(out), flush=True)
    dist.destroy_process_group()
''')


def test_two_ranks_share_bn_statistics_and_rank0_scores_the_whole_table(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % (ROOT, HERE))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdin=subprocess.DEVNULL,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out
        outs.append(json.loads([ln for ln in out.splitlines() if ln.startswith('RESULT ')][0][7:]))
    outs.sort(key=lambda o: o['rank'])
    r0, r1 = outs
    assert r0['before'] == r1['before'] == r0['after'] == r1['after']       # rank 1's drift is gone
    assert r0['evaluated'] is True and r1['evaluated'] is False and r1['mAP'] is None and r0['mAP'] is not None
    assert r0['rows'] > 0 and r0['same'] is True
    for r in outs:
        # one collective per contiguous run of BatchNorm statistics -- this model's float buffers are nothing else, so
        # one -- carrying exactly those segments; parameters and integer buffers untouched
        assert r['broadcasts'] == r['runs'] == 1 and r['sent'] == r['span'] and r['params_same'] and r['ints_same']
