#!/usr/bin/env python
"""Generate tests/golden/loss_variants.npz by running the REFERENCE's ``IoULoss`` (both modes), ``DIoULoss`` and
``CIoULoss`` (mmdet/models/losses/iou_loss.py), imported through _ref_import.py (which stubs ``mmcv.jit``).

Content: box pairs ``pred`` / ``target`` (n, 4) fp32; per kind ``<kind>/loss`` (n,) -- the class's fp32 output with
``reduction='none'`` and ``loss_weight=1`` -- and ``<kind>/grad`` (n, 4), autograd's gradient of ``loss.sum()`` with
respect to ``pred``; the same two in float64 (``loss64`` / ``grad64``: the reference classes on the float64 boxes), which
gives the fixture's own fp32-vs-float64 spread.  ``group`` (n,) names what a pair was built for: 0 random, 1 zero
overlap, 2 identical, 3 containment, 4 shared edge, 5 shared corner.  Identical boxes make CIoU's trade-off term
0 / 0: the nan the reference returns there is recorded as it is.

Run in the build container only; the GPU box never sees /root/reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402
from oracle import build_ref  # noqa: E402

KINDS = dict(iou_linear=('IoULoss', dict(linear=True)), iou_log=('IoULoss', dict(linear=False)),
             diou=('DIoULoss', {}), ciou=('CIoULoss', {}))


def _box(c, wh):
    return torch.cat([c - wh / 2, c + wh / 2], 1)


def pairs(gen):
    def rnd(n, lo=4.0, hi=200.0):
        c = torch.rand(n, 2, generator=gen) * 400.0
        wh = torch.exp(torch.rand(n, 2, generator=gen) * (np.log(hi) - np.log(lo)) + np.log(lo))
        return c, wh
    pred, target, group = [], [], []

    def add(p, t, g):
        pred.append(p)
        target.append(t)
        group.append(torch.full((p.shape[0],), g, dtype=torch.int32))

    c, wh = rnd(160)                                            # random: near one another, so most overlap
    c2 = c + (torch.rand(160, 2, generator=gen) - 0.5) * wh
    wh2 = wh * torch.exp((torch.rand(160, 2, generator=gen) - 0.5) * 1.2)
    add(_box(c, wh), _box(c2, wh2), 0)
    c, wh = rnd(48, hi=60.0)                                    # zero overlap: further apart than both extents
    off = (wh + 70.0) * torch.where(torch.rand(48, 2, generator=gen) < 0.5, -1.0, 1.0)
    off[::3, 0] = 0.0                                           # (a third separated along y only)
    add(_box(c, wh), _box(c + off, wh * 1.3), 1)
    c, wh = rnd(32)                                             # identical
    add(_box(c, wh), _box(c, wh).clone(), 2)
    c, wh = rnd(48)                                             # containment, both ways round
    inner = _box(c + (torch.rand(48, 2, generator=gen) - 0.5) * wh * 0.4, wh * 0.5)
    add(torch.cat([_box(c, wh)[:24], inner[24:]]), torch.cat([inner[:24], _box(c, wh)[24:]]), 3)
    a = torch.round(_box(*rnd(32)))                             # shared edge (integers: the tie is exact): pred right = target left
    a[:, 2:] = torch.max(a[:, 2:], a[:, :2] + 2)
    b = a.clone()
    b[:, 0], b[:, 2] = a[:, 2], a[:, 2] + (a[:, 2] - a[:, 0])
    b[16:, 0] = a[16:, 0]                                       # (half of them: same left edge and same top edge instead)
    b[16:, 2] = a[16:, 2] + 3
    add(a, b, 4)
    b = a.clone()                                               # shared corner: zero overlap with both ties
    b[:, :2], b[:, 2:] = a[:, 2:], a[:, 2:] + (a[:, 2:] - a[:, :2])
    add(a, b, 5)
    return torch.cat(pred).float(), torch.cat(target).float(), torch.cat(group)


def main():
    if not _ref_import.available():
        print('reference not present: nothing to do')
        return
    _ref_import.install_shim(build_ref.load_ext())
    mod = sys.modules['mmdet.models.losses.iou_loss']
    gen = torch.Generator().manual_seed(53)
    pred, target, group = pairs(gen)
    data = dict(pred=pred.numpy(), target=target.numpy(), group=group.numpy())
    for kind, (cls, kw) in KINDS.items():
        fn = getattr(mod, cls)(reduction='none', loss_weight=1.0, **kw)
        for dt, sfx in ((torch.float32, ''), (torch.float64, '64')):
            p = pred.to(dt).requires_grad_(True)
            loss = fn(p, target.to(dt))
            assert loss.dtype == dt and loss.shape == (pred.shape[0],)
            (grad,) = torch.autograd.grad(loss.sum(), p)
            data[f'{kind}/loss{sfx}'] = loss.detach().numpy()
            data[f'{kind}/grad{sfx}'] = grad.numpy()
        print(kind, 'nan', int(np.isnan(data[f'{kind}/loss']).sum()), 'max', float(np.nanmax(data[f'{kind}/loss'])))
    out = os.path.join(HERE, 'loss_variants.npz')
    np.savez_compressed(out, **data)
    print('loss variants', out, pred.shape[0], 'pairs', f'{os.path.getsize(out) / 1e3:.1f} kB')


if __name__ == '__main__':
    main()
