"""The convolution front end routes every layer where it did when tests/golden/conv_routes.npz was written: for each
descriptor of the sweep (every conv of every shipped model config at batch 1 / 2 / 32 / 64 and a Cin x Cout x map x
kernel x batch grid; tests/golden/make_golden_conv_routes.py) the tile the three pick functions resolve AUTO to, the
split-K workspace and ways of both element widths and the weight gradient's workspace for f32 / f16 / bf16 equal the
recorded ones, row by row.  Pure host functions: nothing is launched, no GPU is needed."""
import ctypes as C

import numpy as np

import mmdet_yolov4_amd as pkg

L = pkg._lib


def _routes(lib, fields, desc):
    out = np.zeros((len(desc), 10), np.int64)
    d = L.ConvDesc()
    ks = C.c_int(0)
    for i, row in enumerate(desc):
        for f, v in zip(fields, row):
            setattr(d, f, int(v))
        p = C.byref(d)
        v = [lib.yv4_conv_pick_tile(p), lib.yv4_conv_h16_pick_tile(p), lib.yv4_conv_f8_pick_tile(p)]
        for fn in (lib.yv4_conv_splitk_workspace, lib.yv4_conv_h16_splitk_workspace):
            ks.value = -7
            v += [fn(p, C.byref(ks)), ks.value]
        v += [lib.yv4_conv_wgrad_workspace(p, dt) for dt in (L.F32, L.F16, L.BF16)]
        out[i] = v
    return out


def test_routes_match_the_golden_table(golden):
    g = golden('conv_routes')
    fields, names, desc, want = [str(s) for s in g['desc_fields']], [str(s) for s in g['values']], g['desc'], g['routes']
    assert len(names) == want.shape[1] == 10 and len(desc) == len(want) > 6000 and int(g['n_model_rows']) > 2000
    got = _routes(L.lib(), fields, desc)
    bad = np.nonzero((got != want).any(axis=1))[0]
    lines = [f'{dict(zip(fields, desc[i].tolist()))}: ' +
             ', '.join(f'{n} {want[i, j]} -> {got[i, j]}' for j, n in enumerate(names) if got[i, j] != want[i, j])
             for i in bad[:20]]
    assert not len(bad), f'{len(bad)} of {len(desc)} descriptors moved:\n' + '\n'.join(lines)


def test_the_sweep_reaches_every_route(golden):
    """The table is worth its name only if the sweep exercises the rules: every fp32 and 16-bit kernel family, pinned
    shapes of the wide families, split and unsplit layers, and all weight-gradient chunkings appear in it."""
    g = golden('conv_routes')
    r = g['routes']
    f32, h16 = set(r[:, 0].tolist()), set(r[:, 1].tolist())
    w3_pinned, wide_pinned = ({fam + 16 * (i + 1) for i in range(5)} for fam in (10, 11))      # YV4_TILE_*_SHAPE(i)
    assert {5, 6, 7, 8, 9} <= f32 and f32 & w3_pinned and f32 & wide_pinned, f32
    assert {1, 2, 3, 4, 5, 6, 7, 8} <= h16, h16
    assert len(set(r[:, 2].tolist())) == 3
    for col in (4, 6):
        assert {1, 2, 4, 8} <= set(r[:, col].tolist())
    assert all((r[:, c] > 0).any() and (r[:, c] == 0).any() for c in (3, 5, 7, 8, 9))
