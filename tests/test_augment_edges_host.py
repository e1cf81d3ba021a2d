"""The constructed inputs of tests/_aug_edge_data.py against the references alone, without a GPU: each builder must reach
the branch or edge of csrc/augment.hip / csrc/augment_v3.hip it is aimed at, as seen by oracle/augment_oracle.py and
tests/_v3_aug_ref.py, so that none can quietly stop reaching it.  tests/test_gpu_augment_edges.py runs the kernels on the
same inputs and shares the reference chains defined here."""
import numpy as np
import pytest

from oracle import augment_oracle as A

import _aug_edge_data as D
import _v3_aug_ref as R

F32 = np.float32


# ---- reference chains shared with the GPU tests ---------------------------------------------------------------------------
def resized_tiles(sources, img_scale):
    return [A.resize_linear_u8(im, *A.rescale_size(*im.shape[:2], img_scale)) for im in sources]


def mosaic_canvas(sources, img_scale, pad_val=114):
    """The stitched canvas of four decoded sources (no boxes)."""
    return A.mosaic(resized_tiles(sources, img_scale), [np.zeros((0, 4), F32)] * 4, [np.zeros(0, np.int64)] * 4, pad_val)[0]


def mosaic_reference(four, prm, img_scale, pad_val=114):
    """One sample of the geometry cases -> (uint8 image after the geometric chain, float32 CHW image, boxes, labels)."""
    geo = A.geometric(mosaic_canvas([f[0] for f in four], img_scale, pad_val), prm, pad_val)
    img, boxes, labels, _ = A.train_sample([f[0] for f in four], [f[1] for f in four], [f[2] for f in four], prm,
                                           scale=img_scale, pad_val=pad_val)
    return geo, img, boxes, labels


def boxes_reference(four, prm, img_scale, min_area, min_visibility, min_size, max_aspect_ratio):
    """The oracle's box chain in order for one sample of ((h, w), boxes, labels) tiles: Resize's scale + clip, the mosaic
    shift, the Albu chain with its BboxParams filter, GtBBoxesFilter."""
    ims, bxs = [], []
    for (h, w), b, _ in four:
        nh, nw = A.rescale_size(h, w, img_scale)
        bb = b * np.array([nw / w, nh / h, nw / w, nh / h], dtype=F32)         # A.train_sample's Resize._resize_bboxes
        bb[:, 0::2] = np.clip(bb[:, 0::2], 0, nw)
        bb[:, 1::2] = np.clip(bb[:, 1::2], 0, nh)
        bxs.append(bb.astype(F32))
        ims.append(np.zeros((nh, nw, 3), np.uint8))
    canvas, boxes, labels, _ = A.mosaic(ims, bxs, [f[2] for f in four], 0)
    boxes, labels = A.geometric_boxes(boxes, labels, canvas.shape[:2], prm, min_area=min_area,
                                      min_visibility=min_visibility)
    return A.gt_bboxes_filter(boxes, labels, min_size=min_size, max_aspect_ratio=max_aspect_ratio)


def v3_distorted(src, p):
    """(3, h, w): what the resized region holds under identity geometry, mean 0, std 1, no channel swap."""
    return np.ascontiguousarray(R.distort(src, p).transpose(2, 0, 1))


def v3_branch_counts(src, p):
    """How many pixels of ``src`` take each branch of the photometric chain under parameters ``p``, by the restatement's
    own arithmetic (the steps of R.distort, stopped where each branch is decided)."""
    img = np.array(src, dtype=F32)
    if p['brightness'] is not None:
        img = img + F32(p['brightness'])
    c = dict(v_negative=int((img.max(-1) < 0).sum()))
    if p['contrast'] is not None and p['contrast_first']:
        img = img * F32(p['contrast'])
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    hsv = R.bgr2hsv(img)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    c['v_zero'] = int((v == 0).sum())
    c['tie_v_r_g'] = int(((v == r) & (v == g) & (v > b)).sum())
    c['tie_v_g_b'] = int(((v == g) & (v == b) & (v > r)).sum())
    if p['saturation'] is not None:
        s = s * F32(p['saturation'])
    c['s_zero'] = int((s == 0).sum())
    c['wrap_hi'] = c['wrap_lo'] = 0
    if p['hue'] is not None:
        h = h + F32(p['hue'])
        c['wrap_hi'] = int((h > 360).sum())
        h = np.where(h > 360, h - F32(360), h).astype(F32)
        c['wrap_lo'] = int((h < 0).sum())
        h = np.where(h < 0, h + F32(360), h).astype(F32)
    hh = (h * R.HSCALE).astype(F32)
    live = s != 0                                                   # the s == 0 shortcut never looks at the hue
    c['hh_ge_6'] = int(((hh >= 6) & live).sum())
    hh = np.where(hh >= 6, hh - F32(6), hh).astype(F32)
    assert ((hh >= 0) & (hh < 6)).all()
    sector = np.floor(hh).astype(np.int64)
    for k in range(6):
        c[f'sector{k}'] = int(((sector == k) & live).sum())
    out = R.distort(src, p)
    c['out_below_0'] = int((out < 0).sum())
    c['out_above_255'] = int((out > 255).sum())
    return c


V3_BRANCHES = ('v_negative', 'v_zero', 's_zero', 'wrap_hi', 'wrap_lo', 'hh_ge_6', 'tie_v_r_g', 'tie_v_g_b', 'out_below_0',
               'out_above_255') + tuple(f'sector{k}' for k in range(6))


# ---- 1. colour jitter of the mosaic kernel ---------------------------------------------------------------------------------
def test_cube_quarters_present_every_colour_once_and_every_hue_and_saturation():
    seen = np.zeros(1 << 24, np.int64)
    hues, sats = set(), set()
    for q in range(4):
        tiles = D.cube_quarter_tiles(q)
        assert all(t.shape == (1024, 1024, 3) and t.dtype == np.uint8 for t in tiles)
        canvas = D.stitch4(tiles)
        codes = D.colour_codes(canvas)
        assert codes.min() >> 16 == 64 * q and codes.max() >> 16 == 64 * q + 63
        seen += np.bincount(codes, minlength=1 << 24)
        hsv = A.bgr2hsv_u8(canvas)
        hues |= set(np.unique(hsv[..., 0]).tolist())
        sats |= set(np.unique(hsv[..., 1]).tolist())
    assert (seen == 1).all(), 'the four quarters must be a permutation of arange(2**24)'
    assert hues == set(range(180)) and sats == set(range(256))


def test_stitch4_is_the_oracle_mosaic_of_equal_tiles():
    tiles = D.grid_tiles()
    np.testing.assert_array_equal(D.stitch4(tiles), mosaic_canvas(tiles, (D.GRID_TILE, D.GRID_TILE)))
    codes = D.colour_codes(D.stitch4(tiles))
    assert len(np.unique(codes)) == 28 ** 3 == 21952 and len(D.GRID_LEVELS) == 28


def test_gain_corners_clip_and_wrap_the_luts():
    hsv = A.bgr2hsv_u8(D.grid_colours()[None])
    h, s, v = (np.unique(hsv[..., k]).astype(np.float64) for k in range(3))
    corners = D.gain_corners()
    assert len(set(corners)) == 8 and D.CUBE_GAINS == max(corners)
    hit = dict(sat_clipped=0, sat_free=0, val_clipped=0, val_free=0, hue_wrapped=0)
    for gains in corners:
        lh, ls, lv = A.hsv_luts(np.asarray(gains, np.float64))
        hit['sat_clipped'] += int(((s * gains[1] > 255) & (ls[s.astype(int)] == 255)).sum())
        hit['sat_free'] += int((ls[s.astype(int)] < 255).sum())
        hit['val_clipped'] += int(((v * gains[2] > 255) & (lv[v.astype(int)] == 255)).sum())
        hit['val_free'] += int((lv[v.astype(int)] < 255).sum())
        hit['hue_wrapped'] += int(((h * gains[0] >= 180) & (lh[h.astype(int)] < h)).sum())
    assert all(hit.values()), hit
    lh, ls, lv = A.hsv_luts(np.asarray(D.CUBE_GAINS, np.float64))              # the cube's gains clip and wrap too
    assert (ls == 255).sum() > 1 and (lv == 255).sum() > 1 and lh[178] == 0


# ---- 2. geometry of the mosaic kernel --------------------------------------------------------------------------------------
def _origins(case):
    out = []
    for four, prm in zip(case['samples'], case['params']):
        side = mosaic_canvas([f[0] for f in four], case['img_scale']).shape[0]
        top, left, H, W = A.pad_if_needed_offsets(side, side, prm['pad_to'], prm['pad_to'])
        y1, x1 = A.random_crop_origin(H, W, prm['crop'], prm['crop'], prm['h_start'], prm['w_start'])
        out.append((top, H, y1, x1))
    return out


def test_geometry_case_a_reaches_every_row_of_its_table():
    O, C = D.GEO['out'], D.GEO['crop']
    assert O % 4 and O % 64 and D.CASE_A_CALLS == 4
    seen, last_y, last_x, kinds, pitched = set(), 0, 0, set(), set()
    for call in range(D.CASE_A_CALLS):
        case = D.geometry_case_a(call)
        assert len(case['samples']) == len(case['params']) == 3                 # images follow the first one
        pitched.add(case['pitched'])
        for four, prm, (top, H, y1, x1) in zip(case['samples'], case['params'], _origins(case)):
            S = int(C * prm['scale'])
            seen.add((S, (S - O) // 2, prm['flip']))
            assert top > 0 and H == D.GEO['pad_to']
            last_y += y1 == H - C
            last_x += x1 == H - C
            for i, f in enumerate(four):
                h, w = f[0].shape[:2]
                nh, nw = A.rescale_size(h, w, case['img_scale'])
                kinds.add((i, 'enlarged' if nh > h else 'shrunk' if nh < h else 'copied'))
        assert sum(len(f[1]) for four in case['samples'] for f in four) > 0
    assert seen == {(S, o, flip) for (S, o) in ((67, 0), (100, 16), (134, 33), (201, 67)) for flip in (False, True)}
    assert last_y and last_x, 'the last crop origin H - C must be reached on both axes'
    starts = {(p['h_start'], p['w_start']) for c in range(4) for p in D.geometry_case_a(c)['params']}
    assert len(starts) == 9
    assert kinds == {(i, k) for i in range(4) for k in ('enlarged', 'shrunk', 'copied')}     # every kind in every quadrant
    assert pitched == {0, 1, 2, 3}


def test_geometry_case_b_pads_nothing():
    case = D.geometry_case_b()
    (top, H, y1, x1), = _origins(case)
    assert top == 0 and H == 240 >= D.GEO['pad_to']
    assert y1 == H - D.GEO['crop']                                              # and the crop sits at its last row
    geo, _, boxes, _ = mosaic_reference(case['samples'][0], case['params'][0], case['img_scale'])
    assert len(np.unique(geo)) > 100


def test_geometry_case_c_sees_padding_only():
    case = D.geometry_case_c()
    four, prm = case['samples'][0], case['params'][0]
    assert all(max(f[0].shape[:2]) <= 16 for f in four) and prm['h_start'] == prm['w_start'] == 0.0
    assert len(np.unique(mosaic_canvas([f[0] for f in four], case['img_scale']))) > 100
    geo, img, boxes, labels = mosaic_reference(four, prm, case['img_scale'])
    assert geo.shape == (67, 67, 3) and (geo == 114).all()
    assert len(np.unique(img)) == 1 and len(boxes) == 0
    jittered = A.hsv_jitter(geo, prm['hsv'])
    assert (jittered == jittered[0, 0, 0]).all() and jittered[0, 0, 0] != 114          # the s == 0 shortcut through the LUT


# ---- 3. aug_boxes_kernel -----------------------------------------------------------------------------------------------------
def test_crowded_boxes_pass_one_pass_and_keep_about_half():
    data = D.crowded_boxes()
    counts = [sum(len(f[1]) for f in four) for four in data['samples']]
    assert counts == [64, 65, 0, 180]
    labels = np.concatenate([f[2] for four in data['samples'] for f in four])
    assert len(np.unique(labels)) == len(labels) == sum(counts)
    assert any(p['flip'] for p in data['params']) and any(p['scale'] != 1.0 for p in data['params'])
    last_lane = set()
    for n, (four, prm, k) in enumerate(zip(data['samples'], data['params'], counts)):
        b, l = boxes_reference(four, prm, D.BOX_GEO['img_scale'], **D.BOX_THRESHOLDS)
        assert len(b) == len(l)
        if k:
            assert k / 3 <= len(l) <= 2 * k / 3, (k, len(l))
            order = np.concatenate([f[2] for f in four])
            at = np.searchsorted(order, l)
            assert (np.diff(at) > 0).all()                                      # survivors keep their order
            assert all((at // 64 == q).any() for q in range(-(-k // 64)))       # some in every pass
            last_lane |= {(n, int(i)) for i in at if i % 64 == 63}
        else:
            assert len(l) == 0
    assert last_lane == {(n, i) for n, i in D.BOX_PLANTED if i % 64 == 63}      # lane 63 of every full pass survives


def test_threshold_boxes_sit_on_and_next_to_each_strict_threshold():
    data = D.threshold_boxes()
    four, prm = data['samples'][0], data['params'][0]
    for i, (_, b, _) in enumerate(four):                                        # the float32 tile shift rounds nothing
        shift = np.tile(A.mosaic_origin(i, 64, 64, 64), 2).astype(np.float64)
        np.testing.assert_array_equal((b + shift.astype(F32)).astype(np.float64), b.astype(np.float64) + shift)
    boxes, labels = boxes_reference(four, prm, D.THR_GEO['img_scale'], **D.THR_THRESHOLDS)
    kept = set(labels.tolist())
    for name, (on, past) in data['pairs'].items():
        assert on not in kept and past in kept, name
    assert not kept & set(data['rejected'])
    assert kept == {past for _, past in data['pairs'].values()}
    # each box on a threshold fails that threshold alone: relaxing it by one part in 2^20 keeps the box
    eps = 2.0 ** -20
    relaxed = dict(min_size_w=dict(min_size=2 - eps), min_size_h=dict(min_size=2 - eps), min_area=dict(min_area=16 - eps),
                   min_area_clipped=dict(min_area=16 - eps), max_aspect_ratio=dict(max_aspect_ratio=20 + 16 * eps),
                   min_visibility=dict(min_visibility=0.25 - eps))
    for name, over in relaxed.items():
        _, l = boxes_reference(four, prm, D.THR_GEO['img_scale'], **dict(D.THR_THRESHOLDS, **over))
        assert data['pairs'][name][0] in l.tolist(), name
    # the boxes come through unmoved: identity geometry
    at = {int(l): b for b, l in zip(boxes, labels)}
    np.testing.assert_array_equal(at[1], four[0][1][1])
    np.testing.assert_array_equal(at[10], np.array([88 - 2.0 ** -17, 30, 96, 46], F32))


# ---- 4. photometric chain of the v3 kernel ---------------------------------------------------------------------------------
def test_v3_photometric_table_takes_every_branch():
    src = D.v3_grid_source()
    assert src.shape == (28, 784, 3) and len(np.unique(D.colour_codes(src))) == 28 ** 3
    total = dict.fromkeys(V3_BRANCHES, 0)
    sets = [p for hue in D.V3_HUES for p in D.v3_photometric_table(hue)]
    assert len(sets) == 180 and len({tuple(sorted((k, str(v)) for k, v in p.items())) for p in sets}) == 180
    for p in sets:
        for k, v in v3_branch_counts(src, p).items():
            total[k] += v
    missing = [k for k in V3_BRANCHES if not total[k] and k != 'hh_ge_6']
    assert not missing, missing
    perms = D.v3_permutation_table()
    assert sorted(p['perm'] for p in perms) == sorted({(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)})
    outs = [R.distort(src, p) for p in perms]
    assert all(not np.array_equal(outs[0], o) for o in outs[1:])


def test_v3_planted_pixels_enter_the_wrap_loop():
    src, params, cols = D.v3_planted()
    for p, col in zip(params, cols):
        c = v3_branch_counts(src[:1, col:col + 1], p)
        assert c['hh_ge_6'] == 1, (col, c)
        hsv = R.bgr2hsv(src[:1, col:col + 1].astype(F32))
        h = hsv[..., 0] + F32(p['hue'])
        h = np.where(h < 0, h + F32(360), h).astype(F32)
        assert h.item() == 360.0 and (h * R.HSCALE).astype(F32).item() > 6.0
    assert v3_branch_counts(src[:1, 3:4], params[3])['wrap_lo'] == 1


# ---- 5. resampling of the v3 kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', ['horizontal', 'vertical', 'diagonal'])
def test_v3_resample_crops_straddle_the_placed_image(flip):
    src, params = D.v3_resample_case(flip)
    h, w = src.shape[:2]
    ratios = set()
    for p in params:
        H, W, left, top = p['expand']
        x1, y1, x2, y2 = p['crop']
        assert 0 <= left and left + w <= W and 0 <= top and top + h <= H and 0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H
        inside = x1 < left + w and x2 > left and y1 < top + h and y2 > top
        within = x1 >= left and x2 <= left + w and y1 >= top and y2 <= top + h
        assert inside and not within and p['flip'] == flip
        ratios.add(((y2 - y1, p['rh']), (x2 - x1, p['rw'])))
        out = R.pipeline(src, p, (0, 0, 0), (1, 1, 1), False, 32, D.V3_RESAMPLE_FILL)
        assert out.shape == (3, -(-p['rh'] // 32) * 32, -(-p['rw'] // 32) * 32) and not np.isnan(out).any()
    assert ratios == {((48, 48), (64, 64)), ((24, 48), (32, 64)), ((96, 48), (128, 64)), ((7, 64), (7, 64)),
                      ((200, 33), (200, 33)), ((50, 64), (75, 43))}
