"""Constructed inputs for the train-side augmentation kernels (TEST INFRASTRUCTURE ONLY): pure numpy, deterministic,
nothing imported from the package.  Each builder aims at branches and edges of csrc/augment.hip / csrc/augment_v3.hip that
seeded noise reaches only by luck; tests/test_augment_edges_host.py proves from the references alone that every builder
reaches what it is for, tests/test_gpu_augment_edges.py runs the kernels on them."""
import itertools

import numpy as np

#: 28 levels per channel: 0 / 255 and their neighbours, every power of two with its neighbours, the byte's middle
GRID_LEVELS = (0, 1, 2, 3, 5, 8, 16, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 191, 192, 193, 224, 240, 250, 252,
               253, 254, 255)


def grid_colours():
    """All 28^3 = 21,952 BGR triples of GRID_LEVELS, (21952, 3) uint8, b fastest."""
    lv = np.asarray(GRID_LEVELS, dtype=np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing='ij')
    return np.stack([b.ravel(), g.ravel(), r.ravel()], -1)


def stitch4(tiles):
    """Four equal square tiles -> the mosaic canvas (tile 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right)."""
    return np.ascontiguousarray(np.concatenate([np.concatenate([tiles[0], tiles[1]], 1),
                                                np.concatenate([tiles[2], tiles[3]], 1)], 0))


# ---- 1. the mosaic kernel's colour jitter ----------------------------------------------------------------------------------
CUBE_GAINS = (1.015, 1.7, 1.4)                 # the recipe's upper extremes: the saturation and value LUTs clip
CUBE_TILE = 1024


def cube_quarter_tiles(q):
    """Quarter ``q`` of the 8-bit colour cube -- every BGR value whose red channel is in [64 q, 64 q + 64), 2^22 pixels --
    as four (1024, 1024, 3) uint8 tiles of 2^20 pixels each."""
    i = np.arange(1 << 22, dtype=np.uint32)
    px = np.stack([i & 255, (i >> 8) & 255, (i >> 16) + 64 * q], -1).astype(np.uint8)
    return [np.ascontiguousarray(t) for t in px.reshape(4, CUBE_TILE, CUBE_TILE, 3)]


def colour_codes(img):
    """b + 256 g + 65536 r of every pixel, flat."""
    p = img.reshape(-1, 3).astype(np.int64)
    return p[:, 0] | (p[:, 1] << 8) | (p[:, 2] << 16)


GRID_TILE = 112
HSV_RATIOS = (0.015, 0.7, 0.4)                 # configs/yolov4/yolov4l_coco_mosaic.py: hue, saturation, value


def grid_tiles():
    """The 28-level grid as four (112, 112, 3) tiles: its 21,952 colours first, colour 0 in the remaining pixels."""
    px = np.zeros((4 * GRID_TILE * GRID_TILE, 3), np.uint8)
    c = grid_colours()
    px[:len(c)] = c
    return [np.ascontiguousarray(t) for t in px.reshape(4, GRID_TILE, GRID_TILE, 3)]


def gain_corners():
    """The eight corners of the recipe's gain ranges 1 +- ratio."""
    return [tuple(1.0 + s * r for s, r in zip(signs, HSV_RATIOS)) for signs in itertools.product((-1, 1), repeat=3)]


# ---- 2. the mosaic kernel's geometry ---------------------------------------------------------------------------------------
GEO = dict(pad_to=201, crop=134, out=67)       # out: no multiple of 64 or of 4; crop = 2 out; pad_to = 3 out
RECIPE_GAINS = ((1.012, 1.55, 0.7), (0.99, 0.45, 1.33), (1.0149, 1.69, 1.39))


def noisy_sources(rng, sizes, max_boxes=6):
    """Noise on a colour ramp, so that every bilinear tap matters, plus up to ``max_boxes`` boxes per image."""
    out = []
    for (h, w) in sizes:
        k = rng.randint(0, max_boxes + 1)
        xy = rng.rand(k, 2) * [w, h]
        wh = rng.rand(k, 2) * [w / 2, h / 2] + 1
        b = np.concatenate([xy, np.minimum(xy + wh, [w, h])], 1).astype(np.float32)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 / w, yy * 255 / h, (xx + yy) * 255 / (w + h)], -1) + rng.randn(h, w, 3) * 25
        out.append((np.clip(base, 0, 255).astype(np.uint8), b, rng.randint(0, 80, k).astype(np.int64)))
    return out


def _prm(h_start, w_start, scale, flip, hsv):
    return dict(h_start=h_start, w_start=w_start, scale=scale, flip=flip, hsv=hsv, **GEO)


#: case a, img_scale (48, 48): a tile Resize enlarges, one it shrinks, two it copies; rotated over the quadrants per call
CASE_A_SIZES = ((20, 30), (96, 64), (48, 37), (33, 48))
CASE_A_SCALES = (0.5, 0.75, 1.0, 1.5)          # S = 67 (o = 0), 100 (o = 16, odd difference), 134 (single tap), 201 (upscale)
CASE_A_STARTS = (0.0, 0.5, 0.999999)           # the last one reaches the last crop origin H - C
CASE_A_CALLS = 4


def geometry_case_a(call):
    """Call ``call`` (0..3) of case a: three output images.  Over the four calls the twelve parameter sets hold every scale
    three times with both flips, and all nine pairs of (h_start, w_start).  -> dict(img_scale, samples, params, pitched):
    ``pitched`` = the tile index whose source the GPU test passes as a column slice of a wider tensor."""
    rng = np.random.RandomState(500 + call)
    sizes = [CASE_A_SIZES[(i + call) % 4] for i in range(4)]
    samples, params = [], []
    for n in range(3):
        k = 3 * call + n
        samples.append(noisy_sources(rng, sizes))
        params.append(_prm(CASE_A_STARTS[k % 3], CASE_A_STARTS[(k // 3) % 3], CASE_A_SCALES[k % 4],
                           bool((k // 4 + k) % 2), RECIPE_GAINS[k % 3]))
    return dict(img_scale=(48, 48), samples=samples, params=params, pitched=call % 4)


def geometry_case_b():
    """Canvas 240 >= pad_to 201: PadIfNeeded pads nothing (top = left = 0); the crop origin at its last position."""
    rng = np.random.RandomState(510)
    samples = [noisy_sources(rng, [(120, 90), (50, 60), (60, 80), (240, 180)])]
    return dict(img_scale=(120, 120), samples=samples, params=[_prm(0.999999, 0.5, 0.75, True, RECIPE_GAINS[0])],
                pitched=None)


def geometry_case_c():
    """Sources of at most 16 pixels: the canvas is 32 wide in the middle of the 201 padding, and at scale 1.5 the centre
    crop looks at crop coordinates below 90 only, left of and above every tile (tile 0 is 5 wide): padding alone."""
    rng = np.random.RandomState(520)
    samples = [noisy_sources(rng, [(16, 5), (9, 16), (16, 16), (12, 7)])]
    return dict(img_scale=(16, 16), samples=samples, params=[_prm(0.0, 0.0, 1.5, False, RECIPE_GAINS[1])], pitched=None)


# ---- 3. aug_boxes_kernel -----------------------------------------------------------------------------------------------------
BOX_GEO = dict(img_scale=(64, 64), pad_to=192, crop=128, out=64, scale_limit=0.5)
BOX_THRESHOLDS = dict(min_area=4.0, min_visibility=0.2, min_size=2, max_aspect_ratio=20)
BOX_SRC_SIZES = ((64, 64), (128, 128), (64, 32), (32, 16))      # blank sources: Resize copies, halves, copies, doubles
BOX_TILE_COUNTS = ((30, 0, 34, 0), (17, 16, 16, 16), (0, 0, 0, 0), (45, 45, 45, 45))      # 64, 65, 0, 180 per sample
BOX_PARAMS = (dict(h_start=0.5, w_start=0.5, scale=0.5, flip=True),
              dict(h_start=0.3, w_start=0.6, scale=0.6, flip=False),
              dict(h_start=0.0, w_start=0.999999, scale=1.0, flip=True),
              dict(h_start=0.5, w_start=0.5, scale=0.75, flip=False))
#: (sample, index in the sample) of boxes made to survive: the last lane of each full 64-box pass, the one-box pass
BOX_PLANTED = ((0, 63), (1, 64), (3, 63), (3, 127))


def crowded_boxes():
    """Four samples of 64, 65, 0 and 180 boxes (45 per tile: three passes of the kernel's 64-box loop, the last partial,
    and no sample boundary on a multiple of 64) with a distinct label per box; the box in the last lane of every full pass
    and the only box of the one-box pass survive, so that a miscount there shows.  -> dict(samples, params): ``samples[n]`` =
    four (source (h, w), boxes (k, 4) float32 in source pixels, labels (k,) int64)."""
    rng = np.random.RandomState(530)
    samples, label = [], 0
    for counts in BOX_TILE_COUNTS:
        four = []
        for (h, w), k in zip(BOX_SRC_SIZES, counts):
            xy = rng.rand(k, 2) * [w * 0.9, h * 0.9]
            wh = rng.rand(k, 2) * [w * 0.3, h * 0.3] + [w / 64, h / 64]
            b = np.concatenate([xy, np.minimum(xy + wh, [w, h])], 1).astype(np.float32)
            four.append(((h, w), b, np.arange(label, label + k, dtype=np.int64)))
            label += k
        samples.append(four)
    for n, at in BOX_PLANTED:
        i = int(np.searchsorted(np.cumsum(BOX_TILE_COUNTS[n]), at, side='right'))
        (h, w), b, _ = samples[n][i]
        b[at - sum(BOX_TILE_COUNTS[n][:i])] = (0.3 * w, 0.3 * h, 0.7 * w, 0.7 * h)
    params = [dict(p, hsv=None, pad_to=BOX_GEO['pad_to'], crop=BOX_GEO['crop'], out=BOX_GEO['out']) for p in BOX_PARAMS]
    return dict(samples=samples, params=params)


#: canvas 128 = pad_to: nothing is padded; crop origin 0, scale 1, no flip
THR_GEO = dict(img_scale=(64, 64), pad_to=128, crop=96, out=96, scale_limit=0.0)
THR_THRESHOLDS = dict(min_area=16.0, min_visibility=0.25, min_size=2, max_aspect_ratio=20)
_U = 2.0 ** -20                                                            # float32 spacing in [8, 16)


def threshold_boxes():
    """Boxes on and next to the four strict thresholds under a geometry that moves no coordinate (tile 0 sits at the
    canvas origin, the crop starts at 0, scale 1, no flip).  Every coordinate is a dyadic fraction that float32 holds
    exactly, after the tile shift too, so the reference's arithmetic is exact.  The output is canvas[0:96, 0:96]: tile 1
    (x from 64) is cut at x = 96.  -> dict(samples, params, pairs, rejected): ``pairs`` = name -> (label on the threshold:
    rejected, label of its nearest kept neighbour); ``rejected`` = labels of the zero-area and outside boxes."""
    t0 = [  # tile 0: canvas coordinates = source coordinates
        (8, 8, 10, 20),                        # 0  width 2 = min_size
        (8, 8, 10 + _U, 20),                   # 1  width 2 + 2^-20
        (30, 8, 42, 10),                       # 2  height 2 = min_size
        (30, 8, 42, 10 + _U),                  # 3
        (8, 30, 12, 34),                       # 4  area 16 = min_area
        (8, 30, 12, 34 + 4 * _U),              # 5  (float32 spacing in [32, 64) is 2^-18)
        (4, 40, 54, 42.5),                     # 6  50 / 2.5 = 20 = max_aspect_ratio, exact in float32
        (4, 40, 54, 42.5 + 4 * _U),            # 7
        (20, 50, 20, 60),                      # 8  zero area
    ]
    t1 = [  # tile 1: canvas x = source x + 64
        (24, 8, 56, 24),                       # 9  canvas x 88..120, cut at 96: 8 of 32 visible = min_visibility
        (24 - 8 * _U, 30, 56, 46),             # 10 canvas x0 = 88 - 2^-17 (the float32 spacing in [64, 128))
        (28, 50, 40, 54),                      # 11 canvas x 92..104, cut at 96: clipped area 4 x 4 = min_area, a third visible
        (28, 56, 40, 60 + 4 * _U),             # 12
        (40, 20, 60, 40),                      # 13 wholly right of the crop
    ]
    t3 = [(40, 40, 60, 60)]                    # 14 wholly outside, below and right
    boxes = [np.asarray(t, np.float32).reshape(-1, 4) for t in (t0, t1, [], t3)]
    four, label = [], 0
    for b in boxes:
        four.append(((64, 64), b, np.arange(label, label + len(b), dtype=np.int64)))
        label += len(b)
    prm = dict(h_start=0.0, w_start=0.0, scale=1.0, flip=False, hsv=None, pad_to=THR_GEO['pad_to'], crop=THR_GEO['crop'],
               out=THR_GEO['out'])
    pairs = dict(min_size_w=(0, 1), min_size_h=(2, 3), min_area=(4, 5), max_aspect_ratio=(6, 7), min_visibility=(9, 10),
                 min_area_clipped=(11, 12))
    return dict(samples=[four], params=[prm], pairs=pairs, rejected=(8, 13, 14))


# ---- 4. the v3 kernel's photometric chain ----------------------------------------------------------------------------------
def v3_params(h, w, brightness=None, contrast=None, contrast_first=False, saturation=None, hue=None, perm=None,
              expand=None, crop=None, rh=None, rw=None, flip=None):
    """One parameter dict of FusedV3TrainPipeline; the geometry defaults to the identity on an (h, w) source."""
    return dict(brightness=brightness, contrast=contrast, contrast_first=contrast_first, saturation=saturation, hue=hue,
                perm=perm, expand=expand, crop=crop, rh=h if rh is None else rh, rw=w if rw is None else rw, flip=flip)


def v3_grid_source():
    """The 28-level grid as one (28, 784, 3) uint8 image."""
    return np.ascontiguousarray(grid_colours().reshape(28, 784, 3))


V3_HUES = (None, -18, 18, -0.5)
V3_BRIGHTNESS = (None, -32, 32)
V3_CONTRASTS = ((None, False), (0.5, True), (1.5, True), (0.5, False), (1.5, False))
V3_SATURATIONS = (None, 0.5, 1.5)


def v3_photometric_table(hue):
    """The 45 parameter sets of the 180-set table that share one hue value: one batch."""
    return [v3_params(28, 784, brightness=b, contrast=c, contrast_first=first, saturation=s, hue=hue)
            for b in V3_BRIGHTNESS for (c, first) in V3_CONTRASTS for s in V3_SATURATIONS]


def v3_permutation_table():
    """All six channel permutations on one set that takes every photometric step."""
    return [v3_params(28, 784, brightness=-32, contrast=1.5, contrast_first=False, saturation=1.5, hue=18, perm=perm)
            for perm in itertools.permutations(range(3))]


def v3_planted():
    """Pixels whose hue lands exactly on 360 after the shift, so that h * (6 / 360) = 6.0000005 enters the `hh >= 6` wrap
    loop: h + delta == 360 three ways, and a tiny negative hue that `+ 360` rounds up to 360.
    -> (source (2, 4, 3) uint8, parameter sets, the pixel of row 0 each set is aimed at)."""
    src = np.array([[(3, 0, 10), (1, 0, 5), (1, 0, 10), (0, 0, 200)],
                    [(10, 0, 3), (0, 5, 1), (200, 0, 0), (7, 7, 7)]], np.uint8)
    hues = (18, 12, 6, -1e-6)
    return src, [v3_params(2, 4, saturation=1.5, hue=h) for h in hues], (0, 1, 2, 3)


# ---- 5. the v3 kernel's resampling -----------------------------------------------------------------------------------------
V3_RESAMPLE_SRC = (40, 60)
V3_RESAMPLE_EXPAND = (230, 240, 90, 100)       # canvas (H, W), left, top: the image sits at x 90..150, y 100..140
V3_RESAMPLE_FILL = (10, 20, 30)
#: name -> (crop x1, y1, w, h, resized h, w): every crop straddles an edge of the placed image
V3_RESAMPLE_SIZES = dict(identity=(70, 90, 64, 48, 48, 64), twice=(80, 92, 32, 24, 48, 64), half=(60, 70, 128, 96, 48, 64),
                         up_7_to_64=(86, 96, 7, 7, 64, 64), down_200_to_33=(20, 15, 200, 200, 33, 33),
                         non_square=(100, 95, 75, 50, 64, 43))


def v3_resample_case(flip):
    """-> (source uint8 noise, one parameter set per entry of V3_RESAMPLE_SIZES) for one flip direction."""
    rng = np.random.RandomState(540)
    h, w = V3_RESAMPLE_SRC
    src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    params = [v3_params(h, w, brightness=10.5, saturation=1.2, hue=7.25, contrast=0.9, expand=V3_RESAMPLE_EXPAND,
                        crop=(x1, y1, x1 + cw, y1 + ch), rh=rh, rw=rw, flip=flip)
              for (x1, y1, cw, ch, rh, rw) in V3_RESAMPLE_SIZES.values()]
    return src, params
