"""The train-side augmentation kernels (csrc/augment.hip, csrc/augment_v3.hip) on the constructed inputs of
tests/_aug_edge_data.py, bit for bit against oracle/augment_oracle.py and tests/_v3_aug_ref.py: the mosaic kernel's colour
jitter on every one of the 2^24 BGR values and at the corners of the gain ranges, its geometry at an output side that is no
multiple of the launch tile, on a canvas that needs no padding and inside the padding; aug_boxes_kernel past one 64-box
pass and on its four strict thresholds; the v3 kernel's photometric chain over a table of parameters that takes every
branch, and its resampling where the coefficients clamp.  tests/test_augment_edges_host.py proves from the references
alone that the inputs reach those branches.  No tolerance anywhere: integer pixel arithmetic, IEEE float32 / float64
compiled without contraction."""
import numpy as np
import pytest
import torch

from mmdet_yolov4_amd.augment import FusedTrainPipeline
from mmdet_yolov4_amd.augment_v3 import FusedV3TrainPipeline
from oracle import augment_oracle as A

import _aug_edge_data as D
import _v3_aug_ref as R
from test_augment_edges_host import boxes_reference, mosaic_reference, v3_distorted

pytestmark = pytest.mark.gpu

NO_BOXES = (np.zeros((0, 4), np.float32), np.zeros(0, np.int64))


def assert_same_floats(got, want):
    """Equal values, no NaN, and the same bits (zero signs included)."""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 1. colour jitter of the mosaic kernel ---------------------------------------------------------------------------------
def _colour_pipe(tile):
    """Identity geometry: the image before the jitter IS the stitched tiles, the float image is the jittered canvas."""
    return FusedTrainPipeline(img_scale=(tile, tile), pad_val=114, pad_to=2 * tile, crop=2 * tile, scale_limit=0.0,
                              out_size=2 * tile, flip_p=0.0, min_area=-1.0, min_visibility=-1.0, min_size=-1,
                              hsv=D.HSV_RATIOS, mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False)


def _jittered(canvas, gains):
    return np.ascontiguousarray(A.hsv_jitter(canvas, gains).astype(np.float32).transpose(2, 0, 1))


@pytest.mark.parametrize('quarter', [0, 1, 2, 3])
def test_mosaic_colour_jitter_on_every_colour(gpu_device, quarter):
    """Quarter ``quarter`` of the colour cube (red in [64 q, 64 q + 64), every green and blue) at the recipe's largest
    gains: 2^22 pixels through BGR -> HSV, the three LUTs and HSV -> BGR.  The four cases hold all 2^24 colours."""
    tiles = D.cube_quarter_tiles(quarter)
    canvas = D.stitch4(tiles)
    pipe = _colour_pipe(D.CUBE_TILE)
    four = [(torch.from_numpy(t).to(gpu_device),) + NO_BOXES for t in tiles]
    out = pipe([four], params=[dict(h_start=0.0, w_start=0.0, scale=1.0, flip=False, hsv=D.CUBE_GAINS)], return_u8=True)
    np.testing.assert_array_equal(out['img_u8'][0].cpu().numpy(), canvas)
    assert_same_floats(out['img'][0].cpu().numpy(), _jittered(canvas, D.CUBE_GAINS))
    assert len(out['gt_bboxes'][0]) == 0 and len(out['gt_labels'][0]) == 0


def test_mosaic_colour_jitter_at_the_gain_corners(gpu_device):
    """The 28-level grid (21,952 colours) at all eight corners of the gain ranges, one batch of 8."""
    tiles = D.grid_tiles()
    canvas = D.stitch4(tiles)
    corners = D.gain_corners()
    four = [(torch.from_numpy(t).to(gpu_device),) + NO_BOXES for t in tiles]
    out = _colour_pipe(D.GRID_TILE)([four] * 8, params=[dict(h_start=0.0, w_start=0.0, scale=1.0, flip=False, hsv=g)
                                                        for g in corners], return_u8=True)
    u8, img = out['img_u8'].cpu().numpy(), out['img'].cpu().numpy()
    assert img.shape == (8, 3, 2 * D.GRID_TILE, 2 * D.GRID_TILE)
    for n, gains in enumerate(corners):
        np.testing.assert_array_equal(u8[n], canvas)
        assert_same_floats(img[n], _jittered(canvas, gains))


# ---- 2. geometry of the mosaic kernel --------------------------------------------------------------------------------------
def _pitched(img, dev):
    """``img`` as a column slice of a wider device tensor: the row pitch exceeds 3 * w."""
    wide = np.full((img.shape[0], img.shape[1] + 5, 3), 201, np.uint8)
    wide[:, :img.shape[1]] = img
    view = torch.from_numpy(wide).to(dev)[:, :img.shape[1]]
    assert view.stride(0) > 3 * img.shape[1]
    return view


def _run_geometry_case(case, dev):
    pipe = FusedTrainPipeline(img_scale=case['img_scale'], pad_val=114, pad_to=D.GEO['pad_to'], crop=D.GEO['crop'],
                              out_size=D.GEO['out'])                          # every other argument: the recipe's default
    samples = [[(_pitched(f[0], dev) if i == case['pitched'] else torch.from_numpy(f[0]).to(dev), f[1], f[2])
                for i, f in enumerate(four)] for four in case['samples']]
    out = pipe(samples, params=case['params'], return_u8=True)
    N, O = len(samples), D.GEO['out']
    assert out['img'].shape == (N, 3, O, O) and out['img_u8'].shape == (N, O, O, 3)
    u8, img = out['img_u8'].cpu().numpy(), out['img'].cpu().numpy()
    for n in range(N):
        geo, want, boxes, labels = mosaic_reference(case['samples'][n], case['params'][n], case['img_scale'])
        np.testing.assert_array_equal(u8[n], geo)
        assert_same_floats(img[n], want)
        np.testing.assert_array_equal(out['gt_bboxes'][n].cpu().numpy(), boxes)
        np.testing.assert_array_equal(out['gt_labels'][n].cpu().numpy(), labels)
        assert out['gt_labels'][n].dtype == torch.int64
    return u8, img


@pytest.mark.parametrize('call', range(D.CASE_A_CALLS))
def test_mosaic_geometry_at_an_odd_output_side(gpu_device, call):
    """Case a: a 67-pixel output (no multiple of the 64 x 4 launch tile) in batches of three, so that a thread past the
    edge would write into the next image; the twelve parameter sets of the table three to a call: S = 67 / 100 / 134 / 201,
    crop origins first, middle and last, both flips; tiles Resize enlarges, shrinks and copies in every quadrant, one
    source per call with a row pitch wider than its row."""
    _run_geometry_case(D.geometry_case_a(call), gpu_device)


def test_mosaic_geometry_on_a_canvas_that_needs_no_padding(gpu_device):
    """Case b: the stitched canvas (240) is at least as large as PadIfNeeded's size (201): top = left = 0."""
    _run_geometry_case(D.geometry_case_b(), gpu_device)


def test_mosaic_geometry_inside_the_padding(gpu_device):
    """Case c: the crop window sees padding only; every output pixel is the jittered, normalised pad colour."""
    case = D.geometry_case_c()
    u8, img = _run_geometry_case(case, gpu_device)
    assert (u8 == 114).all()
    pad = A.hsv_jitter(np.full((1, 1, 3), 114, np.uint8), case['params'][0]['hsv'])
    want = A.normalize_chw(pad)
    assert (img[0] == want).all() and want[0, 0, 0] != 0


# ---- 3. aug_boxes_kernel -----------------------------------------------------------------------------------------------------
def _run_boxes(data, geo, thresholds, dev):
    pipe = FusedTrainPipeline(img_scale=geo['img_scale'], pad_val=0, pad_to=geo['pad_to'], crop=geo['crop'],
                              scale_limit=geo['scale_limit'], out_size=geo['out'], hsv=None, max_boxes=8,
                              **thresholds)
    blank = {hw: torch.zeros(hw + (3,), dtype=torch.uint8, device=dev) for four in data['samples'] for hw, _, _ in four}
    samples = [[(blank[hw], b, l) for hw, b, l in four] for four in data['samples']]
    out = pipe(samples, params=data['params'])
    for n, (four, prm) in enumerate(zip(data['samples'], data['params'])):
        boxes, labels = boxes_reference(four, prm, geo['img_scale'], **thresholds)
        got_b, got_l = out['gt_bboxes'][n].cpu().numpy(), out['gt_labels'][n].cpu().numpy()
        assert got_b.dtype == np.float32 and not np.isnan(got_b).any()
        np.testing.assert_array_equal(got_l, labels)                            # which boxes, and in which order
        np.testing.assert_array_equal(got_b, boxes)
        np.testing.assert_array_equal(got_b.view(np.uint32), boxes.view(np.uint32))
    return out


def test_boxes_past_one_pass_keep_their_order(gpu_device):
    """Samples of 64, 65, 0 and 180 boxes in one call: one full pass, a pass of one box, none, and three passes with the
    last partial; the kept boxes and their labels equal the oracle's, row for row."""
    out = _run_boxes(D.crowded_boxes(), D.BOX_GEO, D.BOX_THRESHOLDS, gpu_device)
    assert len(out['gt_labels'][2]) == 0 and out['gt_bboxes'][2].shape == (0, 4)


def test_boxes_on_the_strict_thresholds(gpu_device):
    """A box exactly on min_size, min_area, min_visibility or max_aspect_ratio is dropped, its nearest neighbour kept."""
    data = D.threshold_boxes()
    out = _run_boxes(data, D.THR_GEO, D.THR_THRESHOLDS, gpu_device)
    kept = set(out['gt_labels'][0].tolist())
    assert kept == {past for _, past in data['pairs'].values()}


# ---- 4. photometric chain of the v3 kernel ---------------------------------------------------------------------------------
def _v3_identity(src, params, dev):
    """``src`` through FusedV3TrainPipeline with identity geometry and normalisation, one output image per parameter set:
    the resized region equals R.distort (value for value), the whole padded image R.pipeline (bit for bit)."""
    pipe = FusedV3TrainPipeline(mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False)
    d = torch.from_numpy(src).to(dev)
    out = pipe([(d,) + NO_BOXES] * len(params), params=params)
    img = out['img'].cpu().numpy()
    h, w = src.shape[:2]
    assert img.shape == (len(params), 3, -(-h // 32) * 32, -(-w // 32) * 32) and not np.isnan(img).any()
    for n, p in enumerate(params):
        np.testing.assert_array_equal(img[n, :, :h, :w], v3_distorted(src, p))
        assert_same_floats(img[n], R.pipeline(src, p, pipe.mean, pipe.std, pipe.to_rgb, pipe.size_divisor, pipe.expand_fill))


@pytest.mark.parametrize('hue', D.V3_HUES)
def test_v3_photometric_chain_over_the_parameter_table(gpu_device, hue):
    """The 28-level grid under brightness {off, -32, 32} x contrast {off, 0.5 / 1.5 first, 0.5 / 1.5 last} x saturation
    {off, 0.5, 1.5}, 45 sets per hue value {off, -18, 18, -0.5}: negative and over-255 intermediates, both hue wraps,
    the s == 0 shortcut, the v == r == g and v == g == b ties, every sector."""
    _v3_identity(D.v3_grid_source(), D.v3_photometric_table(hue), gpu_device)


def test_v3_channel_permutations(gpu_device):
    _v3_identity(D.v3_grid_source(), D.v3_permutation_table(), gpu_device)


def test_v3_hue_exactly_on_360_enters_the_wrap_loop(gpu_device):
    """h + delta == 360 is not wrapped by `h > 360`; h * (6 / 360) = 6.0000005 then takes the `hh >= 6` loop."""
    src, params, _ = D.v3_planted()
    _v3_identity(src, params, gpu_device)


# ---- 5. resampling of the v3 kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', ['horizontal', 'vertical', 'diagonal'])
def test_v3_resampling_at_its_coefficient_edges(gpu_device, flip):
    """Identity, exactly 2x and 1/2, 7 -> 64, 200 -> 33 and a non-square 50 x 75 -> 64 x 43, each crop across an edge of
    the placed image so that taps mix distorted pixels with Expand's (non-zero) fill: one ragged batch per direction."""
    src, params = D.v3_resample_case(flip)
    pipe = FusedV3TrainPipeline(expand_mean=D.V3_RESAMPLE_FILL, flip_direction=flip, mean=(123.675, 116.28, 103.53),
                                std=(58.395, 57.12, 57.375), to_rgb=True)
    d = torch.from_numpy(src).to(gpu_device)
    out = pipe([(d,) + NO_BOXES] * len(params), params=params)
    img = out['img'].cpu().numpy()
    assert img.shape == (len(params), 3, 64, 64)
    for n, p in enumerate(params):
        want = R.pipeline(src, p, pipe.mean, pipe.std, pipe.to_rgb, pipe.size_divisor, pipe.expand_fill)
        ph, pw = want.shape[1:]
        assert_same_floats(np.ascontiguousarray(img[n, :, :ph, :pw]), want)
        assert not img[n, :, ph:].any() and not img[n, :, :, pw:].any()
