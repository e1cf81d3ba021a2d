"""JPEG decoding on the GPU, bit for bit against libjpeg-turbo's output (``tests/golden/jpeg.npz``, Pillow's decode of
each file): every fixture alone and all of them as one batch, in BGR and RGB, into guarded buffers at a wider pitch,
twice; then device tensors through ``FusedTestPipeline`` and files through ``inference_detector``."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
import _jpeg_ref as R
from test_jpeg_host import coarse_table_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def jpeg(golden):
    g = golden('jpeg')
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def files(jpeg):
    """name -> (bytes, Pillow's RGB decode)"""
    return {str(n): (jpeg['jpg_' + str(n)].tobytes(), jpeg['rgb_' + str(n)]) for n in jpeg['names']}


@pytest.fixture(scope='module')
def batch_bgr(files, gpu_device):
    """All fixtures in one call (mixed sizes and samplings): computed once, compared by several tests."""
    out = pkg.imdecode([b for b, _ in files.values()], device=gpu_device)
    return [t.cpu().numpy() for t in out]


def test_every_fixture_alone_equals_libjpeg_turbo(files, gpu_device):
    for name, (buf, rgb) in files.items():
        got = pkg.imdecode(buf, device=gpu_device)
        assert got.dtype == torch.uint8 and got.device == gpu_device and tuple(got.shape) == rgb.shape and got.is_contiguous()
        np.testing.assert_array_equal(got.cpu().numpy(), rgb[:, :, ::-1], err_msg=name)
        np.testing.assert_array_equal(pkg.imdecode(buf, channel_order='rgb', device=gpu_device).cpu().numpy(), rgb, err_msg=name)


def test_one_batch_of_all_fixtures_equals_the_single_calls(files, batch_bgr, gpu_device):
    assert len(batch_bgr) == len(files) >= 72
    for (name, (buf, rgb)), got in zip(files.items(), batch_bgr):
        np.testing.assert_array_equal(got, rgb[:, :, ::-1], err_msg=name)
        np.testing.assert_array_equal(got, pkg.imdecode(buf, device=gpu_device).cpu().numpy(), err_msg=name)
    rgb_batch = pkg.imdecode([b for b, _ in files.values()], channel_order='rgb', device=gpu_device)
    for (name, (_, rgb)), got in zip(files.items(), rgb_batch):
        np.testing.assert_array_equal(got.cpu().numpy(), rgb, err_msg=name)


def test_two_runs_of_the_batch_give_identical_bytes(files, batch_bgr, gpu_device):
    again = pkg.imdecode([b for b, _ in files.values()], device=gpu_device)
    for a, b in zip(batch_bgr, again):
        assert a.tobytes() == b.cpu().numpy().tobytes()


def test_wider_pitch_in_a_guarded_buffer_leaves_the_guard_untouched(files, gpu_device):
    """Every image into its own region of one guard-filled buffer: 5 bytes in front of each row, 11 behind, two guard
    rows above and below.  Only the pixels change."""
    GUARD, place, regions, off = 0xA5, [], [], 64
    for buf, rgb in files.values():
        h, w = rgb.shape[:2]
        pitch = 3 * w + 16
        place.append((off + 2 * pitch + 5, pitch))
        regions.append((off, h, w, pitch))
        off += (h + 4) * pitch + 64
    out = torch.full((off,), GUARD, dtype=torch.uint8, device=gpu_device)
    image_io.decode_into([b for b, _ in files.values()], 'bgr', gpu_device, out=out, placement=place)
    got = out.cpu().numpy()
    mask = np.zeros(off, bool)                    # True where a pixel belongs
    for (start, h, w, pitch), (name, (_, rgb)) in zip(regions, files.items()):
        rows = got[start:start + (h + 4) * pitch].reshape(h + 4, pitch)
        np.testing.assert_array_equal(rows[2:2 + h, 5:5 + 3 * w].reshape(h, w, 3), rgb[:, :, ::-1], err_msg=name)
        m = mask[start:start + (h + 4) * pitch].reshape(h + 4, pitch)
        m[2:2 + h, 5:5 + 3 * w] = True
    assert (got[~mask] == GUARD).all()


def test_placement_outside_the_buffer_is_refused_before_the_launch(files, gpu_device):
    buf, rgb = files['17x33_420_grad_q90']
    out = torch.zeros(17 * 99, dtype=torch.uint8, device=gpu_device)
    for place in ((1, 99), (0, 100), (0, 98), (-1, 99)):
        with pytest.raises(pkg._lib.Yv4Error, match='output buffer'):
            image_io.decode_into([buf], 'bgr', gpu_device, out=out, placement=[place])
    assert not out.any()
    image_io.decode_into([buf], 'bgr', gpu_device, out=out, placement=[(0, 99)])
    np.testing.assert_array_equal(out.cpu().numpy().reshape(17, 33, 3), rgb[:, :, ::-1])


def test_out_of_range_file_follows_the_stated_range_limit_rule(jpeg, gpu_device):
    """A hand-made file whose IDCT output reaches the wrap-around of the range-limit table (test_jpeg_host.py): the
    kernel against the restatement, where a clamp gives other bytes."""
    for mult in (20, 40):
        buf = coarse_table_file(jpeg, mult)
        np.testing.assert_array_equal(pkg.imdecode(buf, device=gpu_device).cpu().numpy(), R.decode(buf))


def test_refused_and_damaged_files_raise(jpeg, files, gpu_device):
    with pytest.raises(NotImplementedError, match='progressive'):
        pkg.imdecode(jpeg['jpg_progressive'].tobytes(), device=gpu_device)
    good = files['9x7_420_grad_q90'][0]
    with pytest.raises(NotImplementedError, match='image 1'):             # one bad file of a batch names itself
        pkg.imdecode([good, jpeg['jpg_cmyk'].tobytes()], device=gpu_device)
    with pytest.raises(ValueError, match='image 2'):
        pkg.imdecode([good, good, good[:-20], good], device=gpu_device)


def _tiny_detector(device):
    """The detector of tests/test_gpu_preprocess.py::test_feeds_the_detector."""
    det = pkg.build_detector(dict(
        type='SingleStageDetector',
        backbone=dict(type='DarknetCSP', scale=[['conv', 'bottleneck', 'csp', 'csp'], [None, 1, 1, 1], [8, 16, 16, 32]],
                      out_indices=[1, 2, 3]),
        neck=dict(type='YOLOV4Neck', in_channels=[16, 16, 32], out_channels=[16, 16, 32], csp_repetition=1),
        bbox_head=dict(type='YOLOCSPHead', num_classes=3, in_channels=[16, 16, 32], featmap_strides=[4, 8, 16],
                       anchor_generator=dict(type='YOLOV4AnchorGenerator', strides=[4, 8, 16],
                                             base_sizes=[[(8, 8)] * 3, [(16, 16)] * 3, [(32, 32)] * 3])),
        test_cfg=dict(nms_pre=-1, score_thr=0.001, nms=dict(type='nms', iou_threshold=0.65), max_per_img=10)))
    torch.manual_seed(0)
    det.init_weights()
    return det.eval().to(device)


PIPELINE = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(128, 128), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32),
                             dict(type='Normalize', mean=[114, 114, 114], std=[255, 255, 255], to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


def test_fused_test_pipeline_takes_device_tensors(files, gpu_device):
    arrays = [np.ascontiguousarray(files[n][1][:, :, ::-1]) for n in ('48x64_420_grad_q90', '37x53_444_noise_q90')]
    pipe = pkg.FusedTestPipeline.from_config(PIPELINE, device=gpu_device)
    want, want_metas = pipe(arrays)
    tensors = [torch.from_numpy(a).to(gpu_device) for a in arrays]
    got, metas = pipe(tensors)
    assert torch.equal(got, want)
    mixed, _ = pipe([tensors[0], arrays[1]])
    assert torch.equal(mixed, want)
    for a, b in zip(metas, want_metas):
        assert a.keys() == b.keys()
        for k in a:
            if k == 'img_norm_cfg':
                assert all(np.array_equal(a[k][j], b[k][j]) for j in a[k])
            else:
                assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        pipe([tensors[0].float()])
    with pytest.raises(ValueError):
        pipe([tensors[0].cpu()])


def test_inference_detector_reads_files(files, gpu_device, tmp_path):
    det = _tiny_detector(gpu_device)
    names = ('48x64_420_grad_q90', '40x72_422_grad_q90', '37x53_gray_grad_q90')
    paths = []
    for n in names:
        paths.append(tmp_path / f'{n}.jpg')
        paths[-1].write_bytes(files[n][0])
    arrays = [np.ascontiguousarray(files[n][1][:, :, ::-1]) for n in names]
    want = pkg.inference_detector(det, arrays, test_pipeline=PIPELINE)
    assert sum(r.shape[0] for res in want for r in res) > 0
    got = pkg.inference_detector(det, [str(paths[0]), paths[1], paths[2]], test_pipeline=PIPELINE)      # str and PathLike
    assert all(a.tobytes() == b.tobytes() for ra, rb in zip(want, got) for a, b in zip(ra, rb))
    one = pkg.inference_detector(det, str(paths[0]), test_pipeline=PIPELINE)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, pkg.inference_detector(det, arrays[0], test_pipeline=PIPELINE)))
    mixed = pkg.inference_detector(det, [arrays[0], paths[1], pkg.imread(paths[2], device=gpu_device)], test_pipeline=PIPELINE)
    assert all(a.tobytes() == b.tobytes() for ra, rb in zip(want, mixed) for a, b in zip(ra, rb))


def test_load_image_from_file_fills_the_results(files, gpu_device, tmp_path):
    """loading.py:43-78."""
    (tmp_path / 'a.jpg').write_bytes(files['17x33_420_grad_q90'][0])
    load = pkg.PIPELINES.build(dict(type='LoadImageFromFile', im_decode_backend='turbojpeg'))
    res = load(dict(img_prefix=str(tmp_path), img_info=dict(filename='a.jpg')))
    assert res['filename'] == str(tmp_path / 'a.jpg') and res['ori_filename'] == 'a.jpg' and res['img_fields'] == ['img']
    assert res['img_shape'] == res['ori_shape'] == (17, 33, 3) and res['img'].dtype == torch.uint8
    np.testing.assert_array_equal(res['img'].cpu().numpy(), files['17x33_420_grad_q90'][1][:, :, ::-1])
    res = pkg.LoadImageFromFile(to_float32=True)(dict(img_prefix=None, img_info=dict(filename=str(tmp_path / 'a.jpg'))))
    assert res['img'].dtype == torch.float32 and res['filename'] == str(tmp_path / 'a.jpg')
    np.testing.assert_array_equal(res['img'].cpu().numpy(), files['17x33_420_grad_q90'][1][:, :, ::-1].astype(np.float32))
