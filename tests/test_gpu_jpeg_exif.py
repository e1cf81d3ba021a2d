"""EXIF orientation in the GPU pixel stage, bit for bit against Pillow's ``ImageOps.exif_transpose``
(``tests/golden/jpeg_exif.npz``): every file alone and as one batch mixed with untagged files, in all three entropy
modes, BGR and RGB, into a guarded buffer at a wider pitch; ``orientation=False`` keeps the unrotated pixels."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def files(golden):
    """name -> (bytes, expected oriented RGB, unrotated RGB)"""
    g = golden('jpeg_exif')
    return {str(n): (g['jpg_' + str(n)].tobytes(), g['rgb_' + str(n)], g['rgb_' + str(b)])
            for n, b in zip(g['names'], g['plain'])}


@pytest.fixture(scope='module')
def untagged(golden):
    g = golden('jpeg')
    return [(g['jpg_' + n].tobytes(), g['rgb_' + n]) for n in ('9x7_420_grad_q90', '37x53_422_noise_q90', '48x64_gray_grad_q90')]


def test_every_file_alone_equals_exif_transpose(files, gpu_device):
    for name, (buf, rgb, _) in files.items():
        got = pkg.imdecode(buf, device=gpu_device, orientation=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == rgb.shape and got.is_contiguous(), name
        np.testing.assert_array_equal(got.cpu().numpy(), rgb[:, :, ::-1], err_msg=name)
        got = pkg.imdecode(buf, channel_order='rgb', device=gpu_device, orientation=True)
        np.testing.assert_array_equal(got.cpu().numpy(), rgb, err_msg=name)


@pytest.mark.parametrize('entropy', image_io.ENTROPY_MODES)
def test_one_mixed_batch_in_every_entropy_mode(files, untagged, gpu_device, entropy):
    bufs, want = [], []
    for i, (buf, rgb, _) in enumerate(files.values()):
        bufs.append(buf)
        want.append(rgb)
        if i % 9 == 0:      # untagged files between the tagged ones
            b, r = untagged[(i // 9) % len(untagged)]
            bufs.append(b)
            want.append(r)
    kw = dict(chunk_bytes=16) if entropy == 'device_sync' else {}      # small chunks: the fixture files take the chunk path
    got = pkg.imdecode(bufs, device=gpu_device, entropy=entropy, orientation=True, **kw)
    for n, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.cpu().numpy(), b[:, :, ::-1], err_msg=f'image {n}')
    got = pkg.imdecode(bufs, channel_order='rgb', device=gpu_device, entropy=entropy, orientation=True, **kw)
    for n, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=f'image {n}')


def test_orientation_off_returns_the_unrotated_pixels(files, gpu_device):
    bufs = [b for b, _, _ in files.values()]
    for got in (pkg.imdecode(bufs, device=gpu_device), pkg.imdecode(bufs, device=gpu_device, orientation=False)):
        for (name, (_, _, plain)), a in zip(files.items(), got):
            np.testing.assert_array_equal(a.cpu().numpy(), plain[:, :, ::-1], err_msg=name)
    path_less = pkg.LoadImageFromFile(color_type='color_ignore_orientation')
    assert path_less.apply_orientation is False


def test_wider_pitch_in_a_guarded_buffer_leaves_the_guard_untouched(files, gpu_device):
    """Every oriented image into its own region of one guard-filled buffer: 5 bytes in front of each row, 11 behind,
    two guard rows above and below (the odd offset also takes the word stores of the plain kernel off their alignment)."""
    GUARD = 0xA5
    place, regions, off = [], [], 7
    for _, rgb, _ in files.values():
        h, w = rgb.shape[:2]
        pitch = 3 * w + 16
        place.append((off + 2 * pitch + 5, pitch))
        regions.append((off, h, w, pitch))
        off += (h + 4) * pitch + 64
    out = torch.full((off,), GUARD, dtype=torch.uint8, device=gpu_device)
    _, table = image_io.decode_into([b for b, _, _ in files.values()], 'bgr', gpu_device, out=out, placement=place,
                                    orientation=True)
    got = out.cpu().numpy()
    mask = np.zeros(off, bool)
    for (start, h, w, pitch), (name, (_, rgb, _)), t in zip(regions, files.items(), table):
        assert image_io.oriented_size(t) == (h, w), name
        rows = got[start:start + (h + 4) * pitch].reshape(h + 4, pitch)
        np.testing.assert_array_equal(rows[2:2 + h, 5:5 + 3 * w].reshape(h, w, 3), rgb[:, :, ::-1], err_msg=name)
        mask[start:start + (h + 4) * pitch].reshape(h + 4, pitch)[2:2 + h, 5:5 + 3 * w] = True
    assert (got[~mask] == GUARD).all()


@pytest.mark.parametrize('entropy', image_io.ENTROPY_MODES)
def test_pitch_too_narrow_for_a_transposed_picture_is_refused_before_any_launch(files, gpu_device, entropy):
    """13 x 29 under orientation 6 is 29 rows of 13 pixels; 48 x 64 under 5 is 64 rows of 48.  A pitch that holds the
    unrotated row but a buffer that ends with the unrotated picture, and a pitch below the oriented row, are refused, and
    nothing is written."""
    buf = files['48x64_422_o5'][0]
    out = torch.zeros(64 * 48 * 3, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(ValueError, match='pitch'):
        image_io.decode_into([buf], 'bgr', gpu_device, out=out, placement=[(0, 3 * 48 - 1)], entropy=entropy, orientation=True)
    torch.cuda.synchronize()
    assert not out.any()
    image_io.decode_into([buf], 'bgr', gpu_device, out=out, placement=[(0, 3 * 48)], entropy=entropy, orientation=True)
    np.testing.assert_array_equal(out.cpu().numpy().reshape(64, 48, 3), files['48x64_422_o5'][1][:, :, ::-1])
    # the library's own check, on the host table: the unrotated pitch (3 * 64) does not fit 64 rows into this buffer
    out.zero_()
    with pytest.raises(pkg._lib.Yv4Error, match='output buffer'):
        image_io.decode_into([buf], 'bgr', gpu_device, out=out, placement=[(0, 3 * 64)], entropy='host', orientation=True)
    torch.cuda.synchronize()
    assert not out.any()
