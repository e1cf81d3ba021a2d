"""The JPEG kernels on streams that no encoder writes (``tests/_jpeg_synth.py``, ``tests/golden/jpeg_synth.npz``): the
segment kernel (``entropy='device'``) and the chunk kernels (``entropy='device_sync'``) against the coefficients the
writer put into each file, element for element and inside guard words, alone and interleaved with encoder-made files; the
pixel stage against the numpy restatement and, where the fixture has them, libjpeg-turbo's pixels; and the three files
that must not decode inside a batch of valid ones.  Every file here has passed ``test_jpeg_synth_host.py`` on the CPU
run of the same core."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
import _jpeg_ref as R
import _jpeg_synth as S
from test_gpu_jpeg_entropy import _guarded as _guarded_segments
from test_gpu_jpeg_sync import _guarded as _guarded_chunks, _rounds

pytestmark = pytest.mark.gpu
MIN = pkg._lib.JPEG_MIN_CHUNK_BYTES
CHUNK_BYTES = (4, 5, 7, 16, 64)
ENCODER_MADE = ('1x1_420_noise_q90', '9x7_420_grad_q90', '17x33_422_noise_q90', '37x53_gray_grad_q30_opt',
                '17x33_420_grad_q90_rst2', '48x64_444_noise_q100', '16x16_444_grad_q90', '40x72_422_grad_q90')


@pytest.fixture(scope='module')
def synth(golden):
    """name -> (file bytes, the writer's coefficients), the bytes being the fixture's"""
    g = golden('jpeg_synth')
    out = {}
    for n in g['names']:
        data, want, _ = S.make(str(n))
        assert data == g['jpg_' + str(n)].tobytes(), n
        out[str(n)] = (data, want)
    assert len(out) >= 68
    return out


@pytest.fixture(scope='module')
def mixed(golden, synth):
    """The batch: every synthetic file, an encoder-made one after every eighth -> (names, files, coefficients)"""
    a = golden('jpeg')
    names, extra = [], list(ENCODER_MADE)
    for i, n in enumerate(synth):
        names.append(n)
        if i % 8 == 5 and extra:
            names.append(extra.pop(0))
    assert not extra
    bufs = [synth[n][0] if n in synth else a['jpg_' + n].tobytes() for n in names]
    want = [synth[n][1] if n in synth else image_io.jpeg_entropy_decode(b)[1] for n, b in zip(names, bufs)]
    return names, bufs, want


@pytest.fixture(scope='module')
def pixels(golden, mixed):
    """The restatement's RGB decode of every file of the batch, held to libjpeg-turbo's where a fixture has it: once"""
    g, a = golden('jpeg_synth'), golden('jpeg')
    out = []
    for n, b in zip(mixed[0], mixed[1]):
        out.append(R.decode(b, 'rgb'))
        for fixture in (g, a):
            if 'rgb_' + n in fixture.files:
                np.testing.assert_array_equal(out[-1], fixture['rgb_' + n], err_msg=n)
    return out


def _same_batch(names, t, coef, want):
    for n, sc, w in zip(names, t.scans, want):
        np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], w, err_msg=n)


def test_segment_kernel_returns_what_the_writer_wrote(synth, gpu_device):
    for name, (data, want) in synth.items():
        t, coef, status = _guarded_segments([data], gpu_device)
        assert status[0] == 0, name
        np.testing.assert_array_equal(coef, want, err_msg=name)


def test_segment_kernel_on_the_interleaved_batch_twice(mixed, gpu_device):
    names, bufs, want = mixed
    t, coef, status = _guarded_segments(bufs, gpu_device)
    assert not status.any() and max(sc.nhuff for sc in t.scans) == 6 and len({sc.nhuff for sc in t.scans}) >= 3
    _same_batch(names, t, coef, want)
    again = _guarded_segments(bufs, gpu_device)
    assert again[1].tobytes() == coef.tobytes() and again[2].tobytes() == status.tobytes()


@pytest.mark.parametrize('chunk_bytes', CHUNK_BYTES)
def test_chunk_kernels_return_what_the_writer_wrote(synth, gpu_device, chunk_bytes):
    for name, (data, want) in synth.items():
        t, ch, coef, status, undecided = _guarded_chunks([data], gpu_device, chunk_bytes, _rounds([data], chunk_bytes))
        assert status[0] == 0 and undecided[0] == 0, name
        np.testing.assert_array_equal(coef, want, err_msg=name)


@pytest.mark.parametrize('chunk_bytes', CHUNK_BYTES)
def test_chunk_kernels_on_the_interleaved_batch_twice(mixed, gpu_device, chunk_bytes):
    names, bufs, want = mixed
    rounds = _rounds(bufs, chunk_bytes)
    t, ch, coef, status, undecided = _guarded_chunks(bufs, gpu_device, chunk_bytes, rounds)
    assert not status.any() and not undecided.any()
    _same_batch(names, t, coef, want)
    again = _guarded_chunks(bufs, gpu_device, chunk_bytes, rounds)
    assert again[2].tobytes() == coef.tobytes() and not again[3].any() and not again[4].any()


@pytest.mark.parametrize('name', ['wide_ones', 'ones_dense_plain'])
def test_dense_stuffing_at_the_smallest_chunk(synth, gpu_device, name):
    """One segment of more than 64 chunks of four raw bytes: symbols longer than a chunk, chunks that begin on the zero
    of a stuffed pair, chains across workgroups."""
    data, want = synth[name]
    t, ch, coef, status, undecided = _guarded_chunks([data], gpu_device, MIN, _rounds([data], MIN))
    n = t.segs[0].end - t.segs[0].begin
    assert t.nseg == 1 and ch.nchunk == -(-n // MIN) > 128 and ch.nwg == -(-ch.nchunk // 64) > 2
    assert sum(data[t.segs[0].begin + i * MIN] == 0 and data[t.segs[0].begin + i * MIN - 1] == 0xFF for i in range(1, ch.nchunk)) > 0
    assert status[0] == 0 and undecided[0] == 0
    np.testing.assert_array_equal(coef, want)


def test_without_rounds_the_second_decode_carries_the_batch(mixed, pixels, gpu_device):
    names, bufs, want = mixed
    t, ch, coef, status, undecided = _guarded_chunks(bufs, gpu_device, MIN, 0)
    assert not status.any() and undecided.astype(bool).sum() > len(bufs) // 2      # most chains cannot close
    got = pkg.imdecode(bufs, channel_order='rgb', device=gpu_device, entropy='device_sync', chunk_bytes=MIN, max_rounds=0)
    for n, img, px in zip(names, got, pixels):
        np.testing.assert_array_equal(img.cpu().numpy(), px, err_msg=n)


@pytest.mark.parametrize('mode', ['host', 'device', 'device_sync'])
def test_imdecode_equals_the_restatement_in_every_pixel(mixed, pixels, gpu_device, mode):
    names, bufs, _ = mixed
    for order in ('bgr', 'rgb'):
        got = pkg.imdecode(bufs, channel_order=order, device=gpu_device, entropy=mode)
        for n, img, px in zip(names, got, pixels):
            assert img.dtype == torch.uint8 and img.is_contiguous()
            np.testing.assert_array_equal(img.cpu().numpy(), px if order == 'rgb' else px[:, :, ::-1], err_msg=n)
    for n, b, px in zip(names, bufs, pixels):      # every file alone
        img = pkg.imdecode(b, device=gpu_device, entropy=mode, chunk_bytes=MIN if mode == 'device_sync' else None)
        np.testing.assert_array_equal(img.cpu().numpy(), px[:, :, ::-1], err_msg=n)


@pytest.mark.parametrize('mode', ['host', 'device', 'device_sync'])
def test_loud_padding_and_the_basis_files_at_a_wider_pitch_inside_guards(mixed, pixels, gpu_device, mode):
    names, bufs, _ = mixed
    pick = [i for i, n in enumerate(names) if n.startswith(('padding_loud_', 'basis_'))]
    assert len(pick) == 8
    place, off = [], 128
    for i in pick:
        h, w = pixels[i].shape[:2]
        place.append((off + 7, 3 * w + 19))
        off += h * (3 * w + 19) + 128
    for order in ('bgr', 'rgb'):
        out = torch.full((off,), 0xA5, dtype=torch.uint8, device=gpu_device)
        image_io.decode_into([bufs[i] for i in pick], order, gpu_device, out=out, placement=place, entropy=mode)
        flat = out.cpu().numpy()
        rest = np.ones(off, bool)
        for i, (at, pitch) in zip(pick, place):
            h, w = pixels[i].shape[:2]
            px = pixels[i] if order == 'rgb' else pixels[i][:, :, ::-1]
            rows = at + pitch * np.arange(h)[:, None] + np.arange(3 * w)[None, :]
            np.testing.assert_array_equal(flat[rows].reshape(h, w, 3), px, err_msg=names[i])
            rest[rows] = False
        assert (flat[rest] == 0xA5).all(), 'a store outside an image: between the rows, or in front of or behind the images'


@pytest.mark.parametrize('mode', ['device', 'device_sync'])
def test_an_invalid_file_in_a_batch_names_itself_and_leaves_the_others_right(golden, mixed, pixels, gpu_device, mode):
    g = golden('jpeg_synth')
    names, bufs, _ = mixed
    pick = [names.index(n) for n in ('deep_420', 'slots23_444', 'wide_ones', '9x7_420_grad_q90')]
    assert [str(n) for n in g['invalid']] == list(S.INVALID)
    for bad in S.INVALID:
        batch = [bufs[i] for i in pick[:2]] + [g['jpg_' + bad].tobytes()] + [bufs[i] for i in pick[2:]]
        with pytest.raises(ValueError, match='image 2') as want:
            pkg.imdecode(batch, device=gpu_device, entropy='host')
        t = image_io.ScanTables(batch)
        place, off = [], 0
        for f in t.infos:
            place.append((off, 3 * f.width))
            off += 3 * f.width * f.height
        for cb in ((MIN, 64) if mode == 'device_sync' else (None,)):
            with pytest.raises(ValueError) as got:
                pkg.imdecode(batch, device=gpu_device, entropy=mode, chunk_bytes=cb)
            assert str(got.value) == str(want.value), bad
            # the pixels are written before the error is raised: into the caller's buffer they can be looked at
            out = torch.zeros(off, dtype=torch.uint8, device=gpu_device)
            with pytest.raises(ValueError, match='image 2'):
                image_io.decode_into(batch, 'rgb', gpu_device, out=out, placement=place, entropy=mode, chunk_bytes=cb)
            flat = out.cpu().numpy()
            for j, i in zip((0, 1, 3, 4), pick):
                f = t.infos[j]
                got_px = flat[place[j][0]:place[j][0] + 3 * f.width * f.height].reshape(f.height, f.width, 3)
                np.testing.assert_array_equal(got_px, pixels[i], err_msg=f'{bad}: {names[i]}')
