"""The Huffman scan decoded on the GPU (``csrc/jpeg_entropy.hip``) against the host decoder ``yv4_jpeg_entropy_decode``,
element for element: every file of ``jpeg.npz`` and ``jpeg_entropy.npz`` alone and as one interleaved batch, twice, inside
guard words; then ``imdecode(entropy='device')`` against the fixtures' pixels, ``LoadImageFromFile`` and
``inference_detector`` against the host path, and what a damaged file and a bad table do."""
import ctypes

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
from test_gpu_jpeg import PIPELINE, _tiny_detector

pytestmark = pytest.mark.gpu
GUARD, SGUARD, PAD = 0x5A5A, 0x5A5A5A5A, 256


@pytest.fixture(scope='module')
def files(golden):
    """name -> (bytes, Pillow's RGB decode); the restart files of jpeg_entropy.npz spread among the others, so that in the
    batch workgroup boundaries fall inside images (90 segments: 64 + 26) and between them."""
    a, b = golden('jpeg'), golden('jpeg_entropy')
    plain = [(str(n), a) for n in a['names']]
    special = [(str(n), b) for n in b['names']]
    order = []
    for i, item in enumerate(plain):
        if i % 16 == 3 and special:
            order.append(special.pop(0))
        order.append(item)
    return {n: (g['jpg_' + n].tobytes(), g['rgb_' + n]) for n, g in order + special}


@pytest.fixture(scope='module')
def damaged(golden):
    b = golden('jpeg_entropy')
    return {str(n): b['jpg_' + str(n)].tobytes() for n in b['damaged']}


@pytest.fixture(scope='module')
def host_coef(files):
    """The oracle's coefficients of every file: computed once."""
    return {n: image_io.jpeg_entropy_decode(buf)[1] for n, (buf, _) in files.items()}


def _guarded(bufs, device):
    """The device decode into guarded buffers -> (tables, coefficients, status), after checking the guard words."""
    t = image_io.ScanTables(bufs)
    cbuf = torch.full((t.ncoef + 2 * PAD,), GUARD, dtype=torch.int16, device=device)
    sbuf = torch.full((len(bufs) + 2 * PAD,), SGUARD, dtype=torch.int32, device=device)
    image_io.jpeg_entropy_decode_device(bufs, device, coef=cbuf[PAD:PAD + t.ncoef], status=sbuf[PAD:PAD + len(bufs)], tables=t)
    c, s = cbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (c[:PAD] == GUARD).all() and (c[PAD + t.ncoef:] == GUARD).all(), 'a store left the coefficient buffer'
    assert (s[:PAD] == SGUARD).all() and (s[PAD + len(bufs):] == SGUARD).all(), 'a store left the status array'
    return t, c[PAD:PAD + t.ncoef], s[PAD:PAD + len(bufs)]


@pytest.fixture(scope='module')
def batch(files, gpu_device):
    return _guarded([b for b, _ in files.values()], gpu_device)


def test_each_file_alone_equals_the_host_decoder(files, host_coef, gpu_device):
    assert len(files) == 79 + 5
    for name, (buf, _) in files.items():
        t, coef, status = _guarded([buf], gpu_device)
        assert status[0] == 0, name
        np.testing.assert_array_equal(coef, host_coef[name], err_msg=name)


def test_one_interleaved_batch_equals_the_single_calls(files, host_coef, batch):
    t, coef, status = batch
    assert not status.any()
    runs = [(w.image, w.first_seg, w.count) for w in t.wgs]
    assert t.nwg == len(files) + 3 and sum(c == 64 for _, _, c in runs) == 3      # three images cross a workgroup
    names = list(files)
    assert 0 < names.index('72x80_444_grad_q90_rst1') < names.index('72x80_444_noise_q100_rst1') < len(names) - 1
    for name, sc in zip(names, t.scans):
        np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], host_coef[name], err_msg=name)


def test_two_runs_of_the_batch_give_identical_bytes(files, batch, gpu_device):
    t, coef, status = _guarded([b for b, _ in files.values()], gpu_device)
    assert coef.tobytes() == batch[1].tobytes() and status.tobytes() == batch[2].tobytes()


def test_imdecode_device_equals_the_fixture_pixels(files, gpu_device):
    bufs = [b for b, _ in files.values()]
    for order in ('bgr', 'rgb'):
        got = pkg.imdecode(bufs, channel_order=order, device=gpu_device, entropy='device')
        for (name, (_, rgb)), img in zip(files.items(), got):
            assert img.dtype == torch.uint8 and img.device == gpu_device and img.is_contiguous()
            np.testing.assert_array_equal(img.cpu().numpy(), rgb if order == 'rgb' else rgb[:, :, ::-1], err_msg=name)
    for name in ('72x80_444_grad_q90_rst1', '8x8_gray_block_q90', '37x53_422_grad_q30_opt'):      # single calls
        got = pkg.imdecode(files[name][0], device=gpu_device, entropy='device')
        np.testing.assert_array_equal(got.cpu().numpy(), files[name][1][:, :, ::-1], err_msg=name)


def test_placement_and_out_work_as_with_the_host_path(files, gpu_device):
    names = ('72x80_420_grad_q90_rst1', '17x33_420_grad_q90', '72x80_444_grad_q90_rst1_fill')
    place, off = [], 64
    for n in names:
        h, w = files[n][1].shape[:2]
        place.append((off + 5, 3 * w + 16))
        off += h * (3 * w + 16) + 64
    outs = []
    for mode in ('host', 'device'):
        out = torch.full((off,), 0xA5, dtype=torch.uint8, device=gpu_device)
        image_io.decode_into([files[n][0] for n in names], 'bgr', gpu_device, out=out, placement=place, entropy=mode)
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and (outs[0] != 0xA5).any()


def test_load_image_from_file_and_inference_detector_follow_the_setting(files, gpu_device, tmp_path):
    names = ('72x80_444_grad_q90_rst1', '40x72_422_grad_q90', '72x80_420_grad_q90_rst1', '37x53_gray_grad_q90')
    paths = []
    for n in names:
        paths.append(tmp_path / f'{n}.jpg')
        paths[-1].write_bytes(files[n][0])
    for to_float32 in (False, True):
        res = [pkg.LoadImageFromFile(to_float32=to_float32, entropy=mode)(
            dict(img_prefix=str(tmp_path), img_info=dict(filename=paths[0].name))) for mode in ('host', 'device')]
        assert res[0].keys() == res[1].keys() and res[0]['img_shape'] == res[1]['img_shape'] == (72, 80, 3)
        assert res[0]['img'].dtype == res[1]['img'].dtype and torch.equal(res[0]['img'], res[1]['img'])
    det = _tiny_detector(gpu_device)
    want = pkg.inference_detector(det, [str(p) for p in paths], test_pipeline=PIPELINE)
    assert sum(r.shape[0] for res in want for r in res) > 0
    assert pkg.set_default_entropy('device') == 'host'
    try:
        got = pkg.inference_detector(det, [str(p) for p in paths], test_pipeline=PIPELINE)
        one = pkg.inference_detector(det, paths[2], test_pipeline=PIPELINE)
        img = pkg.imread(paths[0], device=gpu_device)
    finally:
        pkg.set_default_entropy('host')
    assert all(a.tobytes() == b.tobytes() for ra, rb in zip(want, got) for a, b in zip(ra, rb))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, want[2]))
    np.testing.assert_array_equal(img.cpu().numpy(), files[names[0]][1][:, :, ::-1])


def test_a_damaged_file_in_a_batch_names_itself_and_the_rest_decodes_afterwards(files, damaged, golden, gpu_device):
    names = ('72x80_420_grad_q90_rst1', '9x7_420_grad_q90', '72x80_444_grad_q90_rst1', '48x64_444_noise_q90')
    good = [files[n][0] for n in names]
    for bad, reason in (('inserted', 'restart marker'), ('cut_last', 'ends inside a block')):      # found by the kernel
        with pytest.raises(ValueError, match=f'image 2.*{reason}'):
            pkg.imdecode(good[:2] + [damaged[bad]] + good[2:], device=gpu_device, entropy='device')
        t, coef, status = _guarded(good[:2] + [damaged[bad]] + good[2:], gpu_device)
        assert status.tolist() == [0, 0, dict(inserted=5, cut_last=1)[bad], 0, 0]
    for bad in ('swapped', 'removed', 'cut_mid'):                                                     # found by prepare
        with pytest.raises(ValueError, match='image 1.*restart marker'):
            pkg.imdecode(good[:1] + [damaged[bad]] + good[1:], device=gpu_device, entropy='device')
    for bad in damaged:                                                    # the host path: the same exception class
        with pytest.raises(ValueError, match='image 1'):
            pkg.imdecode(good[:1] + [damaged[bad]] + good[1:], device=gpu_device, entropy='host')
    got = pkg.imdecode(good, device=gpu_device, entropy='device')
    for n, img in zip(names, got):
        np.testing.assert_array_equal(img.cpu().numpy(), files[n][1][:, :, ::-1], err_msg=n)
    with pytest.raises(NotImplementedError, match='image 1'):
        pkg.imdecode([good[0], golden('jpeg')['jpg_progressive'].tobytes()], device=gpu_device, entropy='device')


def test_tables_that_address_memory_outside_the_buffers_are_refused_before_the_launch(files, host_coef, gpu_device):
    name = '72x80_444_grad_q90_rst1'
    buf = files[name][0]
    cbuf = torch.full((host_coef[name].size + 2 * PAD,), GUARD, dtype=torch.int16, device=gpu_device)
    coef = cbuf[PAD:PAD + host_coef[name].size]
    for where, field, val, msg in (('scans', 'coef_off', 64, 'coefficients leave'), ('scans', 'data_len', 1 << 20, 'byte buffer'),
                                   ('scans', 'huff_base', 1, 'Huffman tables'), ('scans', 'mcus_y', 10, 'ncoef'),
                                   ('segs', 'end', 1 << 20, 'leaves the file'), ('segs', 'mcu_count', 2, 'MCU range'),
                                   ('wgs', 'count', 65, 'workgroup')):
        t = image_io.ScanTables([buf])
        setattr(getattr(t, where)[0], field, val)
        with pytest.raises(pkg._lib.Yv4Error, match=msg):
            image_io.jpeg_entropy_decode_device([buf], gpu_device, coef=coef, tables=t)
    assert (cbuf.cpu().numpy() == GUARD).all()
    t, got, status = image_io.jpeg_entropy_decode_device([buf], gpu_device, coef=coef)
    assert int(status.cpu()[0]) == 0 and (ctypes.sizeof(t.segs), t.nwg) == (90 * 40, 2)
    np.testing.assert_array_equal(got.cpu().numpy(), host_coef[name])
