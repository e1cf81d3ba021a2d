"""The Huffman scan decoded on the GPU by many lanes per segment (``entropy='device_sync'``: the chunk kernels of
``csrc/jpeg_entropy.hip``) against the host decoder ``yv4_jpeg_entropy_decode``, element for element: every file of
``jpeg.npz`` and ``jpeg_entropy.npz`` alone and as one interleaved batch, twice, inside guard words; a chain that crosses
workgroups; then ``imdecode(entropy='device_sync')`` against the host path's pixels, the damaged fixtures, and the second
decode on its own."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io

pytestmark = pytest.mark.gpu
GUARD, SGUARD, PAD = 0x5A5A, 0x5A5A5A5A, 256
MIN = pkg._lib.JPEG_MIN_CHUNK_BYTES
NOISE = '72x80_444_noise_q100_rst1'


@pytest.fixture(scope='module')
def files(golden):
    """name -> bytes; the restart files of jpeg_entropy.npz spread among the others (mixed samplings and sizes)"""
    a, b = golden('jpeg'), golden('jpeg_entropy')
    plain = [(str(n), a) for n in a['names']]
    special = [(str(n), b) for n in b['names']]
    order = []
    for i, item in enumerate(plain):
        if i % 16 == 3 and special:
            order.append(special.pop(0))
        order.append(item)
    return {n: g['jpg_' + n].tobytes() for n, g in order + special}


@pytest.fixture(scope='module')
def damaged(golden):
    b = golden('jpeg_entropy')
    return {str(n): b['jpg_' + str(n)].tobytes() for n in b['damaged']}


@pytest.fixture(scope='module')
def host_coef(files):
    """The oracle's coefficients of every file: computed once."""
    return {n: image_io.jpeg_entropy_decode(buf)[1] for n, buf in files.items()}


@pytest.fixture(scope='module')
def host_pixels(files, gpu_device):
    """``imdecode(entropy='host')`` of every file as one batch: computed once."""
    return [img.cpu().numpy() for img in pkg.imdecode(list(files.values()), device=gpu_device, entropy='host')]


def _rounds(bufs, chunk_bytes):
    """The round after which no entry of the batch changes any more, from the CPU run of the same core: the kernels
    have to close every chain in exactly as many."""
    r = image_io.jpeg_entropy_decode_sync(bufs, chunk_bytes, pkg._lib.JPEG_MAX_ROUNDS)
    assert not r[5].any()
    return r[6]


def _guarded(bufs, device, chunk_bytes, max_rounds):
    """The chunk kernels into guarded buffers -> (tables, chunk tables, coefficients, status, undecided), after checking
    the guard words."""
    t = image_io.ScanTables(bufs)
    N = len(bufs)
    cbuf = torch.full((t.ncoef + 2 * PAD,), GUARD, dtype=torch.int16, device=device)
    sbuf = torch.full((N + 2 * PAD,), SGUARD, dtype=torch.int32, device=device)
    ubuf = torch.full((N + 2 * PAD,), SGUARD, dtype=torch.int32, device=device)
    _, ch, _, _, _ = image_io.jpeg_entropy_decode_device_sync(
        bufs, chunk_bytes, max_rounds, device, coef=cbuf[PAD:PAD + t.ncoef], status=sbuf[PAD:PAD + N],
        undecided=ubuf[PAD:PAD + N], tables=t)
    c, s, u = cbuf.cpu().numpy(), sbuf.cpu().numpy(), ubuf.cpu().numpy()
    assert (c[:PAD] == GUARD).all() and (c[PAD + t.ncoef:] == GUARD).all(), 'a store left the coefficient buffer'
    assert (s[:PAD] == SGUARD).all() and (s[PAD + N:] == SGUARD).all(), 'a store left the status array'
    assert (u[:PAD] == SGUARD).all() and (u[PAD + N:] == SGUARD).all(), 'a store left the undecided array'
    return t, ch, c[PAD:PAD + t.ncoef], s[PAD:PAD + N], u[PAD:PAD + N]


@pytest.mark.parametrize('chunk_bytes', [MIN, 64])
def test_each_file_alone_equals_the_host_decoder(files, host_coef, gpu_device, chunk_bytes):
    assert len(files) == 79 + 5
    for name, buf in files.items():
        t, ch, coef, status, undecided = _guarded([buf], gpu_device, chunk_bytes, _rounds([buf], chunk_bytes))
        assert status[0] == 0 and undecided[0] == 0, name
        np.testing.assert_array_equal(coef, host_coef[name], err_msg=name)


@pytest.mark.parametrize('chunk_bytes', [MIN, 64])
def test_one_interleaved_batch_twice(files, host_coef, gpu_device, chunk_bytes):
    bufs = list(files.values())
    rounds = _rounds(bufs, chunk_bytes)
    t, ch, coef, status, undecided = _guarded(bufs, gpu_device, chunk_bytes, rounds)
    assert not status.any() and not undecided.any()
    assert ch.nwg > len(files) and sum(w.count == 64 for w in ch.wgs) >= 3      # chains that cross workgroups
    for name, sc in zip(files, t.scans):
        np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], host_coef[name], err_msg=name)
    again = _guarded(bufs, gpu_device, chunk_bytes, rounds)
    assert again[2].tobytes() == coef.tobytes() and not again[3].any() and not again[4].any()


def test_a_chain_across_workgroups_on_its_own(files, host_coef, gpu_device):
    """One segment of more than 64 chunks, and one of more than 128: the exit of a workgroup's last chunk is the entry
    of the next workgroup's first."""
    name = next(n for n, b in files.items() if '_rst' not in n and len(b) > 1200 and 'noise' in n)
    buf = files[name]
    t = image_io.ScanTables([buf])
    n = t.segs[0].end - t.segs[0].begin
    assert t.nseg == 1
    for cb in (max(MIN, n // 65), MIN):
        t, ch, coef, status, undecided = _guarded([buf], gpu_device, cb, _rounds([buf], cb))
        assert ch.nchunk > (64 if cb != MIN else 128) and ch.nwg == -(-ch.nchunk // 64)
        assert status[0] == 0 and undecided[0] == 0
        np.testing.assert_array_equal(coef, host_coef[name])
    # one round short of what the chain needs: the kernels say so, and nothing else
    cb = max(MIN, n // 65)
    need = _rounds([buf], cb)
    if need > 0:
        t, ch, coef, status, undecided = _guarded([buf], gpu_device, cb, need - 1)
        assert status[0] == 0 and undecided[0] != 0


@pytest.mark.parametrize('chunk_bytes', [MIN, 64, None])
def test_imdecode_equals_the_host_path_in_every_pixel(files, host_pixels, gpu_device, chunk_bytes):
    bufs = list(files.values())
    got = pkg.imdecode(bufs, device=gpu_device, entropy='device_sync', chunk_bytes=chunk_bytes)
    for name, img, want in zip(files, got, host_pixels):
        assert img.dtype == torch.uint8 and img.device == gpu_device
        np.testing.assert_array_equal(img.cpu().numpy(), want, err_msg=name)
    for i, (name, buf) in enumerate(files.items()):      # every file alone
        img = pkg.imdecode(buf, device=gpu_device, entropy='device_sync', chunk_bytes=chunk_bytes)
        np.testing.assert_array_equal(img.cpu().numpy(), host_pixels[i], err_msg=name)


def test_damaged_files_raise_as_the_device_mode_does(files, damaged, gpu_device):
    names = ('72x80_420_grad_q90_rst1', '9x7_420_grad_q90', NOISE, '48x64_444_noise_q90')
    good = [files[n] for n in names]
    assert sorted(damaged) == ['cut_last', 'cut_mid', 'inserted', 'removed', 'swapped']
    for bad in damaged:
        bufs = good[:2] + [damaged[bad]] + good[2:]
        with pytest.raises(ValueError) as want:
            pkg.imdecode(bufs, device=gpu_device, entropy='device')
        for cb in (MIN, 64):
            with pytest.raises(ValueError) as got:
                pkg.imdecode(bufs, device=gpu_device, entropy='device_sync', chunk_bytes=cb)
            assert str(got.value) == str(want.value) and 'image 2' in str(got.value), bad


def test_a_damaged_file_in_a_batch_leaves_the_other_images_right(files, damaged, host_pixels, gpu_device):
    names = list(files)
    pick = [names.index(n) for n in ('72x80_420_grad_q90_rst1', '9x7_420_grad_q90', NOISE, '48x64_444_noise_q90')]
    for bad in ('inserted', 'cut_last'):      # accepted by the table pass, found by the bits
        bufs = [files[names[i]] for i in pick[:2]] + [damaged[bad]] + [files[names[i]] for i in pick[2:]]
        t = image_io.ScanTables(bufs)
        with pytest.raises(ValueError, match='image 2'):
            image_io.decode_into(bufs, 'bgr', gpu_device, entropy='device_sync', chunk_bytes=16)
        # the pixels are written before the error is raised: into the caller's buffer they can be looked at
        place, off = [], 0
        for f in t.infos:
            place.append((off, 3 * f.width))
            off += 3 * f.width * f.height
        out = torch.zeros(off, dtype=torch.uint8, device=gpu_device)
        with pytest.raises(ValueError, match='image 2'):
            image_io.decode_into(bufs, 'bgr', gpu_device, out=out, placement=place, entropy='device_sync', chunk_bytes=16)
        flat = out.cpu().numpy()
        for j, i in zip((0, 1, 3, 4), pick):
            f = t.infos[j]
            got = flat[place[j][0]:place[j][0] + 3 * f.width * f.height].reshape(f.height, f.width, 3)
            np.testing.assert_array_equal(got, host_pixels[i], err_msg=f'{bad}: {names[i]}')


def test_without_rounds_the_second_decode_alone_gives_the_pixels(files, host_pixels, gpu_device):
    bufs = list(files.values())
    t, ch, coef, status, undecided = _guarded(bufs, gpu_device, 16, 0)
    assert undecided.astype(bool).sum() > len(files) // 2 and not status.any()      # most chains cannot close
    got = pkg.imdecode(bufs, device=gpu_device, entropy='device_sync', chunk_bytes=16, max_rounds=0)
    for name, img, want in zip(files, got, host_pixels):
        np.testing.assert_array_equal(img.cpu().numpy(), want, err_msg=name)


def test_load_image_from_file_takes_the_mode(files, host_pixels, gpu_device, tmp_path):
    name = NOISE
    (tmp_path / 'a.jpg').write_bytes(files[name])
    res = pkg.LoadImageFromFile(entropy='device_sync', chunk_bytes=32, max_rounds=4)(
        dict(img_prefix=str(tmp_path), img_info=dict(filename='a.jpg')))
    np.testing.assert_array_equal(res['img'].cpu().numpy(), host_pixels[list(files).index(name)])
    assert pkg.set_default_entropy('device_sync') == 'host'
    try:
        img = pkg.imread(str(tmp_path / 'a.jpg'), device=gpu_device)
    finally:
        pkg.set_default_entropy('host')
    np.testing.assert_array_equal(img.cpu().numpy(), host_pixels[list(files).index(name)])


def test_bad_tables_are_refused_before_the_launch(files, host_coef, gpu_device):
    buf = files[NOISE]
    n = host_coef[NOISE].size
    cbuf = torch.full((n + 2 * PAD,), GUARD, dtype=torch.int16, device=gpu_device)
    for where, field, val, msg in (('scans', 'coef_off', 64, 'coefficients leave'), ('segs', 'end', 1 << 20, 'leaves the file'),
                                   ('segs', 'mcu_count', 2, 'MCU range')):
        t = image_io.ScanTables([buf])
        setattr(getattr(t, where)[0], field, val)
        with pytest.raises((pkg._lib.Yv4Error, ValueError), match=msg):
            image_io.jpeg_entropy_decode_device_sync([buf], 16, 4, gpu_device, coef=cbuf[PAD:PAD + n], tables=t)
    assert (cbuf.cpu().numpy() == GUARD).all()
