"""The JPEG encoder on the GPU against libjpeg-turbo's files (tests/golden/jpeg_encode.npz): byte for byte, per case and
as one batch, each stage at its seam behind guard bytes, and round through the project's own decoder."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io as io

import _jpeg_enc_data as D
import _jpeg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cases(golden):
    return D.load_cases(golden)


@pytest.fixture(scope='module')
def batch_files(cases, gpu_device):
    """``imencode`` of all cases as one batch, shared by the tests that only read it."""
    names, srcs, jpgs, quals, samps = cases
    return pkg.imencode(srcs, quals, samps, 'rgb', device=gpu_device)


def test_every_case_alone(cases, gpu_device):
    names, srcs, jpgs, quals, samps = cases
    for name, src, jpg, q, s in zip(names, srcs, jpgs, quals, samps):
        got = pkg.imencode(torch.from_numpy(src).to(gpu_device), q, s, 'rgb')
        assert isinstance(got, bytes) and got == jpg, name


def test_batch_equals_the_single_calls(cases, batch_files):
    names, srcs, jpgs, quals, samps = cases
    assert [n for n, a, b in zip(names, batch_files, jpgs) if a != b] == []


def test_bgr_input_equals_rgb_input(cases, batch_files, gpu_device):
    names, srcs, jpgs, quals, samps = cases
    bgr = [torch.from_numpy(np.ascontiguousarray(a[..., ::-1]) if a.ndim == 3 else a).to(gpu_device) for a in srcs]
    assert pkg.imencode(bgr, quals, samps, 'bgr') == batch_files
    assert pkg.imencode(bgr, quals, samps) == batch_files              # 'bgr' is the default, as imread's


def test_two_runs_give_identical_bytes(cases, batch_files, gpu_device):
    names, srcs, jpgs, quals, samps = cases
    assert pkg.imencode(srcs, quals, samps, 'rgb', device=gpu_device) == batch_files


def test_defaults_are_cv2s(cases, gpu_device):
    names, srcs, jpgs, quals, samps = cases
    k = names.index('37x53_420_grad_q95')
    assert pkg.imencode(srcs[k], channel_order='rgb', device=gpu_device) == jpgs[k]


def test_the_long_case_exceeds_one_workgroup_of_the_bit_offset_scan(cases):
    names, srcs, jpgs, quals, samps = cases
    k = names.index('136x264_420_noise_q100')
    et = io.EncodeTable([srcs[k].shape], quals[k], samps[k])
    assert et.table[0].nblocks == 918 > pkg._lib.JPEG_ENC_WG_BLOCKS


def test_each_stage_at_its_seam_behind_guards(cases, gpu_device):
    """The whole batch, every region behind guard bytes and the input at a wider pitch with guard columns: the device
    coefficients equal the host decoder's for libjpeg-turbo's files; the device scan bytes FROM THOSE equal the files';
    no byte outside an image's regions of the coefficient, workspace and output buffers changes."""
    names, srcs, jpgs, quals, samps = cases
    et = io.EncodeTable([a.shape for a in srcs], quals, samps)
    npix, ncoef, nwork, nout = D.spread(et)
    pix = torch.from_numpy(D.place_pixels(et, srcs, npix)).to(gpu_device)
    want = np.full(ncoef, 0x5A5A, np.int16)
    regions = []
    for t, jpg in zip(et.table, jpgs):
        _, c = io.jpeg_entropy_decode(jpg)
        want[t.coef_off:t.coef_off + c.size] = c
        regions.append((2 * int(t.coef_off), 2 * c.size))
    coef = torch.full((ncoef,), 0x5A5A, dtype=torch.int16, device=gpu_device)
    io.encode_stages(et, pix, 'rgb', coef=coef, stages=1)
    got = coef.cpu().numpy()
    for name, t in zip(names, et.table):
        lo, hi = int(t.coef_off), int(t.coef_off + t.nblocks * 64)
        np.testing.assert_array_equal(got[lo:hi], want[lo:hi], err_msg=name)
    D.assert_guards(got.view(np.uint8), regions, 'coefficients')

    coef = torch.from_numpy(want).to(gpu_device)                    # stage 2 from the host decoder's coefficients
    work = torch.full((nwork,), D.GUARD_BYTE, dtype=torch.uint8, device=gpu_device)
    out = torch.full((nout,), D.GUARD_BYTE, dtype=torch.uint8, device=gpu_device)
    _, _, _, sizes = io.encode_stages(et, pix, 'rgb', coef=coef, work=work, out=out, stages=2)
    sizes, out_h, work_h = sizes.cpu().numpy(), out.cpu().numpy(), work.cpu().numpy()
    for n, (name, t, jpg) in enumerate(zip(names, et.table, jpgs)):
        head = et.header(n)
        assert out_h[t.out_off:t.out_off + int(sizes[n])].tobytes() == jpg[len(head):-2], name
    D.assert_guards(out_h, [(int(t.out_off), int(sizes[n])) for n, t in enumerate(et.table)], 'output')
    D.assert_guards(work_h, [(int(t.work_off), et.work_region_bytes(n)) for n, t in enumerate(et.table)], 'workspace')
    np.testing.assert_array_equal(coef.cpu().numpy(), want)


def test_read_back_is_the_size_of_the_files(cases, gpu_device, monkeypatch):
    """What crosses to the host after the N counts is one pinned copy of exactly the scan bytes, not the bound-sized
    output buffer."""
    names, srcs, jpgs, quals, samps = cases
    seen = []
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        if kw.get('pin_memory') and not any(isinstance(s, np.ndarray) for s in srcs_dev):
            seen.append(t.numel())
        return t

    srcs_dev = [torch.from_numpy(a).to(gpu_device) for a in srcs]
    et = io.EncodeTable([a.shape for a in srcs], quals, samps)
    monkeypatch.setattr(torch, 'empty', empty)
    files = pkg.imencode(srcs_dev, quals, samps, 'rgb')
    monkeypatch.undo()
    assert files == jpgs
    scan = sum(len(f) - len(et.header(n)) - 2 for n, f in enumerate(files))
    assert sorted(seen) == sorted([scan, et.table._length_ * 408]) and scan < et.out_bytes


def test_round_trip_through_the_projects_decoder(cases, batch_files, gpu_device):
    imgs = pkg.imdecode(batch_files, device=gpu_device)
    for name, f, img in zip(cases[0], batch_files, imgs):
        np.testing.assert_array_equal(img.cpu().numpy(), R.decode(f), err_msg=name)


def test_decode_into_table_feeds_encode_into(cases, gpu_device):
    """``decode_into``'s ``(out, table)`` is ``encode_into``'s input: no pixel is copied in between."""
    names, srcs, jpgs, quals, samps = cases
    pick = [k for k, s in enumerate(samps) if s != 'gray'][:6]
    out, table = io.decode_into([jpgs[k] for k in pick], 'rgb', gpu_device)
    got = pkg.encode_into(out, table, 90, '420', 'rgb')
    views = io.image_views(out, table)
    assert got == pkg.imencode(views, 90, '420', 'rgb')


def test_imwrite_writes_the_files(cases, tmp_path, gpu_device):
    names, srcs, jpgs, quals, samps = cases
    ks = [names.index('37x53_420_grad_q95'), names.index('48x64_420_grad_q95')]
    paths = [tmp_path / 'sub' / 'a.jpg', tmp_path / 'b.JPEG']
    assert pkg.imwrite([srcs[k] for k in ks], paths, channel_order='rgb') is True
    assert [p.read_bytes() for p in paths] == [jpgs[k] for k in ks]
    with pytest.raises(ValueError, match='quality'):
        pkg.imencode(srcs[ks[0]], quality=0)
    with pytest.raises(ValueError, match='subsampling'):
        pkg.imencode(srcs[ks[0]], subsampling='410')
