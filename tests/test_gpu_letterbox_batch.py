"""``yv4_letterbox_u8_batch`` / ``FusedTestPipeline(batched=True)``: a whole test batch -- every augmentation of every
image, the collate's zero padding included -- in one launch, against the per-image path (``batched=False``: one
``yv4_letterbox_u8`` launch an image into a zeroed batch), bytes equal; one parametrisation also against
oracle/preprocess_oracle.py.  Each case asserts the geometric property it exists for, so that a change of the sizes
cannot silently drop it.  The entry point itself is driven through the C ABI with a destination pre-filled with a NaN
bit pattern between two guards: every element of every slot is written, nothing else is."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from oracle import preprocess_oracle as P

pytestmark = pytest.mark.gpu

NORM = dict(mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375))
PATTERN = 0x7FC12345          # a quiet NaN no arithmetic of the kernel produces
GUARD = 64


def _img(shape, seed=0):
    return np.random.default_rng(seed * 1000 + shape[0] * 7 + shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)


def _same_meta(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == 'img_norm_cfg':
            assert all(np.array_equal(a[k][j], b[k][j]) for j in ('mean', 'std', 'to_rgb'))
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


def _both(images, **kw):
    """The per-image and the batched pipeline over ``images`` -> ``(batches, metas)`` of the batched one, per
    augmentation, after the comparison: shapes, bytes and metas equal."""
    one, bat = pkg.FusedTestPipeline(**kw), pkg.FusedTestPipeline(batched=True, **kw)
    want, got = one(images), bat(images)
    if one.num_augs == 1:
        want, got = ([want[0]], [want[1]]), ([got[0]], [got[1]])
    assert len(got[0]) == len(want[0]) == one.num_augs
    for bw, bg, mw, mg in zip(want[0], got[0], want[1], got[1]):
        assert bg.dtype == torch.float32 and bg.is_cuda and tuple(bg.shape) == tuple(bw.shape)
        assert bg.cpu().numpy().tobytes() == bw.cpu().numpy().tobytes()
        assert len(mg) == len(mw) == len(images)
        for a, b in zip(mw, mg):
            _same_meta(a, b)
    return got


@pytest.mark.parametrize('scale', [(64, 64), (96, 64)])
@pytest.mark.parametrize('shape', [(1, 7), (32, 32), (97, 1024), (640, 427)])
def test_one_slot_equals_the_per_image_path_and_the_restatement(shape, scale):
    img = _img(shape)
    (batch,), (metas,) = _both([img], img_scale=scale)
    want, meta = P.pipeline(img, scale=scale)
    assert batch.shape[0] == 1 and np.array_equal(batch[0].cpu().numpy(), want)
    assert metas[0]['pad_shape'] == meta['pad_shape'] and metas[0]['img_shape'] == meta['img_shape']


def test_a_group_of_four_straddles_the_resized_and_the_padded_edge():
    """``new_w % 4`` of 1, 2 and 3 under ``size_divisor=32``: the 16-byte form, the predicates per pixel."""
    imgs = [_img((64, 61)), _img((64, 62)), _img((64, 63)), _img((29, 64))]
    (batch,), (metas,) = _both(imgs, img_scale=(64, 64), **NORM)
    assert [m['img_shape'][1] % 4 for m in metas[:3]] == [1, 2, 3] and batch.shape[3] % 4 == 0
    assert metas[3]['pad_shape'][0] == 32 < batch.shape[2]       # and a row range that is all collate padding


def test_ragged_batch_pads_to_the_canvas_with_zeros():
    """A landscape, a portrait and a square image: the square one's padded extent is smaller than the canvas both ways."""
    imgs = [_img((64, 96)), _img((96, 64)), _img((40, 40))]
    (batch,), (metas,) = _both(imgs, img_scale=(96, 64), pad_val=114, **NORM)
    H, W = batch.shape[2:]
    assert (H, W) == (96, 96) and metas[0]['pad_shape'] == (64, 96, 3) and metas[1]['pad_shape'] == (96, 64, 3)
    hp, wp = metas[2]['pad_shape'][:2]
    assert hp < H and wp < W
    got = batch[2].cpu().numpy()
    assert not got[:, hp:, :].any() and not got[:, :, wp:].any() and got[:, :hp, :wp].all()


def test_size_divisor_one_takes_the_scalar_form():
    imgs = [_img((64, 61)), _img((64, 50)), _img((64, 33))]
    (batch,), (metas,) = _both(imgs, img_scale=(64, 64), size_divisor=1, **NORM)
    assert tuple(batch.shape) == (3, 3, 64, 61) and batch.shape[3] % 4 != 0             # a width no 16-byte store fits
    assert metas[1]['pad_shape'] == (64, 50, 3) and metas[2]['pad_shape'] == (64, 33, 3)      # ragged: zeros to 61


def test_no_pad_transform_at_all():
    block = [dict(type='LoadImageFromFile'),
             dict(type='MultiScaleFlipAug', img_scale=(64, 64), flip=False,
                  transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                              dict(type='Normalize', to_rgb=True, **NORM), dict(type='ImageToTensor', keys=['img']),
                              dict(type='Collect', keys=['img'])])]
    one = pkg.FusedTestPipeline.from_config(block)
    bat = pkg.FusedTestPipeline.from_config(block, batched=True)
    assert bat.batched and not one.batched and bat.size_divisor == 1
    imgs = [_img((64, 45)), _img((33, 64))]
    (bw, mw), (bg, mg) = one(imgs), bat(imgs)
    assert tuple(bg.shape) == (2, 3, 64, 64) and mg[0]['pad_shape'] == (64, 45, 3)      # pad == new: two regions only
    assert bg.cpu().numpy().tobytes() == bw.cpu().numpy().tobytes()
    for a, b in zip(mw, mg):
        _same_meta(a, b)


@pytest.mark.parametrize('pad_val', [0, 114])
@pytest.mark.parametrize('pad_first', [True, False])
def test_pad_value_before_and_after_normalize(pad_first, pad_val):
    imgs = [_img((64, 37)), _img((21, 64))]
    (batch,), (metas,) = _both(imgs, img_scale=(64, 64), pad_val=pad_val, pad_before_normalize=pad_first, **NORM)
    border = batch[0, :, 0, 63].cpu().numpy()             # inside pad_w = 64, outside new_w = 37
    assert metas[0]['img_shape'][1] == 37
    mean, std = np.float32(NORM['mean']), np.float32(NORM['std'])
    want = (np.float32(pad_val) - mean) * (1.0 / std.astype(np.float64)).astype(np.float32) if pad_first \
        else np.full(3, pad_val, np.float32)
    assert np.array_equal(border, want)


@pytest.mark.parametrize('to_rgb', [True, False])
def test_channel_order(to_rgb):
    img = _img((50, 64))
    (batch,), _ = _both([img], img_scale=(64, 64), to_rgb=to_rgb, **NORM)
    want, _ = P.pipeline(img, scale=(64, 64), to_rgb=to_rgb, **NORM)
    assert np.array_equal(batch[0].cpu().numpy(), want)


def test_every_flip_on_odd_extents():
    img = _img((63, 45))
    dirs = ['horizontal', 'vertical', 'diagonal']
    batches, metas = _both([img, _img((30, 63))], img_scale=(63, 63), flip=True, flip_direction=dirs, **NORM)
    assert metas[0][0]['img_shape'] == (63, 45, 3)                       # odd both ways: the mirror has a fixed column
    assert [m[0]['flip_direction'] for m in metas] == [None] + dirs and [m[0]['flip'] for m in metas] == [False] + [True] * 3
    plain = batches[0][0, :, :63, :45]
    assert torch.equal(batches[1][0, :, :63, :45], plain.flip(2)) and torch.equal(batches[2][0, :, :63, :45], plain.flip(1))
    assert torch.equal(batches[3][0, :, :63, :45], plain.flip(1).flip(2))


def test_two_scales_three_flips_three_images_in_one_launch():
    imgs = [_img((48, 64)), _img((80, 33)), _img((37, 37))]
    batches, metas = _both(imgs, img_scale=[(64, 64), (96, 64)], flip=True, flip_direction=['horizontal', 'vertical'],
                           **NORM)
    assert len(batches) == 6 and len({tuple(b.shape[2:]) for b in batches}) == 2      # two canvases in one table
    store = {b.untyped_storage().data_ptr() for b in batches}
    assert len(store) == 1                                                             # views of one allocation
    assert all(b.data_ptr() % 16 == 0 for b in batches)


def test_a_source_with_a_row_pitch_is_read_where_it_lies(gpu_device):
    canvas = torch.from_numpy(_img((50, 120))).to(gpu_device)
    view = canvas[:, 10:90, :]
    assert not view.is_contiguous() and view.stride(0) == 360 > 3 * view.shape[1] and view.data_ptr() != canvas.data_ptr()
    (batch,), _ = _both([view], img_scale=(64, 64), **NORM)
    want, _ = P.pipeline(np.ascontiguousarray(view.cpu().numpy()), scale=(64, 64), **NORM)
    assert np.array_equal(batch[0].cpu().numpy(), want)


def test_numpy_and_device_inputs_mixed(gpu_device):
    a, b, c = _img((40, 64)), _img((64, 51)), _img((33, 47))
    imgs = [a, torch.from_numpy(b).to(gpu_device), c[:, ::-1], torch.from_numpy(c).to(gpu_device).transpose(0, 1)]
    assert not imgs[2].flags.c_contiguous and not imgs[3].is_contiguous()
    (batch,), _ = _both(imgs, img_scale=(64, 64))
    assert batch.shape[0] == 4


# ---- the entry point itself ------------------------------------------------------------------------------------------

def _slot(src, h, w, new, pad, canvas, flip=0, pitch=None):
    return dict(src=src, h=h, w=w, pitch=3 * w if pitch is None else pitch, new=new, pad=pad, canvas=canvas, flip=flip)


def _call(slots, dev, offs=None, total=None, mean=(1.5, 2.5, 3.5), std=(2.0, 4.0, 8.0), to_rgb=1, pad_val=114, pad_first=1,
          edit=None):
    """``yv4_letterbox_u8_batch`` over ``slots`` into a pattern-filled buffer between two guards -> ``(status, the
    buffer's bits on the host, the slots' offsets)``.  ``edit(table)`` changes the table after it is filled."""
    L = _lib.lib()
    n = len(slots)
    if offs is None:
        offs, end = [], 0
        for s in slots:
            offs.append(end)
            end += 3 * s['canvas'][0] * s['canvas'][1]
        total = end if total is None else total
    table = (_lib.LetterboxSlot * n)()
    for t, s, off in zip(table, slots, offs):
        t.src = s['src'].data_ptr() if s['src'] is not None else None
        t.src_h, t.src_w, t.src_pitch = s['h'], s['w'], s['pitch']
        (t.new_h, t.new_w), (t.pad_h, t.pad_w), (t.H, t.W) = s['new'], s['pad'], s['canvas']
        t.inv_sx, t.inv_sy = 1.0 / (t.new_w / t.src_w), 1.0 / (t.new_h / t.src_h)
        t.flip, t.dst_off = s['flip'], off
    if edit is not None:
        edit(table)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    buf = torch.full((GUARD + total + GUARD,), PATTERN, dtype=torch.int32, device=dev)
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    status = L.yv4_letterbox_u8_batch(table, table_dev.data_ptr(), n, buf.data_ptr() + 4 * GUARD, total,
                                      mean.ctypes.data_as(C.c_void_p), std.ctypes.data_as(C.c_void_p), to_rgb, pad_val,
                                      pad_first, None)
    torch.cuda.synchronize(dev)
    return status, buf.cpu().numpy(), offs


def _per_image(s, dev, mean=(1.5, 2.5, 3.5), std=(2.0, 4.0, 8.0), to_rgb=1, pad_val=114, pad_first=1):
    """The slot by ``yv4_letterbox_u8_flip`` into its padded extent, placed in a zeroed canvas: what collate makes of it."""
    (hp, wp), (H, W) = s['pad'], s['canvas']
    tmp = torch.empty((3, hp, wp), dtype=torch.float32, device=dev)
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    _lib.check(_lib.lib().yv4_letterbox_u8_flip(
        s['src'].data_ptr(), s['h'], s['w'], s['pitch'], tmp.data_ptr(), hp, wp, hp * wp, s['new'][0], s['new'][1],
        mean.ctypes.data_as(C.c_void_p), std.ctypes.data_as(C.c_void_p), to_rgb, pad_val, pad_first, s['flip'], None),
        'yv4_letterbox_u8_flip')
    out = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    out[:, :hp, :wp] = tmp
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@pytest.fixture(scope='module')
def sources(gpu_device):
    return {s: torch.from_numpy(_img(s, seed=1)).to(gpu_device) for s in ((40, 56), (23, 31), (9, 5))}


def _check_written(slots, bits, offs, dev):
    total = len(bits) - 2 * GUARD
    assert (bits[:GUARD] == PATTERN).all() and (bits[GUARD + total:] == PATTERN).all()           # both guards intact
    for s, off in zip(slots, offs):
        n = 3 * s['canvas'][0] * s['canvas'][1]
        got = bits[GUARD + off:GUARD + off + n]
        assert not (got == PATTERN).any()                                                         # every element written
        assert got.tobytes() == _per_image(s, dev).tobytes()


def test_every_element_of_every_slot_is_written_and_nothing_else(sources, gpu_device):
    """A slot that fills its canvas beside one whose padded extent is smaller both ways, a third on another canvas whose
    width is no multiple of 4 (the scalar form, and it leaves the next slot's base unaligned), flips, in one launch."""
    a, b, c = sources[(40, 56)], sources[(23, 31)], sources[(9, 5)]
    slots = [_slot(a, 40, 56, (64, 90), (64, 96), (64, 96)),
             _slot(b, 23, 31, (21, 29), (32, 32), (64, 96), flip=3),
             _slot(c, 9, 5, (27, 15), (27, 15), (31, 17), flip=1),
             _slot(b, 23, 31, (47, 63), (48, 64), (48, 64), flip=2)]
    assert slots[1]['pad'][0] < slots[1]['canvas'][0] and slots[1]['pad'][1] < slots[1]['canvas'][1]
    status, bits, offs = _call(slots, gpu_device)
    assert status == 0, _lib.lib().yv4_last_error()
    assert offs[3] % 4 != 0 and slots[3]['canvas'][1] % 4 == 0           # 16-byte width, unaligned base: scalar form
    _check_written(slots, bits, offs, gpu_device)


def test_one_slot_alone_and_padded_offsets(sources, gpu_device):
    a = sources[(40, 56)]
    one = [_slot(a, 40, 56, (46, 64), (64, 64), (64, 64))]
    status, bits, offs = _call(one, gpu_device)
    assert status == 0
    _check_written(one, bits, offs, gpu_device)
    # slots apart from one another: the floats between them are not touched either
    two = one + [_slot(a, 40, 56, (20, 28), (32, 32), (32, 32))]
    status, bits, offs = _call(two, gpu_device, offs=[8, 3 * 64 * 64 + 40], total=3 * 64 * 64 + 40 + 3 * 32 * 32 + 4)
    assert status == 0
    _check_written(two, bits, offs, gpu_device)
    body = bits[GUARD:-GUARD]
    assert (body[:8] == PATTERN).all() and (body[8 + 3 * 64 * 64:offs[1]] == PATTERN).all() and (body[-4:] == PATTERN).all()


def test_bad_tables_are_refused_before_any_launch(sources, gpu_device):
    a = sources[(40, 56)]
    good = [_slot(a, 40, 56, (46, 64), (64, 64), (64, 64)), _slot(a, 40, 56, (20, 28), (32, 32), (64, 64))]

    def field(k, name, value):
        def edit(table):
            setattr(table[k], name, value)
        return edit
    n = 2 * 3 * 64 * 64
    cases = {
        'pad_w > W': dict(edit=field(1, 'pad_w', 65)),
        'pad_h > H': dict(edit=field(1, 'pad_h', 65)),
        'beyond the destination': dict(total=n - 1),
        'offset beyond the destination': dict(edit=field(1, 'dst_off', 3 * 64 * 64 + 1)),
        'negative offset': dict(edit=field(0, 'dst_off', -1)),
        'bad flip code': dict(edit=field(0, 'flip', 4)),
        'null source': dict(edit=field(1, 'src', None)),
        'pitch below a row': dict(edit=field(0, 'src_pitch', 3 * 56 - 1)),
        'resized beyond padded': dict(edit=field(1, 'new_w', 33)),
        'ratio not of the sizes': dict(edit=field(0, 'inv_sx', 0.5)),
    }
    for name, kw in cases.items():
        status, bits, _ = _call(good, gpu_device, **kw)
        assert status != 0, name
        assert _lib.lib().yv4_last_error().startswith(b'letterbox_batch'), name
        assert (bits == PATTERN).all(), name                                   # nothing was launched
    status, bits, offs = _call(good, gpu_device)                               # and the table itself is fine
    assert status == 0
    _check_written(good, bits, offs, gpu_device)
