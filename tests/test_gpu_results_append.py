"""``yv4_results_append`` (csrc/results.hip) through the binding, on hand-built ``dets / labels / count``: the table it
writes must be ``flatten_results([bbox2result(dets[n, :k], labels[n, :k], C) for n])`` plus the repeated ``img_index``,
compared with ``np.array_equal`` on all three outputs over the WHOLE capacity (rows the call does not own keep their
sentinel).  Then ``DeviceResults`` on top of it: growth, skipped images, the list form."""
import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import _lib
from mmdet_yolov4_amd.coco_eval import flatten_results
from mmdet_yolov4_amd.results import DeviceResults

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _batch(rng, N, M, C, counts, labels=None, few_scores=False):
    """Distinct boxes per row (a moved or swapped row shows), scores from a handful of values when ``few_scores``."""
    dets = rng.uniform(0, 100, (N, M, 5)).astype(np.float32)
    dets[..., 0] = np.arange(N * M, dtype=np.float32).reshape(N, M)            # the row's identity
    dets[..., 4] = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), (N, M)) if few_scores else rng.random((N, M))
    if labels is None:
        labels = rng.integers(0, C, (N, M))
    return dets, np.asarray(labels, np.int32).reshape(N, M), np.asarray(counts, np.int32)


def _expected(dets, labels, count, img_index, C):
    kept = [n for n in range(len(count)) if img_index[n] >= 0]
    lists = [pkg.bbox2result(dets[n, :count[n]], labels[n, :count[n]], C) for n in kept]
    if not lists:
        return np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    d, l, local = flatten_results(lists)
    return d, l, np.asarray(img_index, np.int64)[kept][local]


def _tables(capacity, dev):
    return (torch.full((capacity, 5), SENTINEL, dtype=torch.float32, device=dev),
            torch.full((capacity,), SENTINEL, dtype=torch.int64, device=dev),
            torch.full((capacity,), SENTINEL, dtype=torch.int64, device=dev))


def _append(tables, dets, labels, count, img_index, C, base, dev):
    N, M = labels.shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (dets, labels, count, np.asarray(img_index, np.int64))]
    capacity = tables[0].shape[0]
    rc = _lib.lib().yv4_results_append(*[x.data_ptr() for x in t], N, M, C, base, capacity,
                                       *[x.data_ptr() for x in tables], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _check(tables, base, want, capacity):
    full_d = np.full((capacity, 5), SENTINEL, np.float32)
    full_l = np.full(capacity, SENTINEL, np.int64)
    full_i = np.full(capacity, SENTINEL, np.int64)
    for b, (wd, wl, wi) in zip(base, want):
        full_d[b:b + len(wd)], full_l[b:b + len(wd)], full_i[b:b + len(wd)] = wd, wl, wi
    assert np.array_equal(tables[0].cpu().numpy(), full_d)
    assert np.array_equal(tables[1].cpu().numpy(), full_l)
    assert np.array_equal(tables[2].cpu().numpy(), full_i)


def _one(dev, dets, labels, count, img_index, C, slack=3, base=0):
    want = _expected(dets, labels, count, img_index, C)
    capacity = base + len(want[0]) + slack
    tables = _tables(capacity, dev)
    assert _append(tables, dets, labels, count, img_index, C, base, dev) == 0
    _check(tables, [base], [want], capacity)
    return want


def test_has_the_entry_point():
    assert _lib.has('results_append')


@pytest.mark.parametrize('M', [1, 300, 1000])
@pytest.mark.parametrize('C', [1, 80])
def test_counts_zero_full_one(gpu_device, M, C):
    """N = 3 with counts [0, max_per_img, 1]: an empty image in front, a full one (1000 rows: four passes of the 256
    threads), one row; equal scores inside the classes."""
    rng = np.random.default_rng(100 * M + C)
    dets, labels, count = _batch(rng, 3, M, C, [0, M, 1], few_scores=True)
    want = _one(gpu_device, dets, labels, count, [4, 5, 6], C)
    assert len(want[0]) == M + 1 and want[2].tolist() == [5] * M + [6]
    if C == 1:
        assert np.array_equal(want[0][:M], dets[1])           # one class: the NMS order itself


def test_single_empty_image(gpu_device):
    rng = np.random.default_rng(0)
    dets, labels, count = _batch(rng, 1, 10, 3, [0])
    want = _one(gpu_device, dets, labels, count, [0], 3)
    assert len(want[0]) == 0


def test_descending_labels_move_every_row(gpu_device):
    rng = np.random.default_rng(1)
    M = 300
    lab = np.arange(M - 1, -1, -1)[None]
    dets, labels, count = _batch(rng, 1, M, M, [M], labels=lab)
    want = _one(gpu_device, dets, labels, count, [9], M)
    assert np.array_equal(want[0], dets[0, ::-1]) and want[1].tolist() == list(range(M))


def test_stability_equal_scores_inside_a_class(gpu_device):
    """Rows of one class keep the order NMS left, also where their scores are equal: the identity column ascends
    inside every class."""
    rng = np.random.default_rng(2)
    M, C = 700, 3
    dets, labels, count = _batch(rng, 2, M, C, [M - 1, 513], few_scores=True)
    d, l, i = _one(gpu_device, dets, labels, count, [0, 1], C)
    for img in (0, 1):
        for c in range(C):
            ident = d[(i == img) & (l == c), 0]
            assert len(ident) > 1 and np.all(np.diff(ident) > 0)
    assert len(np.unique(d[:, 4])) == 3


def test_skipped_image_in_the_middle(gpu_device):
    rng = np.random.default_rng(3)
    dets, labels, count = _batch(rng, 4, 20, 5, [7, 20, 0, 13])
    want = _one(gpu_device, dets, labels, count, [10, -1, 12, 3], 5)
    assert len(want[0]) == 20 and sorted(set(want[2].tolist())) == [3, 10]


def test_two_appends_and_exact_capacity(gpu_device):
    """The second append starts at base = the first's total and ends exactly at capacity; nothing before `base` is
    touched by it."""
    rng = np.random.default_rng(4)
    C = 4
    a = _batch(rng, 2, 50, C, [50, 17])
    b = _batch(rng, 3, 30, C, [1, 0, 30])
    wa, wb = _expected(*a, [0, 1], C), _expected(*b, [2, 3, 4], C)
    capacity = len(wa[0]) + len(wb[0])
    tables = _tables(capacity, gpu_device)
    assert _append(tables, *a, [0, 1], C, 0, gpu_device) == 0
    _check(tables, [0], [wa], capacity)
    assert _append(tables, *b, [2, 3, 4], C, len(wa[0]), gpu_device) == 0
    _check(tables, [0, len(wa[0])], [wa, wb], capacity)


def test_rows_beyond_capacity_are_not_written(gpu_device):
    """The host keeps base + total <= capacity; a caller that does not loses rows, never memory that is not its own."""
    rng = np.random.default_rng(5)
    dets, labels, count = _batch(rng, 1, 40, 2, [40])
    want = _expected(dets, labels, count, [0], 2)
    guard = _tables(64, gpu_device)
    view = tuple(t[:30] for t in guard)
    assert _append(view, dets, labels, count, [0], 2, 0, gpu_device) == 0
    _check(guard, [0], [tuple(w[:30] for w in want)], 64)


def test_argument_errors_launch_nothing(gpu_device):
    L = _lib.lib()
    t = _tables(8, gpu_device)
    p = [x.data_ptr() for x in t]
    buf = torch.zeros(8, device=gpu_device)             # never read: every call below returns before a launch
    src = [buf.data_ptr()] * 4
    sp = torch.cuda.current_stream().cuda_stream
    assert L.yv4_results_append(*src, 1, _lib.RESULTS_MAX_PER_IMG + 1, 3, 0, 8, *p, sp) == -2
    assert b'YV4_RESULTS_MAX_PER_IMG' in L.yv4_last_error()
    assert L.yv4_results_append(*src, -1, 4, 3, 0, 8, *p, sp) == -1 and b'negative batch' in L.yv4_last_error()
    for hole in range(7):
        args = src + p
        args[hole] = None
        assert L.yv4_results_append(*args[:4], 1, 4, 3, 0, 8, *args[4:], sp) == -1 and b'null' in L.yv4_last_error()
    assert L.yv4_results_append(*src, 1, 0, 3, 0, 8, *p, sp) == -1
    assert L.yv4_results_append(*src, 1, 4, 0, 0, 8, *p, sp) == -1
    assert L.yv4_results_append(*src, 1, 4, 3, -1, 8, *p, sp) == -1
    assert L.yv4_results_append(*src, 1, 4, 3, 9, 8, *p, sp) == -1
    assert L.yv4_results_append(None, None, None, None, 0, 4, 3, 0, 0, None, None, None, sp) == 0     # an empty batch
    torch.cuda.synchronize()
    _check(t, [0], [(np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))], 8)


def _post(dets, labels, count, dev):
    N, M = labels.shape
    return dict(N=N, max_per_img=M, dets=torch.from_numpy(dets).to(dev), labels=torch.from_numpy(labels).to(dev),
                count=torch.from_numpy(count).to(dev))


def test_device_results_grows_skips_and_takes_lists(gpu_device):
    rng = np.random.default_rng(6)
    C = 6
    table = DeviceResults(C, gpu_device, capacity=16)
    a = _batch(rng, 3, 40, C, [40, 0, 25], few_scores=True)
    b = _batch(rng, 2, 40, C, [40, 40], few_scores=True)
    assert table.append(_post(*a, gpu_device)) == 65 and table.num_images == 3          # default positions 0, 1, 2
    assert table.capacity >= 65
    first = [t.clone() for t in table.tensors()]
    assert table.append(_post(*b, gpu_device), [7, -1], counts=torch.from_numpy(b[2])) == 40   # grows: the old rows survive
    lists = [pkg.bbox2result(a[0][2, :25], a[1][2, :25], C), pkg.bbox2result(a[0][0, :0], a[1][0, :0], C)]
    assert table.append_lists(lists, [9, 10]) == 25 and table.num_images == 7
    d, l, i = (t.cpu().numpy() for t in table.tensors())
    wa, wb, wc = _expected(*a, [0, 1, 2], C), _expected(*b, [7, -1], C), flatten_results(lists)
    assert np.array_equal(d, np.concatenate([wa[0], wb[0], wc[0]]))
    assert np.array_equal(l, np.concatenate([wa[1], wb[1], wc[1]]))
    assert np.array_equal(i, np.concatenate([wa[2], wb[2], np.full(25, 9)]))
    assert all(torch.equal(x, y[:65]) for x, y in zip(first, table.tensors()))
    assert d.dtype == np.float32 and l.dtype == np.int64 and i.dtype == np.int64
    # counts the split path has not resolved, a wrong number of positions, a foreign class count
    bad = _post(*a, gpu_device)
    bad['count'] = torch.tensor([3, -1, 2], dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError, match='split path'):
        table.append(bad)
    with pytest.raises(ValueError, match='positions'):
        table.append(_post(*a, gpu_device), [0, 1])
    with pytest.raises(ValueError, match='class lists'):
        table.append_lists([lists[0][:2]])
    assert table.D == 130
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceResults(C, 'cpu')
