"""The one-pass COCO error analysis on the MI355X against the literal restatement of the reference's tool
(tests/_coco_error_ref.py: 1 + 2 K runs of the numpy COCOeval on relabelled annotation files).  Every comparison is exact
equality of ``ps``, the gt counts and the per-walk matched / ignored bits.  That is derived, not measured: every device
operation is a single IEEE float64 operation (or an integer one) in the restatement's order, compiled without
contraction; the means run on the host in both."""
import pickle

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import coco_error as CEA
import _cocoeval_ref as R
import _coco_error_ref as E

pytestmark = pytest.mark.gpu


def assert_equal(res, ref):
    bits = res.det_bits()
    for key in ('index', 'problem', 'rank', 'matched', 'ignored'):
        assert bits[key].shape == ref['bits'][key].shape, key
        np.testing.assert_array_equal(bits[key], ref['bits'][key], err_msg=key)
    np.testing.assert_array_equal(res.counts, ref['counts'])
    assert res.ps.dtype == np.float64 and res.ps.shape == ref['ps'].shape
    np.testing.assert_array_equal(res.ps, ref['ps'])
    assert res.cat_ids == list(ref['cat_ids'])
    np.testing.assert_array_equal(res.aps(), E.aps(ref['ps']))
    for k in range(len(res.cat_ids)):
        np.testing.assert_array_equal(res.aps(k), E.aps(ref['ps'], k))


def check(ds, flat, cat_ids, img_ids, **kw):
    ref = E.error_analysis(ds, *flat, cat_ids, img_ids, **kw)
    for (which, k), c in ref['counts_run'].items():                      # npig is the same in all three runs
        np.testing.assert_array_equal(c, ref['counts'][k])
    res = pkg.error_analysis(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids, **kw)
    assert_equal(res, ref)
    return res, ref


@pytest.fixture(scope='module')
def seeded():
    ds, flat, cat_ids, img_ids = R.seeded_dataset()
    return E.with_supercategories(ds), flat, cat_ids, img_ids


@pytest.fixture(scope='module')
def confusion():
    return E.confusion_dataset()


@pytest.mark.parametrize('areas', [None, (400, 4096, 250000)], ids=['default', 'custom'])
def test_hand_case(gpu_device, areas):
    ds, flat, cat_ids, img_ids = E.hand_case()
    res, _ = check(ds, flat, cat_ids, img_ids, areas=areas)
    if areas is None:
        want = [0, 0, 0.25, 1.0 / (2.0 + 1.0 + np.spacing(1)), 1.0 / (1.0 + 1.0 + np.spacing(1)), 1, 1]
        np.testing.assert_array_equal(res.aps(0)[:, 0], [np.full(101, w).mean() for w in want])


@pytest.mark.parametrize('areas', [None, (576, 4096, 40000)], ids=['default', 'custom'])
def test_seeded_dataset(gpu_device, seeded, areas):
    """R.seeded_dataset() (48 images, 5 categories in 2 supercategories, a problem of 1 003 detections cut at 100)."""
    res, ref = check(*seeded, areas=areas)
    ps = ref['ps']
    assert sum((ps[3, :, k] != ps[2, :, k]).any() for k in range(5)) >= 2
    assert sum((ps[4, :, k] != ps[3, :, k]).any() for k in range(5)) >= 3


def test_confusion_dataset(gpu_device, confusion):
    ds, flat, cat_ids, img_ids = confusion
    ev = E.events(ds, *flat, cat_ids, img_ids)
    for name, n in ev.items():                                           # conditions on the input
        assert n > 0, (name, ev)
    check(ds, flat, cat_ids, img_ids)


def test_sixty_eight_walks_take_two_lane_groups(gpu_device):
    """T = 15, A = 4: (T + 2) * A = 68 walks."""
    ds, flat, cat_ids, img_ids = E.confusion_dataset(seed=1, n_img=6)
    thrs = [0.05 * i for i in range(19, 4, -1)]
    assert len(thrs) == 15
    res, _ = check(ds, flat, cat_ids, img_ids, iou_thrs=thrs)
    assert res.ps.shape[0] == 19


def _edge_dataset(D, G, seed):
    """One image, categories 1 and 2 of one supercategory and 3 of another: G gts over the three (a tenth of them crowd),
    D detections of category 1 of which min(D, G) sit near a gt of any category, and three detections of category 2."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 50, (G, 2)) * 8.0
    wh = rng.integers(2, 20, (G, 2)) * 8.0
    gt = np.concatenate([xy, wh], 1)
    cats = rng.integers(1, 4, G)
    anns = [R._ann(g + 1, 1, int(cats[g]), [float(v) for v in gt[g]], iscrowd=int(rng.integers(0, 10) == 0))
            for g in range(G)]
    d = np.concatenate([rng.integers(0, 50, (D + 3, 2)) * 8.0, rng.integers(2, 20, (D + 3, 2)) * 8.0], 1)
    n = min(D, G)
    d[:n] = gt[rng.permutation(G)[:n]]
    d[:n:2, 2] /= 2
    d[1:n:4, 0] += 8
    s = rng.integers(1, 65, D + 3) / 64.0
    rows = [(0, 0 if j < D else 1, b[0], b[1], b[0] + b[2], b[1] + b[3], sc) for j, (b, sc) in enumerate(zip(d, s))]
    ds = R._dataset([1], [1, 2, 3], anns)
    for c, sup in zip(ds['categories'], 'xxy'):
        c['supercategory'] = sup
    return ds, R._flat(rows), [1, 2, 3], [1]


@pytest.mark.parametrize('G', [31, 32, 33, 64, 65])
def test_matched_bit_words(gpu_device, G):
    res, _ = check(*_edge_dataset(5, G, G))
    assert res._state['workspace'] == 0


@pytest.mark.parametrize('D', [100, 101])
def test_the_cut_at_max_det(gpu_device, D):
    res, ref = check(*_edge_dataset(D, 4, D))
    assert (ref['bits']['problem'] == 0).sum() == 100


PAIRS, GTS = pkg._lib.COCO_ERROR_LDS_PAIRS, pkg._lib.COCO_ERROR_LDS_GTS


@pytest.mark.parametrize('D,G', [(32, 32), (25, 41), (32, 64), (25, 82), (95, 97), (96, 96), (20, 461), (97, 96), (2, GTS),
                                 (2, GTS + 1)])
def test_lds_classes_and_the_workspace(gpu_device, D, G):
    """Around the small LDS class (2 048 doubles, and two smaller blocks), around the exported capacity (9 215 and 9 216
    doubles stay in LDS, 9 220 and 9 312 take the workspace) and around the gt capacity.  The workspace is sized by the
    sizing call."""
    assert (PAIRS, GTS) == (9216, 512)
    res, _ = check(*_edge_dataset(D, G, D * G))
    beyond = D * G > PAIRS or G > GTS
    # the problem of category 1 (D detections) and of category 2 (3): block + 64 lanes' matched bits, one lane group
    want = (D * G + (G + 31) // 32 * 32) * beyond + (3 * G + (G + 31) // 32 * 32) * (G > GTS)
    assert res._state['workspace'] == want


def _as_list_form(flat, n_img, n_cls):
    dets, labels, img_index = flat
    return [[dets[(img_index == i) & (labels == c)] for c in range(n_cls)] for i in range(n_img)]


def test_result_forms_and_repeatability(gpu_device, seeded, tmp_path):
    ds, flat, cat_ids, img_ids = seeded
    results = _as_list_form(flat, len(img_ids), len(cat_ids))
    flat_np = pkg.flatten_results(results)
    flat_gpu = tuple(torch.from_numpy(a).to(gpu_device) for a in flat_np)
    dataset = pkg.CocoBBoxDataset(pkg.CocoGt(ds))
    assert dataset.cat_ids == cat_ids and dataset.img_ids == img_ids
    pkl = tmp_path / 'results.pkl'
    pkl.write_bytes(pickle.dumps(results))
    js = dataset.results2json(flat_np, str(tmp_path / 'results'))['bbox']
    runs = [dataset.error_analysis(r) for r in (results, flat_np, flat_gpu, flat_gpu, str(pkl), js)]
    assert_equal(runs[0], E.error_analysis(ds, *flat_np, cat_ids, img_ids))
    b0 = runs[0].det_bits()
    for r in runs[1:]:
        assert r.ps.tobytes() == runs[0].ps.tobytes() and r.counts.tobytes() == runs[0].counts.tobytes()
        b = r.det_bits()
        for key in b0:
            assert b[key].tobytes() == b0[key].tobytes(), key


def test_literal_form_through_the_public_api(gpu_device, seeded):
    """A second, independent oracle: per category two ``pkg.COCOeval`` runs on relabelled ``CocoGt``s, as the reference
    does, stacked -- equal to the one-pass result bit for bit at K = 5."""
    ds, flat, cat_ids, img_ids = seeded
    dets, labels, img_index = flat

    def run(gt, sel, thrs):
        ev = pkg.COCOeval(pkg.CocoGt(gt), (dets[sel], labels[sel], img_index[sel]), 'bbox', cat_ids=cat_ids, img_ids=img_ids)
        ev.params.maxDets = [100]
        ev.params.iouThrs = np.asarray(thrs, dtype=np.float64)
        ev.evaluate()
        ev.accumulate()
        return ev.eval['precision']
    ps = run(ds, np.arange(len(dets)), [0.75, 0.5, 0.1])
    ps = np.vstack([ps, np.zeros((4, *ps.shape[1:]))])
    cat_sorted = sorted(cat_ids)
    assert len(cat_sorted) == 5
    for k, c in enumerate(cat_sorted):
        sel = np.flatnonzero(labels == cat_ids.index(c))
        ps[3, :, k] = run(E.relabelled(ds, c, 'sim'), sel, [0.1])[0, :, k]
        ps[4, :, k] = run(E.relabelled(ds, c, 'oth'), sel, [0.1])[0, :, k]
    ps[ps == -1] = 0
    ps[5] = ps[4] > 0
    ps[6] = 1.0
    res = pkg.error_analysis(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids)
    assert res.ps.tobytes() == ps.tobytes()


def test_empty_results_and_timing(gpu_device, confusion):
    ds, flat, cat_ids, img_ids = confusion
    none = (np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    res, _ = check(ds, none, cat_ids, img_ids)
    assert (res.ps[:5] == 0).all() and (res.ps[6] == 1).all()
    # timing=True fills every phase and changes nothing
    timed = pkg.error_analysis(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids, timing=True)
    plain = pkg.error_analysis(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids)
    assert timed.ps.tobytes() == plain.ps.tobytes() and plain.phases is None
    assert set(CEA.PHASES) | {'ordering_dev', 'matching_dev', 'accumulation_dev'} == set(timed.phases)


def test_the_tool_end_to_end(gpu_device, tmp_path, capsys):
    """tools/coco_error_analysis.py on the hand case from a bbox json: the arrays and tables it writes are the API's."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('coco_error_analysis_tool', os.path.join(root, 'tools', 'coco_error_analysis.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ds, flat, cat_ids, img_ids = E.hand_case()
    ann = tmp_path / 'ann.json'
    ann.write_text(json.dumps(ds))
    js = pkg.CocoBBoxDataset(pkg.CocoGt(ds)).results2json(flat, str(tmp_path / 'res'))['bbox']
    monkey_plt = tool.pyplot
    tool.pyplot = lambda: None                                           # the figures have their own host test
    try:
        tool.main([js, str(tmp_path / 'out'), '--ann', str(ann), '--areas', '400', '4096', '250000'])
    finally:
        tool.pyplot = monkey_plt
    out = capsys.readouterr().out
    assert 'the figures were skipped' in out and 'bbox-allclass' in out
    want = pkg.error_analysis(pkg.CocoGt(ds), flat, cat_ids=cat_ids, img_ids=img_ids, areas=(400, 4096, 250000))
    z = np.load(tmp_path / 'out' / 'bbox' / 'error_analysis.npz')
    assert z['ps'].tobytes() == want.ps.tobytes() and z['counts'].tobytes() == want.counts.tobytes()
    assert list(z['names']) == ['c1', 'c2', 'c3'] and z['area_rng'].tolist() == [[0, 250000], [0, 400], [400, 4096], [4096, 250000]]
    assert want.table() in (tmp_path / 'out' / 'bbox' / 'error_analysis.txt').read_text()
