"""The COCO error analysis without a GPU: the literal restatement (tests/_coco_error_ref.py) against hand-computed values,
the host table build, the result readers, argument validation through ctypes, the tool's arguments and its outputs."""
import ctypes
import importlib.util
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import coco_error as CEA
import _cocoeval_ref as R
import _coco_error_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.spacing(1)


def _tool():
    spec = importlib.util.spec_from_file_location('coco_error_analysis_tool', os.path.join(ROOT, 'tools', 'coco_error_analysis.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the oracle -------------------------------------------------------------------------------------------------------
def test_oracle_on_the_hand_case():
    """Detections of A in rank order: d1 on B's gt (A's supercategory), d2 on C's gt (the other one), d3 on nothing, d4
    with IoU 0.3 on A's own gt; one gt of A (area 10 000: 'allarea' and 'large').
    base 0.75 / 0.5: four fp                                -> precision 0
    base 0.1:  fp fp fp tp   pr = 1 / (3 + 1 + eps)         -> 0.25 at every recall threshold (the envelope)
    Sim:       ig fp fp tp   pr = 1 / (2 + 1 + eps)
    Oth:       ig ig fp tp   pr = 1 / (1 + 1 + eps)"""
    ds, flat, cat_ids, img_ids = E.hand_case()
    ref = E.error_analysis(ds, *flat, cat_ids, img_ids)
    assert ref['ps'].shape == (7, 101, 3, 4, 1) and ref['cat_ids'] == [1, 2, 3]
    b = ref['bits']
    np.testing.assert_array_equal(b['index'], [0, 1, 2, 3])
    np.testing.assert_array_equal(b['matched'][0].astype(int),
                                  [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1], [1, 1, 0, 1]])
    np.testing.assert_array_equal(b['ignored'][0].astype(int),
                                  [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]])
    want = [0, 0, 1 / (3 + 1 + EPS), 1 / (2 + 1 + EPS), 1 / (1 + 1 + EPS), 1, 1]
    # 'large' [9216, 1e10]: the unmatched d3 (area 2 500) is ignored there, so every walk has one fp less
    large = [0, 0, 1 / (2 + 1 + EPS), 1 / (1 + 1 + EPS), 1 / (0 + 1 + EPS), 1, 1]
    for a, values in ((0, want), (3, large)):
        for t in range(7):
            assert (ref['ps'][t, :, 0, a, 0] == values[t]).all(), (t, a)
    assert (ref['ps'][:6, :, 0, 1:3] == 0).all() and (ref['ps'][6] == 1).all()      # no gt of A is small or medium
    assert (ref['ps'][:6, :, 1:] == 0).all()                                       # B and C: gts, no detections
    np.testing.assert_array_equal(ref['counts'], [[1, 0, 0, 1]] * 3)
    np.testing.assert_array_equal(E.aps(ref['ps'], 0)[:, 0], [np.full(101, w).mean() for w in want])     # makeplot's means
    # "allclass": the mean runs over K too, the zero rows of B and C included (their BG row is 0 as well)
    one_of_three = [np.concatenate([np.full((101, 1), w), np.zeros((101, 2))], 1).mean() for w in want[:6]]
    np.testing.assert_array_equal(E.aps(ref['ps'])[:, 0], one_of_three + [1.0])


def test_oracle_on_the_seeded_set():
    ds, flat, cat_ids, img_ids = R.seeded_dataset()
    ds = E.with_supercategories(ds)
    ref = E.error_analysis(ds, *flat, cat_ids, img_ids)
    for (which, k), c in ref['counts_run'].items():
        np.testing.assert_array_equal(c, ref['counts'][k])
    ps = ref['ps']
    assert sum((ps[3, :, k] != ps[2, :, k]).any() for k in range(5)) == 2
    assert sum((ps[4, :, k] != ps[3, :, k]).any() for k in range(5)) == 3
    assert (ps[4] >= ps[3]).all() and (ps[3] >= ps[2]).all() and ((ps[5] == 0) | (ps[5] == 1)).all()
    # custom areas swap R's constant for the call only
    keep = [list(r) for r in R.AREA_RNG]
    custom = E.error_analysis(ds, *flat, cat_ids, img_ids, areas=(576, 4096, 40000))
    assert R.AREA_RNG == keep and not np.array_equal(custom['counts'], ref['counts'])


def test_the_confusion_set_contains_every_corner():
    ds, flat, cat_ids, img_ids = E.confusion_dataset()
    ev = E.events(ds, *flat, cat_ids, img_ids)
    assert set(ev) == set(E.EVENTS)
    for name, n in ev.items():
        assert n > 0, (name, ev)


# ---- the package's host side ----------------------------------------------------------------------------------------
def _small_gt():
    ds = R._dataset([30, 10, 20], [7, 3, 11, 9],
                    [R._ann(1, 10, 11, (0, 0, 10, 10)), R._ann(2, 30, 7, (0, 0, 20, 20), iscrowd=1),
                     R._ann(3, 10, 42, (5, 5, 10, 10)), R._ann(4, 10, 3, (8, 8, 10, 10)), R._ann(5, 99, 3, (0, 0, 5, 5)),
                     R._ann(6, 30, 9, (1, 1, 2, 2))])
    for c, s in zip(ds['categories'], ('a', 'b', 'a')):                # category 9 has no supercategory
        c['supercategory'] = s
    return ds


def test_cat_group():
    g = pkg.CocoGt(_small_gt()).cat_group()
    assert g == {7: 0, 3: 1, 11: 0, 9: 2}
    assert pkg.CocoGt(E.hand_case()[0]).cat_group() == {1: 0, 2: 0, 3: 1}


def test_image_major_table():
    tab = CEA.tables(pkg.CocoGt(_small_gt()))
    assert (tab['N'], tab['K'], tab['P']) == (3, 4, 12)
    np.testing.assert_array_equal(tab['img_ids'], [10, 20, 30])
    np.testing.assert_array_equal(tab['cat_ids'], [3, 7, 9, 11])
    np.testing.assert_array_equal(tab['gt_img_off'], [0, 3, 3, 5])              # image 99 is not in the file's images
    # image 10 in annotation order: category 11, the unlisted 42 (-1), 3; image 30: 7 (crowd), 9
    np.testing.assert_array_equal(tab['gt_cat'], [3, -1, 0, 1, 2])
    assert tab['gt_cat'].dtype == np.int32 and tab['cat_group'].dtype == np.int32
    np.testing.assert_array_equal(tab['gt_flag'], [0, 0, 0, 3, 0])
    np.testing.assert_array_equal(tab['gt_box'][:, 0], [0, 5, 8, 0, 1])
    np.testing.assert_array_equal(tab['gt_area'], [100, 100, 100, 400, 4])
    np.testing.assert_array_equal(tab['cat_group'], [1, 0, 2, 0])               # K-axis order: 3 'b', 7 'a', 9 alone, 11 'a'
    np.testing.assert_array_equal(tab['kmap'], [1, 0, 3, 2])                    # label -> K position, file order 7 3 11 9
    np.testing.assert_array_equal(tab['imap'], [2, 0, 1])
    # a category the file does not list, named by the caller: a group of its own
    tab = CEA.tables(pkg.CocoGt(_small_gt()), cat_ids=[7, 42, 11], img_ids=[10])
    np.testing.assert_array_equal(tab['cat_ids'], [7, 11, 42])
    assert tab['cat_group'][0] == tab['cat_group'][1] != tab['cat_group'][2]
    np.testing.assert_array_equal(tab['gt_cat'], [1, 2, -1])
    with pytest.raises(ValueError, match='must not be empty'):
        CEA.tables(pkg.CocoGt(_small_gt()), cat_ids=[])


def test_area_ranges():
    np.testing.assert_array_equal(CEA.area_ranges(), pkg.coco_eval.AREA_RNG)
    np.testing.assert_array_equal(CEA.area_ranges((4, 9, 16)), [[0, 16], [0, 4], [4, 9], [9, 16]])
    with pytest.raises(ValueError, match='3 integers'):
        CEA.area_ranges((1, 2))


def test_result_readers(tmp_path):
    ds, flat, cat_ids, img_ids = E.confusion_dataset(n_img=6)
    dets, labels, img_index = flat
    results = [[dets[(img_index == i) & (labels == c)] for c in range(len(cat_ids))] for i in range(len(img_ids))]
    flat_np = pkg.flatten_results(results)
    dataset = pkg.CocoBBoxDataset(pkg.CocoGt(ds))
    js = dataset.results2json(flat_np, str(tmp_path / 'r'))['bbox']
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                  # every row survives the round trip
        got = CEA.load_results(js, cat_ids, img_ids)
    for a, b in zip(got, flat_np):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    pkl = tmp_path / 'r.pkl'
    pkl.write_bytes(pickle.dumps(results))
    for a, b in zip(CEA.load_results(str(pkl), cat_ids, img_ids), flat_np):
        assert a.tobytes() == b.tobytes()
    pkl.write_bytes(pickle.dumps(flat_np))
    assert CEA.load_results(pkl, cat_ids, img_ids)[0].tobytes() == flat_np[0].tobytes()
    with pytest.raises(ValueError, match='.pkl'):
        CEA.load_results(str(tmp_path / 'r.txt'), cat_ids, img_ids)
    # rows that are no float32 rows: counted, evaluated as rounded; unknown ids take no part
    rows = [dict(image_id=img_ids[0], category_id=cat_ids[1], bbox=[0.1, 2.0, 3.0, 4.0], score=0.5),
            dict(image_id=img_ids[1], category_id=cat_ids[0], bbox=[1.0, 2.0, 3.0, 4.0], score=0.25),
            dict(image_id=12345, category_id=cat_ids[0], bbox=[1.0, 2.0, 3.0, 4.0], score=1 / 3),
            dict(image_id=img_ids[2], category_id=4242, bbox=[1.0, 2.0, 3.0, 4.0], score=0.75)]
    (tmp_path / 'odd.json').write_text(json.dumps(rows))
    with pytest.warns(UserWarning, match='2 of 4 json rows'):
        d, lab, img = CEA.load_results(str(tmp_path / 'odd.json'), cat_ids, img_ids)
    np.testing.assert_array_equal(d[1], [1, 2, 4, 6, 0.25])
    np.testing.assert_array_equal(d[0], np.array([0.1, 2.0, 3.1, 6.0, 0.5], np.float32))
    np.testing.assert_array_equal(lab, [1, 0, 0, -1])
    np.testing.assert_array_equal(img, [0, 1, -1, 2])


def test_segm_and_a_missing_entry_point_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="iou_type='segm' is not built"):
        pkg.error_analysis(pkg.CocoGt(_small_gt()), [], iou_type='segm')
    # the two entry points belong to every build: a library without one does not bind, and the error names it
    L = pkg._lib
    assert {'yv4_coco_error_need', 'yv4_coco_error_match'} <= set(L.SIGNATURES)
    assert not any(s.startswith('yv4_coco_error') for ft in L.FEATURES.values() for s in ft.symbols)

    class Fn:
        restype = argtypes = None

        def __call__(self):
            return L.ABI_VERSION
    handle = type('Handle', (), {})()
    for name in L.SIGNATURES:
        if name != 'yv4_coco_error_match':
            setattr(handle, name, Fn())
    with pytest.raises(AttributeError, match='yv4_coco_error_match'):
        L._bind(handle)


def test_the_capacities_are_the_headers():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    for name in ('COCO_ERROR_LDS_PAIRS', 'COCO_ERROR_LDS_GTS'):
        assert int(re.search(rf'\bYV4_{name} = (\d+)', text).group(1)) == getattr(pkg._lib, name)
    # one wave per workgroup: the block, 64 lanes' matched bits and the base fit half of a CU's 160 KiB
    assert 8 * pkg._lib.COCO_ERROR_LDS_PAIRS + 8 * pkg._lib.COCO_ERROR_LDS_GTS + 8 <= 80 * 1024


def test_argument_validation_without_gpu():
    """Bad arguments are refused before the device is touched (no GPU here: anything else would fail differently)."""
    lib = pkg._lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def match(**kw):
        a = dict(det=p, order=p, det_off=p, gt_box=p, gt_area=p, gt_flag=p, gt_cat=p, gt_img_off=p, cat_group=p, P=4, K=2,
                 total_det=1, total_gt=1, max_det=100, iou_thrs=p, T=3, conf_thr=0.1, area_rng=p, A=4, work=None, work_len=0,
                 state=p, flags=p, counts=p, stream=None)
        a.update(kw)
        return lib.yv4_coco_error_match(*a.values())
    E_INVALID = pkg._lib.E_INVALID
    for bad in (dict(det=None), dict(order=None), dict(flags=None), dict(det_off=None), dict(gt_img_off=None),
                dict(cat_group=None), dict(gt_box=None), dict(gt_area=None), dict(gt_flag=None), dict(gt_cat=None),
                dict(iou_thrs=None), dict(area_rng=None), dict(state=None), dict(counts=None), dict(A=65), dict(A=0),
                dict(T=0), dict(K=0), dict(P=0), dict(P=5), dict(max_det=0), dict(total_det=-1), dict(total_gt=-1),
                dict(work_len=8), dict(work_len=-1), dict(T=2 ** 31 - 3, K=2 ** 20, P=2 ** 20), dict(K=2 ** 29, P=2 ** 29)):
        assert match(**bad) == E_INVALID, bad
        assert b'coco_error_match' in lib.yv4_last_error()

    def need(**kw):
        a = dict(det_off=p, gt_img_off=p, P=4, K=2, max_det=100, num_walks=20, need=p, stream=None)
        a.update(kw)
        return lib.yv4_coco_error_need(*a.values())
    for bad in (dict(det_off=None), dict(gt_img_off=None), dict(need=None), dict(P=0), dict(K=0), dict(P=3), dict(max_det=0),
                dict(num_walks=0)):
        assert need(**bad) == E_INVALID, bad


# ---- the tool ---------------------------------------------------------------------------------------------------------
def test_tool_arguments(capsys):
    tool = _tool()
    a = tool.parse_args(['res.json', 'out'])
    assert (a.result, a.out_dir, a.types, a.extraplots, a.areas) == ('res.json', 'out', ['bbox'], False, [1024, 9216, 10 ** 10])
    assert a.ann == 'data/coco/annotations/instances_val2017.json'
    a = tool.parse_args(['r.pkl', 'o', '--ann', 'a.json', '--extraplots', '--areas', '4', '9', '16', '--types', 'bbox'])
    assert (a.ann, a.extraplots, a.areas) == ('a.json', True, [4, 9, 16])
    with pytest.raises(SystemExit):
        tool.parse_args(['r.json', 'o', '--types', 'segm'])
    assert '--types segm is not built' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tool.parse_args(['r.json', 'o', '--areas', '1', '2'])
    with pytest.raises(SystemExit):
        tool.parse_args(['r.json'])


def _synthetic_result():
    rng = np.random.default_rng(0)
    base = np.sort(rng.random((5, 101, 2, 4, 1)), axis=0)                 # C75 <= C50 <= Loc <= Sim <= Oth
    base[:, :, 1, 1] = -1                                               # a category without small gts
    ps = CEA.stack_ps(base)
    return CEA.ErrorAnalysis(ps, np.linspace(0, 1, 101), [3, 8], ['cat', 'dog'], np.array([[5, 1, 2, 2], [4, 0, 1, 3]]),
                             CEA.area_ranges(), np.array([0.75, 0.5, 0.1]), 0.1, None, None)


def test_stack_ps_aps_and_table():
    res = _synthetic_result()
    ps = res.ps
    assert ps.shape == (7, 101, 2, 4, 1) and (ps >= 0).all() and (ps[6] == 1).all()
    assert (ps[:6, :, 1, 1] == 0).all() and (ps[5, :, 0] == 1).all()
    np.testing.assert_array_equal(res.aps(), E.aps(ps))
    np.testing.assert_array_equal(res.aps(1), E.aps(ps, 1))
    assert res.aps().shape == (7, 4)
    lines = res.table(0).splitlines()
    assert lines[0] == 'bbox-cat' and lines[1].split() == ['type', 'allarea', 'small', 'medium', 'large']
    assert [ln.split()[0] for ln in lines[2:]] == list(E.TYPES)
    assert lines[2].split()[1] == f'{res.aps(0)[0, 0]:.3f}' and res.table().splitlines()[0] == 'bbox-allclass'


def test_tool_outputs_without_matplotlib(tmp_path, capsys):
    tool = _tool()
    res = _synthetic_result()
    assert tool.write_outputs(res, str(tmp_path / 'bbox'), extraplots=True, plt=None) == []
    assert 'the figures were skipped' in capsys.readouterr().out
    z = np.load(tmp_path / 'bbox' / 'error_analysis.npz')
    assert z['ps'].tobytes() == res.ps.tobytes() and list(z['names']) == ['cat', 'dog'] and list(z['cat_ids']) == [3, 8]
    np.testing.assert_array_equal(z['aps'], res.aps())
    np.testing.assert_array_equal(z['aps_per_class'][1], res.aps(1))
    text = (tmp_path / 'bbox' / 'error_analysis.txt').read_text()
    assert text.count('bbox-') == 3 and 'bbox-allclass' in text
    assert sorted(os.listdir(tmp_path / 'bbox')) == ['error_analysis.npz', 'error_analysis.txt']


def test_tool_figures(tmp_path):
    pytest.importorskip('matplotlib')
    tool = _tool()
    res = _synthetic_result()
    out = tmp_path / 'bbox'
    written = tool.write_outputs(res, str(out), extraplots=True, gt_areas=[4.0, 100.0, 2500.0])
    names = {os.path.basename(p) for p in written}
    want = {f'bbox-{c}-{a}.png' for c in ('cat', 'dog', 'allclass') for a in ('allarea', 'small', 'medium', 'large')}
    want |= {f'bbox-{c}-ap bar plot.png' for c in ('cat', 'dog', 'allclass')}
    want |= {'number of annotations per area group.png', 'gt annotation areas histogram plot.png'}
    assert names == want and len(written) == len(want)
    for p in written:
        with open(p, 'rb') as f:
            assert f.read(8) == b'\x89PNG\r\n\x1a\n', p
    plain = tool.write_outputs(res, str(tmp_path / 'plain'))
    assert len(plain) == 12
