"""The proposal recall without a GPU: the numpy restatement (tests/_recall_ref.py) against what the reference's
``eval_recalls`` produced (tests/golden/recall.npz), ``set_recall_param``, the summary text, the ``RecallGt`` tables,
``fast_eval_recall``'s gt selection, the ABI refusals and the missing-GPU error."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import recall_eval as RE

import _recall_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', RR.SETS)
def test_restatement_equals_the_reference_fixture(name, golden):
    gts, proposals, nums, thrs, want, want_ious = RR.load_set(golden('recall'), name)
    got, ious = RR.recalls(gts, proposals, nums, thrs, return_ious=True)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (len(nums), len(thrs))
    np.testing.assert_array_equal(got, want)
    assert ious.dtype == want_ious.dtype == np.float32
    np.testing.assert_array_equal(-np.sort(-ious, axis=1), want_ious)


def test_fixture_holds_the_stated_cases(golden):
    z = golden('recall')
    gts, proposals, nums, thrs, rec, _ = RR.load_set(z, 'main')
    assert nums == [1, 10, 100] and len(thrs) == 10 and thrs.dtype == np.float64
    nd = np.array([len(p) for p in proposals])
    assert (nd > 100).sum() >= 3 and ((nd > 10) & (nd <= 100)).any() and ((nd > 1) & (nd <= 10)).any()
    i = int(z['main/iou07_image'])
    v = RR.R.overlaps(gts[i], proposals[i][:, :4])[0, 0]
    assert v == np.float32(0.7) and not float(v) >= thrs[4] and np.float32(thrs[4]) == v      # a miss in float64 only
    names = list(z['hand/names'])
    assert names == ['no_gts', 'gts_none', 'no_proposals', 'more_gts_than_proposals', 'identical_proposals',
                     'identical_gts', 'second_best', 'best_for_three', 'no_scores']
    hg, hp, hn, _, _, hs = RR.load_set(z, 'hand')
    assert hg[names.index('gts_none')] is None and len(hg[names.index('no_gts')]) == 0
    assert len(hp[names.index('no_proposals')]) == 0 and hp[names.index('no_scores')].shape[1] == 4
    assert (hs[-1] == -1).sum() == 2                                  # 5 gts, 3 proposals: at the largest number only they
    assert RR.load_set(z, 'hand_unsorted')[2] == [300, 100]
    wg, wp, wn, _, _, _ = RR.load_set(z, 'wide')
    assert wn == [64, 65, 1000]
    assert {len(g) for g in wg} == {1, 63, 64, 65, 130} and {len(p) for p in wp} == {1, 63, 64, 65, 257, 1001}
    for name in RR.SETS:                                               # no stored value depends on a tie order
        for p in RR.load_set(z, name)[1]:
            assert p.shape[1] == 4 or len(np.unique(p[:, 4])) == len(p)


def test_restatement_orders_ties_stably_and_cuts_at_the_last_number():
    gts = [np.array([[0, 0, 10, 10]], np.float32)]
    p = np.array([[0, 0, 10, 5, 0.5], [0, 0, 10, 10, 0.5], [0, 0, 10, 8, 0.5]], np.float32)
    assert RR.gt_ious(gts, [p], [1]).tolist() == [[0.5]]              # the first of the equal scores is the top-1
    assert RR.gt_ious(gts, [p[::-1]], [1]).tolist() == [[np.float32(0.8)]]
    assert RR.gt_ious(gts, [p], [3, 1]).tolist() == [[0.5], [0.5]]    # cols = min(n, nums[-1])
    assert RR.gt_ious(gts, [p], [1, 3]).tolist() == [[0.5], [1.0]]
    with pytest.warns(RuntimeWarning):
        assert np.isnan(np.zeros((1, 1), np.int64) / float(0)).all()  # what zero gts give, in numpy's own words
    assert np.isnan(RR.recalls([None], [p], [1], [0.5])).all()


def test_set_recall_param():
    nums, thrs = pkg.set_recall_param([100, 300], None)
    assert nums.tolist() == [100, 300] and thrs.tolist() == [0.5]
    nums, thrs = pkg.set_recall_param(7, 0.75)
    assert nums.tolist() == [7] and thrs.tolist() == [0.75]
    nums, thrs = pkg.set_recall_param((1, 2), (0.5, 0.6))
    assert nums.tolist() == [1, 2] and thrs.tolist() == [0.5, 0.6]
    a, t = np.array([3, 4]), np.arange(0.5, 0.96, 0.05)
    nums, thrs = pkg.set_recall_param(a, t)
    assert nums is a and thrs is t
    assert pkg.set_recall_param(None, t)[0] is None                   # as the reference: passed through


def test_summary_text(capsys):
    rec = np.array([[0.5, 0.25, 0.125], [1.0, 0.3333, 0.0]])
    pkg.print_recall_summary(rec, [10, 100], [0.5, 0.75, 0.9])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln]
    assert lines[1].split('|')[1:-1] == ['     ', ' 0.5   ', ' 0.75  ', ' 0.9   ']
    assert lines[3].split('|')[1:-1] == [' 10  ', ' 0.500 ', ' 0.250 ', ' 0.125 ']
    assert lines[4].split('|')[1:-1] == [' 100 ', ' 1.000 ', ' 0.333 ', ' 0.000 ']
    assert lines[0] == lines[2] == lines[5] and set(lines[0]) == {'+', '-'}
    pkg.print_recall_summary(rec, [10, 100], [0.5, 0.75, 0.9], row_idxs=np.array([1]), col_idxs=np.array([0, 2]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln]
    assert len(lines) == 5 and lines[3].split('|')[1:-1] == [' 100 ', ' 1.000 ', ' 0.000 ']
    pkg.print_recall_summary(rec, [10, 100], [0.5, 0.75, 0.9], logger='silent')
    assert capsys.readouterr().out == ''


def test_recall_gt_tables():
    g = pkg.RecallGt([np.array([[0, 0, 1, 1], [2, 2, 3, 3]], np.float64), None, np.zeros((0, 4)), [[4, 4, 5, 5]]])
    assert g.num_imgs == 4 and g.total_gt == 3 and g.gt.dtype == np.float32 and g.gt.shape == (3, 4)
    assert g.gt_off.tolist() == [0, 2, 2, 2, 3] and g.gt_off.dtype == np.int64 and g.ng.tolist() == [2, 0, 0, 1]
    assert g.gt[2].tolist() == [4, 4, 5, 5]
    assert pkg.RecallGt([]).total_gt == 0 and pkg.RecallGt([None]).gt_off.tolist() == [0, 0]
    with pytest.raises(ValueError, match=r'gts\[0\]'):
        pkg.RecallGt([np.zeros((2, 3))])


def _ann(i, img, cat, box, **kw):
    return dict(id=i, image_id=img, category_id=cat, bbox=box, area=box[2] * box[3], iscrowd=0, **kw)


def coco_dict():
    return dict(images=[dict(id=10, file_name='a.jpg', height=100, width=100), dict(id=20, file_name='b.jpg', height=100, width=100),
                        dict(id=30, file_name='c.jpg', height=100, width=100)],
                categories=[dict(id=1, name='cat'), dict(id=2, name='dog'), dict(id=7, name='bird')],
                annotations=[_ann(1, 10, 1, [0.1, 0.2, 10.3, 20.4]), dict(_ann(2, 10, 2, [5, 5, 10, 10]), iscrowd=1),
                             _ann(3, 10, 7, [50, 50, 20, 30]), _ann(4, 10, 2, [1, 1, 2, 2], ignore=True),
                             _ann(5, 30, 2, [51.18, 40, 95.05, 8.1]), _ann(6, 10, 2, [60, 10, 5, 5], ignore=False)])


def test_fast_eval_recall_selects_the_gts_of_the_reference():
    ds = pkg.CocoBBoxDataset(coco_dict(), classes=('cat', 'dog'))          # 'bird' is outside classes: its box still counts
    assert ds.img_ids == [10, 20, 30]
    g = ds.recall_gt()
    assert g is ds.recall_gt() and isinstance(g, pkg.RecallGt)
    assert g.ng.tolist() == [3, 0, 1]                                      # crowd and ignore dropped; an image without annotations
    want = np.array([[0.1, 0.2, 0.1 + 10.3, 0.2 + 20.4], [50, 50, 70, 80], [60, 10, 65, 15], [51.18, 40, 51.18 + 95.05, 40 + 8.1]],
                    dtype=np.float32)                                      # float64 sums, then one rounding
    np.testing.assert_array_equal(g.gt, want)
    assert g.gt[3, 2] != np.float32(51.18) + np.float32(95.05)              # which a float32 sum would not give


def test_the_refusals_that_stay():
    ds = pkg.CocoBBoxDataset(coco_dict(), classes=('cat', 'dog'))
    empty = [[np.zeros((0, 5), np.float32)] * 2] * 3
    with pytest.raises(NotImplementedError, match="metric='proposal' is not built"):
        ds.evaluate(empty, metric='proposal')
    with pytest.raises(NotImplementedError, match="metric='proposal' is not built"):
        ds.evaluate(empty, metric=['proposal', 'proposal_fast'])
    with pytest.raises(NotImplementedError, match="metric='proposal_fast' is not built"):
        pkg.evaluate_bbox(empty, coco_dict(), metric='proposal_fast')
    with pytest.raises(KeyError, match='nonsense'):
        ds.evaluate(empty, metric=['proposal_fast', 'nonsense'])
    cds = pkg.CustomBBoxDataset([dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64))], ('a',))
    with pytest.raises(NotImplementedError, match="metric='recall'"):
        cds.evaluate([[np.zeros((0, 5), np.float32)]], metric='recall')


def test_without_a_gpu_every_entry_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    gts = [np.array([[0, 0, 10, 10]], np.float32)]
    p = [np.array([[0, 0, 10, 9, 0.5]], np.float32)]
    for call in (lambda: pkg.eval_recalls(gts, p, [1], [0.5]),
                 lambda: pkg.eval_recalls(gts, [p], [1], [0.5]),
                 lambda: pkg.eval_recalls(gts, [p[0][:, :4]], [1], [0.5]),
                 lambda: pkg.eval_recalls(gts, RR.flat_form(p), [1], [0.5]),
                 lambda: pkg.recall_device(RR.flat_form(p), pkg.RecallGt(gts), [1], [0.5]),
                 lambda: pkg.CocoBBoxDataset(coco_dict()).evaluate([[np.zeros((0, 5), np.float32)] * 3] * 3, metric='proposal_fast'),
                 lambda: pkg.CustomBBoxDataset([dict(bboxes=gts[0], labels=np.zeros(1, np.int64))], ('a',)).eval_recalls([p])):
        with pytest.raises(RuntimeError, match='no GPU is visible'):
            call()


def test_headers_binding_and_library_hold_the_new_symbols():
    text = open(os.path.join(ROOT, 'include', 'yv4.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(yv4_[a-z0-9_]+)\s*\(', text))
    new = {'yv4_recall_work', 'yv4_recall_match'}
    assert new <= declared and new <= set(pkg._lib.SIGNATURES) and new == set(pkg._lib.FEATURES['recall'].symbols)
    assert re.search(r'#define\s+YV4_ABI_VERSION\s+8\b', text) and pkg._lib.ABI_VERSION == 8
    lib = pkg._lib.lib()
    for name in new:
        assert hasattr(lib, name), name
    assert pkg._lib.has('recall')
    src = open(os.path.join(ROOT, 'mmdet-yolov4_amd', 'csrc', 'recall.hip')).read()
    for const, value in (('kRcMaxNums', pkg._lib.RECALL_MAX_NUMS), ('kRcLdsBoxes', pkg._lib.RECALL_LDS_BOXES)):
        assert re.search(rf'constexpr int {const} = {value};', src)
    assert pkg._lib.RECALL_MAX_THRS == 256
    for name in ('eval_recalls', 'set_recall_param', 'print_recall_summary', 'RecallGt', 'recall_device'):
        assert hasattr(pkg, name), name
    assert RE.eval_recalls is pkg.eval_recalls


def test_abi_refuses_bad_tables_before_any_device_work():
    lib = pkg._lib.lib()
    # sized by the gts (12 bytes each per number) and one mask bit per box (whole 64-bit words per image) alone
    assert lib.yv4_recall_work(1000, 100, 10, 3) == 8 * 3 * (1000 // 64 + 10 + 1) + 12 * 3 * 100 + 8
    assert lib.yv4_recall_work(0, 0, 1, 1) == 8 * 2 + 8
    assert lib.yv4_recall_work(10, 10, 1, 17) == 0 and lib.yv4_recall_work(-1, 0, 1, 1) == 0
    nums = (ctypes.c_int32 * 17)(*([5] * 17))
    p = ctypes.addressof(nums)
    fake = 0x1000                      # never dereferenced: every call below is refused on the host
    need = lib.yv4_recall_work(8, 4, 2, 2)

    def call(det4=fake, det_off=fake, gt4=fake, gt_off=fake, off_elems=3, N=2, D=8, G=4, nums_p=p, M=2, thrs=fake, T=3,
             work=fake, work_bytes=need, ious=fake, ious_elems=8, counts=fake, counts_elems=6, cap=0):
        return lib.yv4_recall_match(det4, det_off, gt4, gt_off, off_elems, N, D, G, nums_p, M, thrs, T, 1e-6, cap, work,
                                    work_bytes, ious, ious_elems, counts, counts_elems, None)

    def refused(word, **kw):
        assert call(**kw) == -1
        assert word.encode() in lib.yv4_last_error(), lib.yv4_last_error()

    refused('null', det_off=None)
    refused('null', gt_off=None)
    refused('null', counts=None)
    refused('null', thrs=None)
    refused('null', nums_p=None)
    refused('null', work=None)
    refused('null det4', det4=None)
    refused('null gt4', gt4=None)
    refused('proposal numbers', M=17)
    refused('proposal numbers', M=0)
    refused('thresholds', T=257)
    refused('thresholds', T=0)
    refused('N must be positive', N=0)
    refused('entries', off_elems=2)
    refused('gt_ious holds', ious_elems=7)
    refused('counts holds', counts_elems=5)
    refused('work holds', work_bytes=need - 1)
    refused('8-byte aligned', work=fake + 4)
    refused('16-byte aligned', det4=fake + 8)
    refused('lds_cap', cap=-1)
    refused('more than 2^31', D=2 ** 31)
    neg = (ctypes.c_int32 * 2)(5, -1)
    refused('negative', nums_p=ctypes.addressof(neg))
