"""tests/_post_ref.py pinned without a GPU: its merge and slot tables against the CPU restatement of aug_test in
tests/test_tta_host.py on the reference's own per-augmentation outputs (tests/golden/v3_tta.npz), its float64 decode
against the fp32 oracles on the tiny goldens' pred maps, and its comparator against planted single-element faults.
tests/test_gpu_tta_kernels.py and tests/test_gpu_decode_edges.py hold the kernels to it."""
import json

import numpy as np
import pytest
import torch

import _post_ref as R
from oracle import yolov3_oracle as V3
from oracle import yolov4_oracle as O
from test_tta_host import _map_back

FLIP = {None: 0, 'horizontal': 1, 'vertical': 2, 'diagonal': 3}
TTA_CASES = ['scales_hflip', 'vflip_dflip', 'split', 'empty']


def _case(g, name):
    return json.loads(str(g['cases']))[name]


def _fixture_augs(g, name, case):
    """The reference's get_bboxes(with_nms=False) outputs as merge inputs: every row is a slot, in order."""
    augs, meta = [], []
    for a in range(case['num_augs']):
        b, s, c = g[f'{name}/bboxes{a}'], g[f'{name}/scores{a}'], g[f'{name}/conf{a}']
        augs.append(dict(boxes=b[None], conf=c[None], cls=np.ascontiguousarray(s[:, :-1])[None],
                         slots=np.arange(b.shape[0])[None], flip=FLIP[case['flips'][a]]))
        shape = g[f'{name}/img_shape{a}']
        meta.append([[shape[0], shape[1], *g[f'{name}/scale_factor{a}']]])
    return augs, np.asarray(meta, np.float32)


@pytest.mark.parametrize('name', TTA_CASES)
def test_merge_ref_equals_cpu_aug_merge_inputs(golden, name):
    g = golden('v3_tta')
    case = _case(g, name)
    thr = case['test_cfg']['score_thr']
    augs, meta = _fixture_augs(g, name, case)
    boxes_out, keys, max_coord = R.merge_ref(augs, meta, 6, thr)
    mapped, scores, confs = [], [], []
    for a in range(case['num_augs']):
        shape = tuple(int(v) for v in g[f'{name}/img_shape{a}'])
        mapped.append(_map_back(torch.from_numpy(g[f'{name}/bboxes{a}']), shape, g[f'{name}/scale_factor{a}'],
                                case['flips'][a]))
        scores.append(torch.from_numpy(g[f'{name}/scores{a}']))
        confs.append(torch.from_numpy(g[f'{name}/conf{a}']))
        # every augmentation's mapped boxes, bit for bit
        lo = sum(m.shape[0] for m in mapped[:-1])
        assert R.diff_bits(boxes_out[0, lo:lo + mapped[-1].shape[0]], mapped[-1].numpy(), f'boxes of aug {a}') is None
    mapped, scores, confs = torch.cat(mapped), torch.cat(scores), torch.cat(confs)
    # multiclass_nms' inputs (bbox_nms.py:52-62): the passing set, then scores * score_factors
    valid = scores[:, :-1] > thr
    m, c = valid.nonzero(as_tuple=True)
    want_score = (scores[:, :-1] * confs[:, None])[valid].numpy()
    flat = R.key_flat(keys[0])
    order = np.argsort(flat)
    np.testing.assert_array_equal(flat[order], (m * 6 + c).numpy())
    assert R.diff_bits(R.key_score(keys[0])[order], want_score, 'scores') is None
    if m.numel():
        assert R.diff_bits(max_coord, mapped[m.unique()].max().numpy()[None], 'max_coord') is None
    else:
        assert name == 'empty' and max_coord[0] == -np.inf and keys[0].size == 0
    # ascending key = descending score, ties to the lower flat index
    by_score = np.lexsort((flat, -R.key_score(keys[0]).astype(np.float64)))
    np.testing.assert_array_equal(by_score, np.arange(flat.size))


@pytest.mark.parametrize('name', ['scales_hflip', 'vflip_dflip', 'split'])
def test_slots_ref_equals_host_lexsort(golden, name):
    g = golden('v3_tta')
    case = _case(g, name)
    nms_pre = case['test_cfg']['nms_pre']
    for a in range(case['num_augs']):
        preds = [torch.from_numpy(g[f'{name}/pred{a}_{i}']) for i in range(3)]
        confs = [c[0].numpy() for _, c, _ in V3.decode_maps_v3(preds, 6)]
        sizes = [c.shape[0] for c in confs]
        want, base = [], 0
        for c in confs:                                  # tests/test_tta_host.py's statement, per level
            idx = np.arange(c.shape[0])
            if 0 < nms_pre < c.shape[0]:
                idx = np.lexsort((idx, -c.astype(np.float64)))[:nms_pre]
            want.append(idx + base)
            base += c.shape[0]
        slots, keys = R.slots_ref(np.concatenate(confs)[None], sizes, nms_pre)
        assert R.diff_slots(slots, np.concatenate(want)[None], R.slot_sizes(sizes, nms_pre)) is None
        # the slots pick the fixture's rows
        np.testing.assert_array_equal(np.concatenate(confs)[slots[0]], g[f'{name}/conf{a}'])
        for l, n_l in enumerate(sizes):                  # the admission key admits exactly the level's slots
            lo = sum(sizes[:l])
            adm = R.conf_key(confs[l], np.arange(lo, lo + n_l)) <= keys[0, l]
            assert adm.sum() == (nms_pre if 0 < nms_pre < n_l else n_l)
            assert set(np.nonzero(adm)[0] + lo) == set(want[l])


def test_keys_are_order_preserving_and_invertible():
    s = np.array([-np.inf, -2.5, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.05, 0.5, 1.0, 3.0, np.inf], np.float32)
    k = R.score_to_key(s)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) < 0).all()          # descending score = ascending key
    assert R.diff_bits(R.key_to_score(k), s, 'round trip') is None
    assert R.score_to_key(np.float32(1.0)) == np.uint32(0x407FFFFF)                   # ~(0x3F800000 | 0x80000000)
    ck = R.conf_key(np.float32([0.5, 0.5, 0.75]), np.array([7, 3, 9]))
    assert ck.dtype == np.uint64 and ck[2] < ck[1] < ck[0] and int(ck[1]) & 0xFFFFFFFF == 3


def _nchw_to_nhwc(p):
    return np.ascontiguousarray(p.transpose(0, 2, 3, 1))


@pytest.mark.parametrize('name', ['tiny_v4', 'tiny_v5'])
def test_decode_ref_agrees_with_csp_oracle(golden, name):
    g = golden(name)
    preds = [g[f'pred{i}'] for i in range(3)]
    boxes, conf, cls = O.decode_maps([torch.from_numpy(p) for p in preds], 80)
    base = R.base_anchors(O.DEFAULT_BASE_SIZES, O.DEFAULT_STRIDES)
    for b, o in zip(base, O.base_anchors()):
        np.testing.assert_array_equal(b, o.numpy())
    rb, rc, rs = R.decode_ref([_nchw_to_nhwc(p) for p in preds], 3, 80, O.DEFAULT_STRIDES, base, v3=False)
    # fp32 torch against float64: a few ulp of the largest coordinate
    assert np.abs(boxes.numpy() - rb).max() <= 4 * np.spacing(np.float32(np.abs(rb).max()))
    assert np.abs(conf.numpy() - rc).max() <= 2e-7 and np.abs(cls.numpy() - rs).max() <= 2e-7
    sf = g['scale_factors']
    rb2 = R.decode_ref([_nchw_to_nhwc(p) for p in preds], 3, 80, O.DEFAULT_STRIDES, base, False, scale_factor=sf)[0]
    np.testing.assert_array_equal(rb2, rb / sf.astype(np.float64)[:, None, :])


def test_decode_ref_agrees_with_v3_oracle(golden):
    g = golden('tiny_v3')
    preds = [g[f'pred{i}'] for i in range(3)]
    lv = V3.decode_maps_v3([torch.from_numpy(p) for p in preds], 6)
    base = R.base_anchors(V3.V3_BASE_SIZES, V3.V3_STRIDES)
    rb, rc, rs = R.decode_ref([_nchw_to_nhwc(p) for p in preds], 3, 6, V3.V3_STRIDES, base, v3=True)
    boxes = torch.cat([b for b, _, _ in lv], 1).numpy()
    # x = centre -+ size / 2 cancels: the error scales with the box's largest coordinate (= |centre| + size / 2), of
    # which the fp32 chain sigmoid / exp, scale, shift, halve, add is allowed 6 ulp
    ulp = np.spacing(np.abs(rb).max(-1, keepdims=True).astype(np.float32)).astype(np.float64)
    assert (np.abs(boxes - rb) <= 6 * ulp).all(), (np.abs(boxes - rb) / ulp).max()
    assert np.abs(torch.cat([c for _, c, _ in lv], 1).numpy() - rc).max() <= 2e-7
    assert np.abs(torch.cat([s for _, _, s in lv], 1).numpy() - rs).max() <= 2e-7


def test_candidates_from_restates_the_heads():
    rng = np.random.default_rng(11)
    N, sizes, C = 2, [5, 9], 3
    conf = rng.random((N, 14), dtype=np.float32)
    cls = rng.random((N, 14, C), dtype=np.float32)
    conf[0, 3] = conf[0, 4] = conf[0, 8]                     # ties: the lower anchor index is admitted first
    thr = cls[1, 2, 1] * conf[1, 2]                          # a product equal to the threshold does not pass
    keys, adm = R.candidates_from(conf, cls, thr, v3=False)
    assert adm.all() and 2 * C + 1 not in R.key_flat(keys[1])
    for n in range(N):
        want = np.nonzero((cls[n] * conf[n][:, None] > thr).reshape(-1))[0]
        np.testing.assert_array_equal(np.sort(R.key_flat(keys[n])), want)
    # v3: the test is on cls, the key carries cls * conf; per-level top-2 and conf >= conf_thr
    _, tk = R.slots_ref(conf, sizes, 2)
    cthr = float(np.sort(conf[0])[-4])
    keys, adm = R.candidates_from(conf, cls, 0.5, v3=True, level_sizes=sizes, topk_keys=tk, conf_thr=cthr)
    for n in range(N):
        top = np.concatenate([np.lexsort((np.arange(5), -conf[n, :5].astype(np.float64)))[:2],
                              5 + np.lexsort((np.arange(9), -conf[n, 5:].astype(np.float64)))[:2]])
        want_adm = np.zeros(14, bool)
        want_adm[top] = True
        want_adm &= conf[n] >= np.float32(cthr)
        np.testing.assert_array_equal(adm[n], want_adm)
        want = np.nonzero(((cls[n] > np.float32(0.5)) & want_adm[:, None]).reshape(-1))[0]
        flat = R.key_flat(keys[n])
        np.testing.assert_array_equal(np.sort(flat), want)
        np.testing.assert_array_equal(R.key_score(keys[n]), (cls[n] * conf[n][:, None]).reshape(-1)[flat])
    assert adm[0, np.argsort(conf[0])[-4]] or not np.isin(np.argsort(conf[0])[-4], top)     # `>=`: equality stays
    # class-agnostic: one column, score = conf
    keys, _ = R.candidates_from(conf, None, conf[0, 6], v3=False)
    np.testing.assert_array_equal(np.sort(R.key_flat(keys[0])), np.nonzero(conf[0] > conf[0, 6])[0])


# ---- the comparator names the element -------------------------------------------------------------------------------
def _merge_case():
    rng = np.random.default_rng(5)
    N, C, S = 2, 3, (4, 6)
    augs = []
    for a, s in enumerate(S):
        total = s + 3
        augs.append(dict(boxes=(rng.random((N, total, 4), dtype=np.float32) * 100), conf=rng.random((N, total), dtype=np.float32),
                         cls=rng.random((N, total, C), dtype=np.float32),
                         slots=np.stack([rng.permutation(total)[:s] for _ in range(N)]), flip=a + 1))
    meta = (rng.random((2, N, 6), dtype=np.float32) + 0.5) * np.float32([300, 300, 1, 1, 1, 1])
    return augs, meta, C, S


def test_comparator_names_a_swapped_pair_of_equal_conf_slots():
    conf = np.random.default_rng(2).random((2, 50), dtype=np.float32)
    conf[1, 30] = conf[1, 41] = np.float32(0.99)             # level 1 of image 1: two equal, highest values
    slots, _ = R.slots_ref(conf, [20, 30], 10)
    assert list(slots[1, 10:12]) == [30, 41]
    bad = slots.copy()
    bad[1, 10], bad[1, 11] = slots[1, 11], slots[1, 10]
    assert R.diff_slots(slots, slots, [10, 10]) is None
    msg = R.diff_slots(bad, slots, [10, 10])
    assert msg.startswith('image 1 level 1 slot 0: got anchor 41, want 30'), msg


def test_comparator_names_a_key_one_ulp_off_and_a_missing_key():
    augs, meta, C, S = _merge_case()
    _, keys, _ = R.merge_ref(augs, meta, C, 0.3)
    want = keys[1]
    assert want.size > 6 and R.diff_keys(want[::-1], want, C, S, image=1) is None
    i = 5
    flat = int(R.key_flat(want[i]))
    where = f'image 1 augmentation {0 if flat // C < S[0] else 1} slot {flat // C - (0 if flat // C < S[0] else S[0])} class {flat % C}'
    for step in (1, -1):                                     # the score one ulp down / up
        bad = want.copy()
        one = np.uint64(1) << np.uint64(32)
        bad[i] = want[i] + one if step > 0 else want[i] - one
        assert R.key_score(bad[i]) == np.nextafter(R.key_score(want[i]), np.float32(-step * np.inf))
        msg = R.diff_keys(bad, want, C, S, image=1)
        assert msg.startswith('score differs: got ' + where) and 'want ' + where in msg, msg
    msg = R.diff_keys(np.delete(want, i), want, C, S, image=1)
    assert msg.startswith(f'{want.size - 1} keys, want {want.size}') or msg.startswith('missing'), msg
    assert 'missing ' + where in msg, msg
    msg = R.diff_keys(want, np.delete(want, i), C, S, image=1)
    assert 'unexpected ' + where in msg, msg


def test_comparator_names_a_max_coord_one_ulp_off():
    augs, meta, C, _ = _merge_case()
    boxes, _, mc = R.merge_ref(augs, meta, C, 0.3)
    assert R.diff_bits(mc, mc.copy(), 'max_coord') is None
    bad = mc.copy()
    bad[1] = np.nextafter(mc[1], np.float32(np.inf), dtype=np.float32)
    msg = R.diff_bits(bad, mc, 'max_coord')
    assert msg.startswith('max_coord image 1: got'), msg
    bad = boxes.copy()
    bad[0, 7, 2] = np.nextafter(boxes[0, 7, 2], np.float32(0), dtype=np.float32)
    assert R.diff_bits(bad, boxes, 'boxes_out').startswith('boxes_out image 0 element (7, 2)')
    # -0.0 and +0.0 are different bits
    assert R.diff_bits(np.float32([-0.0]), np.float32([0.0]), 'max_coord') is not None
