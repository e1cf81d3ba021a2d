"""Generate tests/golden/recall.npz: outputs of the REFERENCE's ``eval_recalls`` on synthetic images.

Run in the build container only:   python tests/golden/make_golden_recall.py
``mmdet/core/evaluation/recall.py`` and ``bbox_overlaps.py`` are imported from the reference checkout the way
``make_golden_map.py`` imports ``mean_ap.py`` and run as they are under this container's numpy (2.x).  What they import
and the container lacks is represented by stand-ins with no arithmetic: ``mmcv.utils.print_log`` and
``terminaltables.AsciiTable``.  No line of the reference is copied here.

Two things are wrapped around the reference's module, neither inside its arithmetic:

* ``np``.  Under numpy 2 ``np.array(all_ious)`` (``recall.py:102``) raises on images of unequal shapes.  The module's
  ``np`` is replaced by a proxy that forwards every attribute; only ``array`` differs: when numpy raises on an
  inhomogeneous list it falls back to the 1-D object array (one block per image) that ``_recalls`` indexes.
* ``_recalls``.  The sorted ``_ious`` are a local of ``_recalls``.  The wrapper calls the reference's ``_recalls`` a second
  time with, as thresholds, every distinct float32 value of the IoU blocks plus -1 and 0: every recorded value is one
  of them, so ``recall * total_gt`` at consecutive candidates gives each value's multiplicity, and with it the sorted
  rows exactly (``-0`` reads as ``0``).

The fixture is data only: per set the inputs (flat), the parameters, ``recalls`` (float64) and the sorted ``_ious``
(float32, descending).  Scores are distinct inside every image (asserted), so no stored value depends on a tie order.

Sets.  ``main``: 40 synthetic images of ``_map_data.synth_dataset`` plus its four crafted ones (the IoU == float32(0.7)
pair among them), per image the class lists concatenated and the labels dropped, plus three dense images of more than
100 proposals; thresholds ``np.arange(0.5, 0.96, 0.05)``, proposal numbers (1, 10, 100).  ``hand``: built by hand, see
``hand_built``; ``hand_unsorted``: ``proposal_nums = (300, 100)``, where the last entry truncates.  ``wide``: G and n
around 64 and beyond, proposal numbers (64, 65, 1000), gts on a grid and proposals that are copies jittered by whole
pixels, so that most steps hand a gt to a proposal, many rows lose their cached best column and equal IoUs occur.
"""
import importlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import as R  # noqa: E402
import _recall_ref as RR  # noqa: E402
from _map_data import boxes, synth_dataset  # noqa: E402


class _NumpyProxy:
    """numpy, except that ``array`` of an inhomogeneous list gives the 1-D object array numpy 1.x built."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *args, **kwargs):
        try:
            return np.array(obj, *args, **kwargs)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


class _Table:
    """terminaltables.AsciiTable's place: it takes the rows and renders nothing."""
    table = ''

    def __init__(self, table_data):
        pass


def import_reference_recall():
    mmcv = R._mod('mmcv')
    mmcv.utils = R._mod('mmcv.utils', print_log=lambda *a, **k: None)
    R._mod('terminaltables', AsciiTable=_Table)
    m = os.path.join(R.REF, 'mmdet')
    R._pkg('mmdet', m)
    R._pkg('mmdet.core', os.path.join(m, 'core'))
    R._pkg('mmdet.core.evaluation', os.path.join(m, 'core', 'evaluation'))
    M = importlib.import_module('mmdet.core.evaluation.recall')
    M.np = _NumpyProxy()
    return M


class Reference:
    """The reference's ``eval_recalls`` with its sorted ``_ious`` recovered (see the module docstring)."""

    def __init__(self):
        self.M = import_reference_recall()
        self.inner = self.M._recalls
        self.M._recalls = self._wrapped
        self.sorted_ious = None

    def _wrapped(self, all_ious, proposal_nums, thrs):
        out = self.inner(all_ious, proposal_nums, thrs)
        total = sum(b.shape[0] for b in all_ious)
        values = [np.asarray(b, np.float32).reshape(-1) for b in all_ious] + [np.array([-1, 0], np.float32)]
        cand = np.unique(np.concatenate(values))                       # ascending float32
        assert cand.dtype == np.float32
        if total:
            at_least = np.rint(self.inner(all_ious, proposal_nums, cand) * total).astype(np.int64)     # (M, len(cand))
            exactly = at_least - np.concatenate([at_least[:, 1:], np.zeros((len(at_least), 1), np.int64)], axis=1)
            assert (exactly >= 0).all() and (exactly.sum(axis=1) == total).all()
            self.sorted_ious = np.stack([np.repeat(cand[::-1], e[::-1]) for e in exactly]).astype(np.float32)
        else:
            self.sorted_ious = np.zeros((len(proposal_nums), 0), np.float32)
        return out

    def __call__(self, gts, proposals, proposal_nums, iou_thrs):
        rec = self.M.eval_recalls(gts, proposals, proposal_nums, iou_thrs, logger='silent')
        return rec, self.sorted_ious


def _f(rows, cols):
    return np.array(rows, np.float32).reshape(-1, cols)


def distinct_scores(proposals):
    return all(p.shape[1] != 5 or len(np.unique(p[:, 4])) == len(p) for p in proposals if p.size)


def main_set():
    for seed in itertools.count(20261020):                              # the first seed whose images have distinct scores
        rng = np.random.default_rng(seed)
        dets, annos = synth_dataset(rng, 40, 6, distinct_scores=True)
        proposals = RR.concat_classes(dets)
        gts = [a['bboxes'] for a in annos]
        for n, g in ((150, 12), (101, 3), (260, 30)):                   # dense images: more than 100 proposals
            gb = boxes(rng, g)
            reps = np.concatenate([gb[rng.integers(0, g, n - 20)] + rng.normal(0, 8, (n - 20, 4)).astype(np.float32),
                                   boxes(rng, 20)], axis=0)
            sc = (rng.choice(20000, size=n, replace=False) / 20000).astype(np.float32)
            proposals.append(np.concatenate([reps, sc[:, None]], axis=1).astype(np.float32))
            gts.append(gb)
        if distinct_scores(proposals):
            return gts, proposals


def hand_built(ref):
    """(gts, proposals, names); every claim in the comments is asserted on the reference's own output."""
    gts, proposals, names = [], [], []

    def image(name, g, p, cols=5):
        gts.append(None if g is None else _f(g, 4))
        proposals.append(_f(p, cols))
        names.append(name)

    def alone(nums=(10,)):
        return ref([gts[-1]], [proposals[-1]], list(nums), [0.5])[1]

    image('no_gts', [], [[10, 10, 50, 50, 0.9], [60, 60, 90, 90, 0.4]])
    image('gts_none', None, [[10, 10, 50, 50, 0.8], [60, 60, 90, 90, 0.3]])
    image('no_proposals', [[10, 10, 50, 50], [100, 100, 180, 160]], [])
    assert (alone() == 0).all() and alone().shape == (1, 2)            # G zeros
    # 5 gts and 3 proposals: two -1 entries, recall at most 3/5
    image('more_gts_than_proposals',
          [[0, 0, 40, 40], [100, 0, 140, 40], [200, 0, 240, 40], [300, 0, 340, 40], [400, 0, 440, 40]],
          [[0, 0, 40, 38, 0.9], [100, 0, 140, 30, 0.7], [300, 2, 340, 40, 0.5]])
    assert (alone()[0] == -1).sum() == 2 and (alone()[0] >= 0.5).sum() == 3
    # two identical proposals on one gt: the gt takes the first in visiting order, nothing is left for the second
    image('identical_proposals', [[10, 10, 50, 50]], [[10, 10, 50, 48, 0.6], [10, 10, 50, 48, 0.7]])
    # two identical gts under one proposal: the first row takes it, the second falls to a proposal it does not touch
    image('identical_gts', [[10, 10, 50, 50], [10, 10, 50, 50]], [[10, 10, 50, 50, 0.9], [200, 200, 240, 240, 0.8]])
    assert alone()[0].tolist() == [1.0, 0.0]
    # gt B's best proposal (0.9) is taken by gt A (1.0): B falls to its second best (0.8 / 0.9)
    image('second_best', [[0, 0, 100, 100], [0, 0, 100, 90]], [[0, 0, 100, 100, 0.9], [0, 0, 100, 80, 0.8]])
    s = alone()[0]
    assert s[0] == 1.0 and s[1] == np.float32(8000) / np.float32(9000) and s[1] < np.float32(0.9)
    # one proposal is the best of three gts; the two losers fall to weaker ones
    image('best_for_three', [[0, 0, 100, 100], [0, 0, 100, 96], [0, 4, 100, 100]],
          [[300, 300, 340, 340, 0.95], [0, 0, 100, 99, 0.9], [0, 0, 90, 100, 0.5], [0, 0, 100, 60, 0.4]])
    from mmdet.core.evaluation.bbox_overlaps import bbox_overlaps
    assert (bbox_overlaps(gts[-1], proposals[-1][:, :4]).argmax(axis=1) == 1).all()
    # (n, 4) proposals without scores keep their order
    image('no_scores', [[10, 10, 50, 50], [100, 100, 180, 160]],
          [[100, 100, 180, 150], [10, 10, 50, 44], [12, 10, 50, 50], [300, 300, 320, 320]], cols=4)
    assert alone((1,))[0].max() == np.float32(50) / np.float32(60)       # the first ROW of the array, not a best score
    return gts, proposals, names


def unsorted_set(rng):
    """proposal_nums = (300, 100): cols = min(n, 100), so the '300' row sees 100 columns too."""
    gts, proposals = [], []
    for n, g in ((350, 9), (150, 5), (40, 4)):
        gb = boxes(rng, g)
        # the good copies sit late in visiting order: beyond column 100 they must not count
        far = boxes(rng, n - g) + np.float32(1000)
        sc = np.sort((rng.choice(20000, size=n, replace=False) / 20000).astype(np.float32))[::-1]
        p = np.concatenate([far, gb + np.float32(1)], axis=0)
        proposals.append(np.concatenate([p, sc[:, None]], axis=1).astype(np.float32))
        gts.append(gb)
    return gts, proposals


def wide_set(rng):
    pairs = [(1, 1), (1, 1001), (63, 64), (64, 63), (64, 64), (65, 65), (65, 257), (63, 257), (130, 63), (64, 1001),
             (130, 1001)]
    assert {g for g, _ in pairs} == {1, 63, 64, 65, 130} and {n for _, n in pairs} == {1, 63, 64, 65, 257, 1001}
    gts, proposals = [], []
    for G, n in pairs:
        k = np.arange(G)
        gb = np.stack([(k % 12) * 40, (k // 12) * 40, (k % 12) * 40 + 32, (k // 12) * 40 + 32], axis=1).astype(np.float32)
        src = rng.integers(0, G, n)
        p = gb[src] + rng.integers(-4, 5, (n, 4)).astype(np.float32)     # whole pixels: equal IoUs occur
        sc = (rng.permutation(n) + 1).astype(np.float32) / np.float32(2048)
        proposals.append(np.concatenate([p, sc[:, None]], axis=1).astype(np.float32))
        gts.append(gb)
    return gts, proposals


def main():
    ref = Reference()
    rng = np.random.default_rng(20261021)
    out = {}
    thrs = np.arange(0.5, 0.96, 0.05)
    sets = {}
    sets['main'] = main_set() + ((1, 10, 100), thrs)
    hg, hp, names = hand_built(ref)
    sets['hand'] = (hg, hp, (1, 2, 3, 10), thrs)
    sets['hand_unsorted'] = unsorted_set(rng) + ((300, 100), thrs)
    sets['wide'] = wide_set(rng) + ((64, 65, 1000), thrs)
    assert sorted(sets) == sorted(RR.SETS)
    for name, (gts, proposals, nums, t) in sets.items():
        assert distinct_scores(proposals), name
        rec, sorted_ious = ref(gts, proposals, list(nums), t)
        assert rec.dtype == np.float64 and rec.shape == (len(nums), len(t))
        RR.store_set(out, name, gts, proposals, nums, t, rec, sorted_ious)
        print(name, len(gts), 'images', sum(len(p) for p in proposals), 'proposals', rec.mean(axis=1))
    out['hand/names'] = np.array(names)
    # the crafted IoU == float32(0.7) pair of the main set: a miss at the float64 threshold 0.7
    g, p = sets['main'][0], sets['main'][1]
    i = next(i for i in range(len(g)) if len(g[i]) == 1 and len(p[i]) == 1 and (g[i][0] == [0, 0, 10, 10]).all())
    s = ref([g[i]], [p[i]], [1], thrs)
    assert s[1][0, 0] == np.float32(0.7) and s[0][0].tolist() == [1.0] * 4 + [0.0] * 6
    out['main/iou07_image'] = np.int64(i)
    # the unsorted case: both rows see the first 100 columns only, so the late good copies never count
    r = ref(*sets['hand_unsorted'][:2], [300, 100], thrs)[0]
    assert (r[0] == r[1]).all() and r[0, 0] < 1.0
    assert ref(*sets['hand_unsorted'][:2], [100, 300], thrs)[0][1, 0] > r[0, 0]
    path = os.path.join(HERE, 'recall.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
