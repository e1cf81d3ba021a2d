"""Plain-numpy statement of the per-image mAP this package computes on the GPU (analysis.py, csrc/map_image.hip), and
the reading of tests/golden/image_map.npz.

Per image: for each of the ten thresholds and each class the true / false positives of ``_map_ref``'s default rule --
with the IoU compared against the ``np.float64`` threshold in float64, and the visiting order descending score, stable
-- then the 'area' AP over the (image, class)'s own detections, the float32 mean over the classes that have gts as numpy
forms it (pairwise), and the float64 average over the thresholds.  tests/test_image_map_host.py holds it bit for bit
against the fixture, which the reference's ``bbox_map_eval`` produced under numpy 2; tests/test_gpu_image_map.py holds
the kernels against both.
"""
import numpy as np

import _map_ref as R

IOU_THRS = np.linspace(0.5, 0.95, 10)      # ten np.float64 values: what bbox_map_eval iterates over


def tpfp(dets, gts, ignored, thr):
    """One (image, class) at one threshold (``_map_ref.tpfp_default`` without area ranges): ``best >= thr`` is compared
    in ``thr``'s own format -- float64 for the ``np.float64`` thresholds of bbox_map_eval -- and the detections are
    visited by descending score, equal scores in input order.  Returns (tp, fp) bool (num_dets,) IN VISITING ORDER."""
    dets = R.f32(dets).reshape(-1, 5)
    gt, ign = R._stack_gts(gts, ignored)
    visit = np.argsort(-dets[:, 4], kind='stable')
    tp, fp = np.zeros(len(dets), bool), np.zeros(len(dets), bool)
    if len(gt) == 0:
        fp[:] = True
        return tp, fp
    iou = R.overlaps(dets, gt)
    best, which = iou.max(axis=1), iou.argmax(axis=1)
    free = np.ones(len(gt), bool)
    for pos, d in enumerate(visit):
        if best[d] >= thr:
            g = which[d]
            if ign[g]:
                continue
            (tp if free[g] else fp)[pos] = True
            free[g] = False
        else:
            fp[pos] = True
    return tp, fp


def problem_ap(tp, fp, num_gts):
    """The 'area' AP of one problem from its flags in visiting order: integer cumulative counts, recall =
    float32(ctp) / max(num_gts, float32 eps) in float64, precision in float32, the envelope in float64, and the terms
    where recall changes added in ascending position into ONE float64 accumulator, rounded to float32."""
    if len(tp) == 0:
        return np.float32(0)
    ctp, cfp = np.cumsum(tp.astype(np.int64)).astype(np.float32), np.cumsum(fp.astype(np.int64)).astype(np.float32)
    recall = ctp / np.maximum(np.int64(num_gts), R.F32_EPS)
    precision = ctp / np.maximum(ctp + cfp, R.F32_EPS)
    assert recall.dtype == np.float64 and precision.dtype == np.float32
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision.astype(np.float64), [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    acc = np.float64(0)
    for i in np.flatnonzero(mrec[1:] != mrec[:-1]):
        acc = acc + (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return np.float32(acc)


def pairwise_sum(a):
    """numpy's float32 pairwise sum, restated: fewer than 8 values from 0 left to right; up to 128 through eight
    accumulators and the tail; more by halves."""
    n = len(a)
    if n < 8:
        res = np.float32(0)
        for v in a:
            res = np.float32(res + v)
        return res
    if n <= 128:
        r = [np.float32(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = np.float32(r[j] + a[i + j])
            i += 8
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                         + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[i:]:
            res = np.float32(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return np.float32(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def pairwise_mean(aps):
    """``np.array(aps, np.float32).mean()``: the pairwise sum and one float32 division; 0.0 for no value."""
    a = np.asarray(aps, np.float32).reshape(-1)
    if len(a) == 0:
        return np.float32(0)
    return np.float32(pairwise_sum(a) / np.float32(len(a)))


def threshold_average(means):
    """``sum(mean_aps) / len(mean_aps)`` over Python floats."""
    acc = 0.0
    for m in means:
        acc = acc + float(m)
    return np.float64(acc / len(means))


def image_maps(det_results, annotations, iou_thrs=IOU_THRS):
    """(image_map (N,) float64, mean_ap (T, N) float32) of per-image per-class lists against their annotations."""
    N, T = len(det_results), len(iou_thrs)
    C = len(det_results[0])
    per_thr = np.zeros((T, N), np.float32)
    probs = [R.class_problem(det_results, annotations, c) for c in range(C)]
    for i in range(N):
        for t, thr in enumerate(iou_thrs):
            aps = []
            for c in range(C):
                d, g, ign = probs[c][i]
                if len(g) == 0:
                    continue
                tp, fp = tpfp(d, g, ign, thr)
                aps.append(problem_ap(tp, fp, len(g)))
            per_thr[t, i] = pairwise_mean(aps)
    return np.array([threshold_average(per_thr[:, i]) for i in range(N)], np.float64), per_thr


# ---- tests/golden/image_map.npz: every set is stored flat ---------------------------------------------------------------
SETS = ('main', 'wide')


def store_set(out, name, dets, annos):
    N, C = len(dets), len(dets[0])
    rows = [(d, c, i) for i, per_cls in enumerate(dets) for c, d in enumerate(per_cls) if len(d)]
    out[f'{name}/num_img'], out[f'{name}/num_cls'] = np.int64(N), np.int64(C)
    out[f'{name}/det'] = np.concatenate([d for d, _, _ in rows]).astype(np.float32).reshape(-1, 5)
    out[f'{name}/det_label'] = np.concatenate([np.full(len(d), c, np.int32) for d, c, _ in rows])
    out[f'{name}/det_img'] = np.concatenate([np.full(len(d), i, np.int32) for d, _, i in rows])
    gt, lab, img, ign = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros(0, bool)]
    for i, a in enumerate(annos):
        parts = [(a['bboxes'], a['labels'], False)]
        if a.get('labels_ignore') is not None:
            parts.append((a['bboxes_ignore'], a['labels_ignore'], True))
        for b, l, flag in parts:
            gt.append(np.asarray(b, np.float32).reshape(-1, 4))
            lab.append(np.asarray(l, np.int32).reshape(-1))
            img.append(np.full(len(lab[-1]), i, np.int32))
            ign.append(np.full(len(lab[-1]), flag))
    out[f'{name}/gt'], out[f'{name}/gt_label'] = np.concatenate(gt), np.concatenate(lab)
    out[f'{name}/gt_img'], out[f'{name}/gt_ignore'] = np.concatenate(img), np.concatenate(ign)
    out[f'{name}/has_ignore'] = np.array([a.get('labels_ignore') is not None for a in annos])


def load_set(z, name):
    """(det_results, annotations, image_map (N,) float64, mean_ap (T, N) float32) of one set of the fixture."""
    N, C = int(z[f'{name}/num_img']), int(z[f'{name}/num_cls'])
    det, dl, di = z[f'{name}/det'], z[f'{name}/det_label'], z[f'{name}/det_img']
    dets = [[np.zeros((0, 5), np.float32) for _ in range(C)] for _ in range(N)]
    key = di.astype(np.int64) * C + dl
    order = np.argsort(key, kind='stable')
    cuts = np.searchsorted(key[order], np.arange(N * C + 1))
    for p in np.flatnonzero(np.diff(cuts)):
        dets[p // C][p % C] = det[order[cuts[p]:cuts[p + 1]]]
    gt, gl, gi, ign = z[f'{name}/gt'], z[f'{name}/gt_label'], z[f'{name}/gt_img'], z[f'{name}/gt_ignore']
    annos = []
    for i, has in enumerate(z[f'{name}/has_ignore']):
        m = gi == i
        a = dict(bboxes=gt[m & ~ign], labels=gl[m & ~ign].astype(np.int64))
        if has:
            a.update(bboxes_ignore=gt[m & ign], labels_ignore=gl[m & ign].astype(np.int64))
        annos.append(a)
    return dets, annos, z[f'{name}/map'], z[f'{name}/mean_ap']
