"""The good / bad gallery end to end on the GPU: ``ResultVisualizer.evaluate_and_show`` over six small JPEG files with
hand-made results and annotations -- the names under ``good/`` and ``bad/``, every file's bytes, the clipping of
``topk``, a callable ``eval_fn`` -- and ``tools/analyze_results.py`` over the same files as a COCO set."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import analysis as A

import _draw_data as D
import _draw_gt_ref as GR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ('cat', 'dog', 'bird')
SIZES = [(48, 64), (64, 80), (80, 96), (56, 72), (72, 88), (64, 64)]                 # (h, w): 64x48 .. 96x80
GT = [10.0, 8.0, 50.0, 40.0]                                                         # 40 wide: a shift of s gives IoU (40-s)/(40+s)
# image -> (class of the gt or None, the class's detections): mAP 1.0, 0.0, 0.7, 0.0, 1.0, 0.1
CASES = [(0, [[10, 8, 50, 40, 0.9]]), (1, []), (2, [[14, 8, 54, 40, 0.8], [30, 30, 44, 44, 0.2]]), (None, [[5, 5, 30, 30, 0.6]]),
         (1, [[10, 8, 50, 40, 0.7]]), (0, [[22, 8, 62, 40, 0.5]])]
WANT_MAPS = [1.0, 0.0, 0.7, 0.0, 1.0, 0.1]


class Data:
    """What ``evaluate_and_show`` reads of a dataset."""
    CLASSES = CLASSES

    def __init__(self, prefix, annos):
        self.img_prefix = prefix
        self.data_infos = [dict(filename=f'img{k}.jpg') for k in range(len(annos))]
        self.annos = annos

    def __len__(self):
        return len(self.annos)

    def get_ann_info(self, i):
        return self.annos[i]


@pytest.fixture(scope='module')
def gallery(tmp_path_factory, gpu_device):
    src = tmp_path_factory.mktemp('src')
    imgs = [D.image(h, w, 50 + k) // 2 + 64 for k, (h, w) in enumerate(SIZES)]
    pkg.imwrite(imgs, [str(src / f'img{k}.jpg') for k in range(len(imgs))])
    results, annos = [], []
    for cls, rows in CASES:
        per_cls = [np.zeros((0, 5), np.float32) for _ in CLASSES]
        per_cls[2 if cls is None else cls] = np.array(rows, np.float32).reshape(-1, 5)
        results.append(per_cls)
        annos.append(dict(bboxes=np.array([GT] if cls is not None else [], np.float32).reshape(-1, 4),
                          labels=np.array([cls] if cls is not None else [], np.int64)))
    decoded = [a.cpu().numpy() for a in pkg.imread([str(src / f'img{k}.jpg') for k in range(len(imgs))])]
    return dict(src=str(src), results=results, annos=annos, decoded=decoded, data=Data(str(src), annos))


def _expected_file(g, k, score_thr=0):
    dets = np.concatenate(g['results'][k])
    labels = np.concatenate([np.full(len(r), c) for c, r in enumerate(g['results'][k])]).astype(int)
    want = GR.draw_gt_det(g['decoded'][k], g['annos'][k]['bboxes'], list(g['annos'][k]['labels']), dets, list(labels),
                          list(CLASSES), score_thr=score_thr)
    return pkg.imencode(want)


def _files(d):
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def test_the_scores_are_the_hand_made_ones(gallery):
    maps = pkg.image_maps(gallery['results'], gallery['annos'])
    assert [round(float(m), 12) for m in maps] == WANT_MAPS


def test_topk_2_names_and_bytes(gallery, tmp_path):
    good, bad = pkg.ResultVisualizer().evaluate_and_show(gallery['data'], gallery['results'], topk=2, show_dir=str(tmp_path / 'w'))
    assert [i for i, _ in bad] == [1, 3] and [i for i, _ in good] == [0, 4]             # ties stay in index order
    got_good, got_bad = _files(tmp_path / 'w' / 'good'), _files(tmp_path / 'w' / 'bad')
    assert sorted(got_good) == ['img0_1.0.jpg', 'img4_1.0.jpg'] and sorted(got_bad) == ['img1_0.0.jpg', 'img3_0.0.jpg']
    for files in (got_good, got_bad):
        for name, data in files.items():
            assert data == _expected_file(gallery, int(name[3])), name


def test_topk_5_clips_to_3_and_the_score_threshold_reaches_the_drawing(gallery, tmp_path):
    vis = pkg.ResultVisualizer(score_thr=0.3)
    good, bad = vis.evaluate_and_show(gallery['data'], gallery['results'], topk=5, show_dir=str(tmp_path / 'w'))
    assert [i for i, _ in bad] == [1, 3, 5] and [i for i, _ in good] == [2, 0, 4]
    got_good, got_bad = _files(tmp_path / 'w' / 'good'), _files(tmp_path / 'w' / 'bad')
    assert sorted(got_good) == ['img0_1.0.jpg', 'img2_0.7.jpg', 'img4_1.0.jpg']
    assert sorted(got_bad) == ['img1_0.0.jpg', 'img3_0.0.jpg', 'img5_0.1.jpg']
    assert got_good['img2_0.7.jpg'] == _expected_file(gallery, 2, score_thr=0.3)       # its 0.2 detection is not drawn
    assert got_good['img2_0.7.jpg'] != _expected_file(gallery, 2)
    assert got_bad['img5_0.1.jpg'] == _expected_file(gallery, 5, score_thr=0.3)


def test_a_callable_eval_fn_is_honoured(gallery, tmp_path):
    seen = []

    def by_detections(result, ann):
        seen.append((sum(len(r) for r in result), len(ann['labels'])))
        return float(sum(len(r) for r in result))                                       # 1, 0, 2, 1, 1, 1
    good, bad = pkg.ResultVisualizer().evaluate_and_show(gallery['data'], gallery['results'], topk=1,
                                                         show_dir=str(tmp_path / 'w'), eval_fn=by_detections)
    assert seen == [(1, 1), (0, 1), (2, 1), (1, 0), (1, 1), (1, 1)]
    assert bad == [(1, 0.0)] and good == [(2, 2.0)]
    assert sorted(_files(tmp_path / 'w' / 'bad')) == ['img1_0.0.jpg'] and sorted(_files(tmp_path / 'w' / 'good')) == ['img2_2.0.jpg']
    assert _files(tmp_path / 'w' / 'good')['img2_2.0.jpg'] == _expected_file(gallery, 2)


def test_flat_results_and_a_cached_map_gt(gallery, tmp_path):
    data = gallery['data']
    data.map_gt = pkg.MapGt(gallery['annos'], len(CLASSES))
    try:
        good, bad = pkg.ResultVisualizer().evaluate_and_show(data, pkg.flatten_results(gallery['results']), topk=2,
                                                             show_dir=str(tmp_path / 'w'))
    finally:
        del data.map_gt
    assert [i for i, _ in bad] == [1, 3] and [i for i, _ in good] == [0, 4]
    assert _files(tmp_path / 'w' / 'good')['img4_1.0.jpg'] == _expected_file(gallery, 4)


def test_the_tool_over_a_coco_set(gallery, tmp_path):
    images = [dict(id=100 + k, file_name=f'img{k}.jpg', width=w, height=h) for k, (h, w) in enumerate(SIZES)]
    anns = [dict(id=k + 1, image_id=100 + k, category_id=10 * (cls + 1), bbox=[GT[0], GT[1], GT[2] - GT[0], GT[3] - GT[1]],
                 area=(GT[2] - GT[0]) * (GT[3] - GT[1]), iscrowd=0) for k, (cls, _) in enumerate(CASES) if cls is not None]
    cats = [dict(id=10 * (c + 1), name=n) for c, n in enumerate(CLASSES)]
    ann_file, pkl = tmp_path / 'ann.json', tmp_path / 'results.pkl'
    ann_file.write_text(json.dumps(dict(images=images, annotations=anns, categories=cats)))
    pkl.write_bytes(pickle.dumps(gallery['results']))
    spec = importlib.util.spec_from_file_location('tool_analyze_results', os.path.join(ROOT, 'tools', 'analyze_results.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    good, bad = tool.main([str(ann_file), gallery['src'], str(pkl), str(tmp_path / 'show'), '--topk', '2', '--classes', *CLASSES])
    assert [i for i, _ in bad] == [1, 3] and [i for i, _ in good] == [0, 4]
    assert sorted(os.listdir(tmp_path / 'show' / 'good')) == ['img0_1.0.jpg', 'img4_1.0.jpg']
    got = _files(tmp_path / 'show' / 'bad')
    assert sorted(got) == ['img1_0.0.jpg', 'img3_0.0.jpg']
    assert got['img3_0.0.jpg'] == _expected_file(gallery, 3)
    assert A.clip_topk(5, len(SIZES)) == 3
