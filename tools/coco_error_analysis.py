#!/usr/bin/env python
"""COCO error analysis: the C75 / C50 / Loc / Sim / Oth / BG / FN breakdown of a bbox result file, with the arguments of
the reference's tools/analysis_tools/coco_error_analysis.py.
Usage (GPU box):  python tools/coco_error_analysis.py RESULT OUT_DIR --ann ANNOTATIONS [--extraplots] [--areas A0 A1 A2]
RESULT: a bbox .json as results2json writes it, or the .pkl of a test loop.  The analysis is one pass on the device
(mmdet_yolov4_amd.coco_error).  Writes OUT_DIR/bbox/error_analysis.npz (ps, rec_thrs, cat_ids, names, counts, area_rng,
aps) and OUT_DIR/bbox/error_analysis.txt (the table of every class and of "allclass"); with matplotlib installed also
the reference's figures, one per class and area range, and with --extraplots the bar plots, the number of annotations per
area group and the histogram of the annotation areas.  Without matplotlib one line says that the figures were skipped.
The K axis is the sorted category ids and every class is labelled by its own name."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ('C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN')
AREA_NAMES = ('allarea', 'small', 'medium', 'large')
AREA_LABELS = ('all', 'small', 'medium', 'large')
# the fill colour of each type's band: white for the two strict thresholds, then the reference's palette
COLORS = ((1, 1, 1), (1, 1, 1), (0.31, 0.51, 0.74), (0.75, 0.31, 0.30), (0.36, 0.90, 0.38), (0.50, 0.39, 0.64), (1, 0.6, 0))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='COCO Error Analysis Tool')
    parser.add_argument('result', help='result file (bbox json, or the pkl of a test loop) path')
    parser.add_argument('out_dir', help='dir to save analyze result images')
    parser.add_argument('--ann', default='data/coco/annotations/instances_val2017.json', help='annotation file path')
    parser.add_argument('--types', type=str, nargs='+', default=['bbox'], help='result types')
    parser.add_argument('--extraplots', action='store_true', help='export extra bar/stat plots')
    parser.add_argument('--areas', type=int, nargs='+', default=[1024, 9216, 10000000000], help='area regions')
    args = parser.parse_args(argv)
    for res_type in args.types:
        if res_type == 'segm':
            parser.error("--types segm is not built: it scores masks, which no detector of this package produces; "
                         "only 'bbox' is")
        if res_type != 'bbox':
            parser.error(f'--types {res_type}: bbox or segm')
    if len(args.areas) != 3:
        parser.error('3 integers should be specified as areas, representing 3 area regions')
    return args


def pyplot():
    """matplotlib.pyplot on the Agg backend, or None when matplotlib is not installed."""
    try:
        import matplotlib
    except ImportError:
        return None
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    return plt


def makeplot(plt, rs, ps, out_dir, class_name, iou_type='bbox'):
    """One stacked precision-recall figure per area range.  ``ps`` (7, R, A, 1) of a class or (7, R, K, A, 1)."""
    written = []
    for a, area_name in enumerate(AREA_NAMES):
        title = f'{iou_type}-{class_name}-{area_name}'
        area_ps = ps[..., a, 0]
        aps = [p.mean() for p in area_ps]
        curves = [np.zeros(len(rs))] + [p.mean(axis=1) if p.ndim > 1 else p for p in area_ps]
        fig = plt.figure()
        ax = plt.subplot(111)
        for t, name in enumerate(TYPES):
            ax.plot(rs, curves[t + 1], color=[0, 0, 0], linewidth=0.5)
            ax.fill_between(rs, curves[t], curves[t + 1], color=COLORS[t], label=f'[{aps[t]:.3f}]{name}')
        plt.xlabel('recall')
        plt.ylabel('precision')
        plt.xlim(0, 1.0)
        plt.ylim(0, 1.0)
        plt.title(title)
        plt.legend()
        written.append(os.path.join(out_dir, f'{title}.png'))
        fig.savefig(written[-1])
        plt.close(fig)
    return written


def _label_bars(ax, rects):
    for rect in rects:
        height = rect.get_height()
        text = f'{height * 100:2.0f}' if 0 < height <= 1 else f'{height:2.0f}'
        ax.annotate(text, xy=(rect.get_x() + rect.get_width() / 2, height), xytext=(0, 3), textcoords='offset points',
                    ha='center', va='bottom', fontsize='x-small')


def makebarplot(plt, rs, ps, out_dir, class_name, iou_type='bbox'):
    """The six APs (FN left out) per area range as grouped bars."""
    title = f'{iou_type}-{class_name}-ap bar plot'
    fig, ax = plt.subplots()
    x = np.arange(len(AREA_NAMES))
    width = 0.60
    bars = []
    for t, name in enumerate(TYPES[:-1]):
        aps = [p.mean() for p in ps[t, ..., 0].T]
        bars.append(ax.bar(x - width / 2 + (t + 1) * width / len(TYPES), aps, width / len(TYPES), label=name))
    ax.set_ylabel('Mean Average Precision (mAP)')
    ax.set_title(title)
    ax.set_xticks(x)
    ax.set_xticklabels(AREA_NAMES)
    ax.legend()
    for rects in bars:
        _label_bars(ax, rects)
    path = os.path.join(out_dir, f'{title}.png')
    fig.savefig(path)
    plt.close(fig)
    return path


def make_gt_area_group_numbers_plot(plt, counts, out_dir, verbose=True):
    """``counts`` (K, A): the ground truths that count per category and area range (``ErrorAnalysis.counts``)."""
    numbers = dict(zip(AREA_LABELS, (int(v) for v in np.asarray(counts).sum(axis=0))))
    if verbose:
        print('number of annotations per area group:', numbers)
    title = 'number of annotations per area group'
    fig, ax = plt.subplots()
    x = np.arange(len(numbers))
    rects = ax.bar(x, list(numbers.values()), 0.60)
    ax.set_ylabel('Number of annotations')
    ax.set_title(title)
    ax.set_xticks(x)
    ax.set_xticklabels(list(numbers))
    _label_bars(ax, rects)
    fig.tight_layout()
    path = os.path.join(out_dir, f'{title}.png')
    fig.savefig(path)
    plt.close(fig)
    return path


def make_gt_area_histogram_plot(plt, areas, out_dir):
    title = 'gt annotation areas histogram plot'
    fig, ax = plt.subplots()
    ax.hist(np.sqrt(np.asarray(areas, dtype=np.float64)), bins=100)
    ax.set_xlabel('Squareroot Area')
    ax.set_ylabel('Number of annotations')
    ax.set_title(title)
    fig.tight_layout()
    path = os.path.join(out_dir, f'{title}.png')
    fig.savefig(path)
    plt.close(fig)
    return path


def write_outputs(res, out_dir, extraplots=False, gt_areas=(), plt='auto'):
    """The arrays, the tables and -- with matplotlib -- the figures of an ``ErrorAnalysis``-like ``res`` (``ps``,
    ``rec_thrs``, ``cat_ids``, ``names``, ``counts``, ``area_rng``, ``aps``, ``table``) into ``out_dir``."""
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, 'error_analysis.npz'), ps=res.ps, rec_thrs=res.rec_thrs, cat_ids=np.asarray(res.cat_ids),
             names=np.asarray(res.names), counts=res.counts, area_rng=res.area_rng, aps=res.aps(),
             aps_per_class=np.stack([res.aps(k) for k in range(len(res.cat_ids))]))
    with open(os.path.join(out_dir, 'error_analysis.txt'), 'w') as f:
        for k in range(len(res.cat_ids)):
            f.write(res.table(k) + '\n\n')
        f.write(res.table() + '\n')
    if plt == 'auto':
        plt = pyplot()
    if plt is None:
        print('matplotlib is not installed: the figures were skipped (the arrays and tables are written)')
        return []
    written = []
    for k, name in enumerate(res.names):
        written += makeplot(plt, res.rec_thrs, res.ps[:, :, k], out_dir, name)
        if extraplots:
            written.append(makebarplot(plt, res.rec_thrs, res.ps[:, :, k], out_dir, name))
    written += makeplot(plt, res.rec_thrs, res.ps, out_dir, 'allclass')
    if extraplots:
        written.append(makebarplot(plt, res.rec_thrs, res.ps, out_dir, 'allclass'))
        written.append(make_gt_area_group_numbers_plot(plt, res.counts, out_dir))
        written.append(make_gt_area_histogram_plot(plt, gt_areas, out_dir))
    return written


def analyze_results(res_file, ann_file, res_types, out_dir, extraplots=None, areas=None):
    from mmdet_yolov4_amd import CocoGt, error_analysis
    coco_gt = CocoGt(ann_file)
    for res_type in res_types:
        res = error_analysis(coco_gt, res_file, areas=areas, iou_type=res_type)
        write_outputs(res, os.path.join(out_dir, res_type), extraplots=bool(extraplots), gt_areas=coco_gt.ann_area)
        print(res.table())


def main(argv=None):
    args = parse_args(argv)
    analyze_results(args.result, args.ann, args.types, out_dir=args.out_dir, extraplots=args.extraplots, areas=args.areas)


if __name__ == '__main__':
    main()
