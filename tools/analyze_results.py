#!/usr/bin/env python
"""Rank the images of a COCO-format test set by their per-image mAP and write the best and the worst, ground truth and
detections drawn, into show_dir/good and show_dir/bad (the reference's tools/analysis_tools/analyze_results.py).
Usage (GPU box):   python tools/analyze_results.py ANN_FILE IMG_PREFIX PREDICTION.pkl SHOW_DIR [--topk 20]
                       [--show-score-thr 0] [--classes NAME ...]
PREDICTION.pkl: the pickled results of a test run, per image the per-class list of (n, 5) arrays, images in the order of
the annotation file.  The reference takes a config file and builds the test dataset from it; here the two values of it
that matter, the annotation file and the image directory, are the arguments, and the dataset is
``CocoDataset(test_mode=True)``.  Every image is scored in one device pass (``image_maps``); the sources are decoded,
drawn on and encoded on the GPU, one batch per directory.  There is no display (no --show)."""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='per-image mAP of a test run: the good / bad gallery')
    ap.add_argument('ann_file', help='COCO-format annotation file of the test set')
    ap.add_argument('img_prefix', help='directory of the images (JPEG)')
    ap.add_argument('prediction_path', help='pickled test results')
    ap.add_argument('show_dir', help='where good/ and bad/ are written')
    ap.add_argument('--topk', default=20, type=int, help='number of best and of worst images saved')
    ap.add_argument('--show-score-thr', type=float, default=0, help='score threshold of the detections drawn (default: 0.)')
    ap.add_argument('--classes', nargs='+', default=None, help='class names (default: the 80 COCO names)')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not os.path.isfile(args.prediction_path):
        raise FileNotFoundError(f'no prediction file at {args.prediction_path!r}')
    from mmdet_yolov4_amd import CocoDataset, ResultVisualizer
    dataset = CocoDataset(args.ann_file, classes=args.classes, img_prefix=args.img_prefix, test_mode=True)
    with open(args.prediction_path, 'rb') as f:
        outputs = pickle.load(f)
    if len(outputs) != len(dataset):
        raise ValueError(f'{args.prediction_path} holds {len(outputs)} results, {args.ann_file} {len(dataset)} images')
    good, bad = ResultVisualizer(False, 0, args.show_score_thr).evaluate_and_show(dataset, outputs, topk=args.topk,
                                                                                  show_dir=args.show_dir)
    print(f'{len(good)} good and {len(bad)} bad images written under {os.path.abspath(args.show_dir)}')
    return good, bad


if __name__ == '__main__':
    main()
