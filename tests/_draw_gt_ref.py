"""Boxes without a score, as ground truth is drawn: what ``draw_boxes`` is held to for ``(k, 4)`` boxes
(``YV4_DRAW_NO_SCORE``), bit for bit.

``_draw_ref``'s rule with two differences, which are the reference's (``imshow_det_bboxes`` writes ``|score`` only when a
box has a fifth column, and filters by score only then): the label is the class name alone, and no box is skipped,
whatever ``score_thr`` is.  ``draw_gt_det`` is the picture of ``imshow_gt_det_bboxes``: the ground truth, then the
detections over it.
"""
import numpy as np

from _draw_ref import COLORS, clean_name, draw, text_mask


def draw_gt(img, boxes, labels, class_names, bbox_color=(72, 101, 241), text_color=(72, 101, 241), thickness=2,
            font_size=13, score_thr=None):
    """(h, w, 3) uint8, (k, 4) float32, (k,) int -> the drawn copy.  ``score_thr`` is accepted and has no effect."""
    out = np.array(img, np.uint8, copy=True)
    h, w = out.shape[:2]
    scale = max(1, font_size // 7)
    bbox_color = COLORS.get(bbox_color, bbox_color) if isinstance(bbox_color, str) else bbox_color
    text_color = COLORS.get(text_color, text_color) if isinstance(text_color, str) else text_color
    yy, xx = np.mgrid[0:h, 0:w]
    for b, lab in zip(np.asarray(boxes, np.float32).reshape(-1, 4), labels):
        x1, y1, x2, y2 = (int(v) for v in b.astype(np.int32))
        inside = (xx >= x1) & (xx <= x2) & (yy >= y1) & (yy <= y2)
        frame = inside & ((xx - x1 < thickness) | (x2 - xx < thickness) | (yy - y1 < thickness) | (y2 - yy < thickness))
        out[frame] = bbox_color
        name = class_names[lab] if 0 <= lab < len(class_names) else '?'
        mask = text_mask(clean_name(name), scale)                  # the name alone: no '|', no score
        for my in range(mask.shape[0]):
            for mx in range(mask.shape[1]):
                y, x = y1 + my, x1 + mx
                if 0 <= y < h and 0 <= x < w:
                    out[y, x] = text_color if mask[my, mx] else img[y, x] // 5
    return out


def draw_gt_det(img, gt_boxes, gt_labels, dets, det_labels, class_names, score_thr=0, gt_bbox_color=(255, 102, 61),
                gt_text_color=(255, 102, 61), det_bbox_color=(72, 101, 241), det_text_color=(72, 101, 241), thickness=2,
                font_size=13):
    """Two successive draws: the ground truth, then the detections with a score above ``score_thr`` on that picture."""
    first = draw_gt(img, gt_boxes, gt_labels, class_names, gt_bbox_color, gt_text_color, thickness, font_size)
    return draw(first, dets, det_labels, class_names, score_thr=score_thr, bbox_color=det_bbox_color,
                text_color=det_text_color, thickness=thickness, font_size=font_size)
