"""Cases of boxes without a score, shared by the host and GPU tests: ``_draw_data``'s cases with the score column cut
off, and three of their own.  Each ``(image, boxes (k, 4), labels, class names, style)``."""
import numpy as np

import _draw_data as D


def cases():
    out = {}
    for name, (img, dets, labels, names, style) in D.cases().items():
        style = {k: v for k, v in style.items() if k != 'score_thr'}
        out[name] = (img, np.ascontiguousarray(dets[:, :4]), labels, names, style)
    b = np.array
    # partly outside the image on every side, a label outside the classes, thickness 1 and 3
    out['partly_outside'] = (D.image(48, 64, 21), b([[-8.0, 30.0, 20.0, 60.0], [50.0, -6.0, 80.0, 12.0]], np.float32), [1, 2],
                             D.NAMES, {})
    out['label_outside_classes'] = (D.image(40, 72, 22), b([[4.0, 4.0, 60.0, 30.0], [10.0, 20.0, 70.0, 38.0]], np.float32),
                                    [len(D.NAMES), -1], D.NAMES, dict(thickness=1))
    out['thickness_3'] = (D.image(40, 72, 23), b([[6.5, 5.5, 64.9, 33.2]], np.float32), [0], D.NAMES,
                          dict(thickness=3, bbox_color=(255, 102, 61), text_color=(255, 102, 61)))
    return out
