"""Hand-made drawing cases shared by the host and GPU tests: each ``(image, dets, labels, class names, style)``."""
import numpy as np

NAMES = ['person', 'bicycle', 'car', 'tr\xe4in\n', 'a name that is much longer than thirty-one characters']
ALL_GLYPHS = [bytes(range(0x20 + 19 * k, min(0x20 + 19 * k + 19, 0x7F))).decode() for k in range(5)]


def image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def cases():
    out = {}
    d = np.array
    out['clipped_left_top'] = (image(40, 60, 1), d([[-10.5, -7.2, 25.9, 20.1, 0.9]], np.float32), [0], NAMES, {})
    out['clipped_right_bottom'] = (image(40, 60, 2), d([[30.0, 18.0, 90.0, 70.0, 0.55]], np.float32), [2], NAMES, {})
    out['outside'] = (image(20, 20, 3), d([[40.0, 40.0, 50.0, 50.0, 0.9], [-30.0, -30.0, -5.0, -5.0, 0.9]], np.float32),
                      [0, 1], NAMES, {})
    out['thick_box'] = (image(30, 80, 4), d([[50.0, 2.0, 56.0, 25.0, 0.8]], np.float32), [1], NAMES, dict(thickness=9))
    out['later_wins'] = (image(64, 96, 5), d([[5.0, 5.0, 60.0, 40.0, 0.7], [20.0, 8.0, 90.0, 60.0, 0.8]], np.float32),
                         [0, 2], NAMES, dict(bbox_color='green', text_color=(1, 2, 3)))
    out['at_threshold'] = (image(32, 48, 6), d([[4.0, 4.0, 40.0, 28.0, 0.3], [6.0, 6.0, 30.0, 20.0, 0.30000004]],
                                               np.float32), [0, 1], NAMES, {})
    out['scaled_font'] = (image(50, 200, 7), d([[3.0, 3.0, 190.0, 45.0, 0.995]], np.float32), [2], NAMES,
                          dict(font_size=21, thickness=1, text_color='white'))
    out['names'] = (image(60, 260, 8), d([[0.0, 0.0, 250.0, 20.0, 1.0], [0.0, 25.0, 250.0, 50.0, 0.004],
                                          [5.0, 40.0, 100.0, 58.0, 0.5]], np.float32), [3, 4, 7], NAMES, dict(score_thr=0.0))
    k = len(ALL_GLYPHS)
    out['all_glyphs'] = (image(12 * k, 160, 9), d([[0.0, 12.0 * i, 159.0, 12.0 * i + 10, 0.87] for i in range(k)], np.float32),
                         list(range(k)), ALL_GLYPHS, dict(font_size=7, thickness=1))
    out['degenerate'] = (image(24, 24, 10), d([[10.0, 10.0, 5.0, 5.0, 0.9], [3.0, 3.0, 3.0, 3.0, 0.9]], np.float32), [0, 0],
                         NAMES, {})
    return out


def batch():
    """Three images of different sizes with 0, 1 and 40 boxes."""
    rng = np.random.default_rng(11)
    imgs = [image(33, 47, 12), image(64, 80, 13), image(120, 200, 14)]
    xy = rng.uniform(-20, 180, (40, 2)).astype(np.float32)
    wh = rng.uniform(2, 90, (40, 2)).astype(np.float32)
    many = np.concatenate([xy, xy + wh, rng.uniform(0, 1, (40, 1)).astype(np.float32)], 1)
    dets = [np.zeros((0, 5), np.float32), np.array([[10.0, 12.0, 50.0, 40.0, 0.66]], np.float32), many]
    labels = [np.zeros(0, np.int64), np.array([1]), rng.integers(0, 5, 40)]
    return imgs, dets, labels
