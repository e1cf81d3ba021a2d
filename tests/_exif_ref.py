"""The EXIF orientation table of include/yv4.h ("baseline JPEG decoding", yv4_jpeg_image.orientation) in numpy: what the
pixel stage writes for a decoded picture ``D`` (h, w, ...) under orientation 0 .. 8.  Written index by index from the
table, not with ``np.rot90`` / ``np.flip``, so that it checks the table itself against Pillow's ``exif_transpose``
(tests/test_jpeg_exif_host.py) and the kernel against the table (tests/test_gpu_jpeg_exif.py)."""
import numpy as np


def orient(D, o):
    D = np.asarray(D)
    h, w = D.shape[:2]
    if o in (0, 1):
        return D.copy()
    H, W = (w, h) if o >= 5 else (h, w)
    y, x = np.mgrid[0:H, 0:W]
    sy, sx = {2: (y, w - 1 - x), 3: (h - 1 - y, w - 1 - x), 4: (h - 1 - y, x), 5: (x, y), 6: (h - 1 - x, y),
              7: (h - 1 - x, w - 1 - y), 8: (x, w - 1 - y)}[o]
    return np.ascontiguousarray(D[sy, sx])
