"""Writes the cases of tests/golden/jpeg_encode.npz as files: ``python tools/jpeg_encode_fixtures_dump.py DIR`` (the
input of tools/jpeg_encode_sanitize.cpp, the stand-alone sanitizer run of the encoder's host code).  A ``.bin`` file is
seven int32 -- height, width, channels, quality, hs, vs, file length -- then the pixels, then libjpeg-turbo's file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLINGS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'gray': (1, 1)}


def main(out):
    os.makedirs(out, exist_ok=True)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_encode.npz'))
    for n in g['names']:
        src, jpg = g['src_' + n], g['jpg_' + n]
        parts = str(n).split('_')
        hs, vs = SAMPLINGS[parts[1]]
        head = np.array([src.shape[0], src.shape[1], 1 if src.ndim == 2 else 3, int(parts[-1][1:]), hs, vs, jpg.size], np.int32)
        with open(os.path.join(out, f'{n}.bin'), 'wb') as f:
            f.write(head.tobytes() + np.ascontiguousarray(src).tobytes() + jpg.tobytes())
    print(f"{len(g['names'])} files -> {out}")


if __name__ == '__main__':
    main(sys.argv[1])
