"""Writes the JPEG byte strings of tests/golden/jpeg.npz as files: ``python tools/jpeg_fixtures_dump.py DIR``
(the input of tools/jpeg_sanitize.cpp, the stand-alone sanitizer run of the decoder's host half)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(out):
    os.makedirs(out, exist_ok=True)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg.npz'))
    names = list(g['names']) + list(g['refused'])
    for n in names:
        with open(os.path.join(out, f'{n}.jpg'), 'wb') as f:
            f.write(g['jpg_' + n].tobytes())
    print(f'{len(names)} files -> {out}')


if __name__ == '__main__':
    main(sys.argv[1])
