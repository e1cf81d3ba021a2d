"""Writes the JPEG byte strings of tests/golden/jpeg.npz, jpeg_entropy.npz, jpeg_exif.npz and jpeg_synth.npz as files:
``python tools/jpeg_fixtures_dump.py DIR`` (the input of tools/jpeg_sanitize.cpp and tools/jpeg_entropy_sanitize.cpp, the
stand-alone sanitizer runs of the decoder's host code)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(out):
    os.makedirs(out, exist_ok=True)
    count = 0
    for fixture, lists in (('jpeg.npz', ('names', 'refused')), ('jpeg_entropy.npz', ('names', 'damaged')),
                           ('jpeg_exif.npz', ('names',)), ('jpeg_synth.npz', ('names', 'invalid'))):
        g = np.load(os.path.join(ROOT, 'tests', 'golden', fixture))
        for n in (n for key in lists for n in g[key]):
            with open(os.path.join(out, f'{n}.jpg'), 'wb') as f:
                f.write(g['jpg_' + n].tobytes())
            count += 1
    print(f'{count} files -> {out}')


if __name__ == '__main__':
    main(sys.argv[1])
