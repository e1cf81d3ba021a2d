"""Writes tests/golden/jpeg_encode.npz: pixels and the JPEG file libjpeg-turbo (through Pillow) encodes them to.

Run in the build container only (``python tests/golden/make_golden_jpeg_encode.py``); the tests read the .npz and never
need Pillow.  Per case ``src_<name>`` holds the pixels given to Pillow ((h, w, 3) RGB, for gray the (h, w) plane) and
``jpg_<name>`` Pillow's file; ``names`` lists the cases, ``<size>_<sampling>_<kind>_q<quality>``.  The cases are the
smallest at which each rule of the encode can go wrong: make_golden_jpeg.py's sizes in every sampling, every quality
regime of the table scaling, strips one or two pixels wide (dummy block columns and rows in every position), a saturated
checkerboard (the largest coefficients), and one 918-block noise file whose scan is long and full of stuffed bytes.  The
maker asserts, through the numpy restatement of the encoder (tests/_jpeg_enc_ref.py), that every pad length, a ZRL, a
stuffed byte and a block with a nonzero last coefficient occur -- and that the restatement gives Pillow's bytes.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import _jpeg_enc_ref as E      # noqa: E402
from make_golden_jpeg import SAMPLINGS, SIZES, picture      # noqa: E402


def source(h, w, kind, seed, sampling):
    if kind == 'checker':
        yy, xx = np.mgrid[0:h, 0:w]
        rgb = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    else:
        rgb = picture(h, w, kind, seed)
    return np.ascontiguousarray(np.asarray(Image.fromarray(rgb).convert('L'))) if sampling == 'gray' else rgb


def pillow(src, sampling, quality):
    buf = io.BytesIO()
    if sampling == 'gray':
        Image.fromarray(src, 'L').save(buf, 'JPEG', quality=quality)
    else:
        Image.fromarray(src).save(buf, 'JPEG', quality=quality, subsampling=SAMPLINGS[sampling])
    return buf.getvalue()


def cases():
    seed = 1000
    for h, w in SIZES:
        for samp in SAMPLINGS:
            for kind in ('grad', 'noise'):
                seed += 1
                yield h, w, samp, kind, 90, seed
    for h, w in ((37, 53), (48, 64)):
        for samp in SAMPLINGS:
            for q in (1, 30, 50, 75, 95, 100):
                seed += 1
                yield h, w, samp, 'noise' if q in (1, 100) else 'grad', q, seed
    for h, w in ((2, 65), (33, 1), (23, 130)):
        for samp in SAMPLINGS:
            seed += 1
            yield h, w, samp, 'grad', 90, seed
    for samp in SAMPLINGS:
        yield 16, 16, samp, 'checker', 100, 0
    yield 136, 264, '420', 'noise', 100, seed + 1


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'
    out, names = {}, []
    pads, zrl, stuffed, last63 = set(), 0, 0, 0
    for h, w, samp, kind, q, seed in cases():
        name = f'{h}x{w}_{samp}_{kind}_q{q}'
        assert name not in names, name
        src = source(h, w, kind, seed, samp)
        jpg = pillow(src, samp, q)
        stats = {}
        assert E.encode(src, q, samp, 'rgb', stats) == jpg, f'{name}: the restatement and Pillow differ'
        pads.add(stats['pad'])
        zrl += stats['zrl']
        stuffed += stats['stuffed']
        last63 += stats['last63']
        names.append(name)
        out['src_' + name] = src
        out['jpg_' + name] = np.frombuffer(jpg, np.uint8)
    assert pads == set(range(8)), f'pad lengths {sorted(pads)}'
    assert zrl and stuffed and last63, (zrl, stuffed, last63)
    out['names'] = np.array(names)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_encode.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f'{len(names)} cases, {size} bytes; pads {sorted(pads)}, {zrl} ZRL, {stuffed} stuffed bytes, {last63} blocks '
          'with a nonzero coefficient 63')


if __name__ == '__main__':
    main()
