"""Writes tests/golden/jpeg.npz: JPEG byte strings and libjpeg-turbo's decode of them (through Pillow).

Run in the build container only (``python tests/golden/make_golden_jpeg.py``); the tests read the .npz and never need
Pillow.  Per case ``jpg_<name>`` holds the file's bytes and ``rgb_<name>`` Pillow's (h, w, 3) RGB decode (a grayscale
file's plane three times, as ``flag='color'`` gives it); ``names`` lists the cases, ``refused`` the files the decoder
must refuse (``jpg_<name>`` only).  The cases are the smallest at which each rule of the decode can go wrong: one
pixel, one block, sizes that are no multiple of the MCU in either direction, more than one MCU row and column, each
sampling, restart intervals, optimised Huffman tables, coarse tables, and quality-100 noise (all-ones tables: the
largest coefficients an encoder writes).
"""
import io
import os

import numpy as np
from PIL import Image, features

SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (37, 53), (40, 72), (48, 64)]      # (h, w)
SAMPLINGS = {'444': 0, '422': 1, '420': 2, 'gray': None}


def picture(h, w, kind, seed):
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, w, 3))
    if kind == 'noise':
        return noise.astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 255 * (xx + yy) / max(h + w - 2, 1)], -1)
    return np.clip(grad + (noise - 128) * 0.15, 0, 255).astype(np.uint8)


def encode(rgb, sampling, **kw):
    buf = io.BytesIO()
    if SAMPLINGS[sampling] is None:
        Image.fromarray(rgb).convert('L').save(buf, 'JPEG', **kw)
    else:
        Image.fromarray(rgb).save(buf, 'JPEG', subsampling=SAMPLINGS[sampling], **kw)
    return buf.getvalue()


def decoded(data):
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else a


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'
    out, names, seed = {}, [], 0

    def add(name, data):
        names.append(name)
        out['jpg_' + name] = np.frombuffer(data, np.uint8)
        out['rgb_' + name] = decoded(data)

    for h, w in SIZES:
        for samp in SAMPLINGS:
            for kind in ('grad', 'noise'):
                seed += 1
                add(f'{h}x{w}_{samp}_{kind}_q90', encode(picture(h, w, kind, seed), samp, quality=90))
    for h, w in ((17, 33), (37, 53), (48, 64)):
        seed += 1
        add(f'{h}x{w}_420_grad_q90_rst2', encode(picture(h, w, 'grad', seed), '420', quality=90, restart_marker_blocks=2))
    for samp in SAMPLINGS:
        seed += 1
        add(f'37x53_{samp}_grad_q30_opt', encode(picture(37, 53, 'grad', seed), samp, quality=30, optimize=True))
        for h, w in ((17, 33), (48, 64)):
            seed += 1
            add(f'{h}x{w}_{samp}_noise_q100', encode(picture(h, w, 'noise', seed), samp, quality=100))
    refused = []
    seed += 1
    out['jpg_progressive'] = np.frombuffer(encode(picture(17, 33, 'grad', seed), '420', quality=90, progressive=True), np.uint8)
    buf = io.BytesIO()
    Image.fromarray(picture(17, 33, 'grad', seed)).convert('CMYK').save(buf, 'JPEG', quality=90)
    out['jpg_cmyk'] = np.frombuffer(buf.getvalue(), np.uint8)
    refused += ['progressive', 'cmyk']
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg.npz')
    np.savez_compressed(path, names=np.array(names), refused=np.array(refused), **out)
    print(f'{len(names)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
    main()
