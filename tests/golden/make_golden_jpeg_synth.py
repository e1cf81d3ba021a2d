"""Writes tests/golden/jpeg_synth.npz: the synthetic streams of ``tests/_jpeg_synth.py`` and libjpeg-turbo's decode of
them (through Pillow).

Run in the build container only (``python tests/golden/make_golden_jpeg_synth.py``); the tests read the .npz and never
need Pillow.  ``names`` lists the valid cases and ``invalid`` the three files that must not decode; ``jpg_<name>`` holds a
file's bytes, ``rgb_<name>`` Pillow's (h, w, 3) RGB decode.  Pixels are recorded only where every sample of the
restatement's IDCT, before the range limit, lies in -512 <= v < 512 and every dequantised coefficient fits 16 bits:
outside that range libjpeg-turbo's SIMD code saturates where this decoder (and ``_jpeg_ref.py``) wraps, so those cases,
listed under ``unpinned_pixels``, are held to the restatement only.  Inside the range a difference between Pillow and
the restatement stops the script: it would be a finding, not a fixture.
"""
import os
import sys

import numpy as np
from PIL import features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _jpeg_ref as R      # noqa: E402
import _jpeg_synth as S      # noqa: E402
from make_golden_jpeg import decoded      # noqa: E402


def in_range(info, coef):
    """Whether libjpeg-turbo and the restatement have to agree on this file: no sample leaves the range limit table's
    unambiguous half, no dequantised coefficient leaves int16."""
    off = 0
    for i in range(info['ncomp']):
        n = 64 * info['blocks_h'][i] * info['blocks_w'][i]
        x = coef[off:off + n].reshape(-1, 8, 8).astype(np.int32) * info['quant'][info['tq'][i]].reshape(8, 8).astype(np.int32)
        off += n
        if np.abs(x).max() > 32767:
            return False
        ws = (R._idct8(x.transpose(1, 2, 0)) + np.int32(1024)) >> 11
        v = (R._idct8(ws.transpose(1, 0, 2)) + np.int32(1 << 17)) >> 18
        if v.min() < -512 or v.max() >= 512:
            return False
    return True


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'
    out, names, unpinned = {}, [], []
    for name in S.CASES:
        data, expected, _ = S.make(name)
        info, coef = R.entropy_decode(data)
        assert np.array_equal(coef, expected), name
        names.append(name)
        out['jpg_' + name] = np.frombuffer(data, np.uint8)
        if in_range(info, coef):
            rgb = decoded(data)
            assert np.array_equal(rgb, R.decode(data, 'rgb')), f'{name}: libjpeg-turbo and the restatement differ'
            out['rgb_' + name] = rgb
        else:
            unpinned.append(name)
    for name in S.INVALID:
        out['jpg_' + name] = np.frombuffer(S.make(name)[0], np.uint8)
    path = os.path.join(HERE, 'jpeg_synth.npz')
    np.savez_compressed(path, names=np.array(names), invalid=np.array(list(S.INVALID)), unpinned_pixels=np.array(unpinned),
                        **out)
    print(f'{len(names)} valid cases ({len(unpinned)} without pixels: {", ".join(unpinned)}) and {len(S.INVALID)} invalid '
          f'ones, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
    main()
