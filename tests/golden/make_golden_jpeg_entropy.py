"""Writes tests/golden/jpeg_entropy.npz: the files that exercise the segment-parallel Huffman decode.

Run in the build container only (``python tests/golden/make_golden_jpeg_entropy.py``, after the library is built); the
tests read the .npz and never need Pillow.  Layout as in jpeg.npz: ``jpg_<name>`` / ``rgb_<name>`` per valid case
(``names``), and per damaged case (``damaged``) ``jpg_<name>`` and ``status_<name>``, the status class the HOST decoder
(``yv4_jpeg_entropy_decode``, the oracle) returned for it when the fixture was made.

  72x80_444_grad_q90_rst1     restart interval 1: 90 segments -- more than one workgroup of 64, and the marker counter
                              wraps past 7 eleven times
  72x80_420_grad_q90_rst1     25 segments of six blocks
  72x80_444_noise_q100_rst1   all-ones tables over black-and-white noise: stuffed FF00 pairs, long codes, 10-bit
                              magnitudes
  8x8_gray_block_q90          a single block, no restart interval
  72x80_444_grad_q90_rst1_fill   the first file with two 0xFF fill bytes in front of marker 37: valid
  swapped / removed / cut_mid / cut_last / inserted
                              the first file with markers 20 and 21 exchanged, marker 30 taken out, cut in the middle of
                              segment 40, cut in the middle of the last segment, and one data byte put in front of
                              marker 50
"""
import ctypes
import os
import sys

import numpy as np
from PIL import features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from make_golden_jpeg import decoded, encode, picture      # noqa: E402


def markers(data, scan):
    """Offsets of the RSTn markers behind ``scan``: inside entropy-coded data 0xFF is followed by 0x00 or a marker."""
    return [i for i in range(scan, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def main():
    import mmdet_yolov4_amd as pkg
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'
    L = pkg._lib.lib()
    out, names, damaged = {}, [], []

    def host(data):
        info = pkg._lib.JpegInfo()
        st = L.yv4_jpeg_parse(data, len(data), ctypes.byref(info))
        assert st == 0
        coef = np.empty(int(info.ncoef), np.int16)
        return L.yv4_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, coef.size), info

    def add(name, data, rgb=None):
        assert host(data)[0] == 0, name
        names.append(name)
        out['jpg_' + name] = np.frombuffer(data, np.uint8)
        out['rgb_' + name] = decoded(data) if rgb is None else rgb

    def add_damaged(name, data):
        st = host(data)[0]
        assert st == -1, (name, st)
        damaged.append(name)
        out['jpg_' + name] = np.frombuffer(data, np.uint8)
        out['status_' + name] = np.int32(st)

    first = encode(picture(72, 80, 'grad', 101), '444', quality=90, restart_marker_blocks=1)
    add('72x80_444_grad_q90_rst1', first)
    add('72x80_420_grad_q90_rst1', encode(picture(72, 80, 'grad', 102), '420', quality=90, restart_marker_blocks=1))
    # black-and-white noise, mostly white on the left and mostly black on the right: with all-ones tables the DC terms
    # (never differenced, the interval being one MCU) and the largest AC terms need 10-bit magnitude fields
    rng = np.random.default_rng(103)
    white = rng.random((72, 80, 1)) < np.where(np.arange(80) < 40, 0.9, 0.1)[None, :, None]
    harsh = np.where(white ^ (rng.random((72, 80, 3)) < 0.05), 255, 0).astype(np.uint8)
    add('72x80_444_noise_q100_rst1', encode(harsh, '444', quality=100, restart_marker_blocks=1))
    coef = np.empty(64 * 3 * 90, np.int16)
    info = pkg._lib.JpegInfo()
    assert L.yv4_jpeg_entropy_decode(out['jpg_72x80_444_noise_q100_rst1'].tobytes(), out['jpg_72x80_444_noise_q100_rst1'].size,
                                     ctypes.byref(info), coef.ctypes.data, coef.size) == 0
    assert np.abs(coef).max() >= 512, np.abs(coef).max()
    add('8x8_gray_block_q90', encode(picture(8, 8, 'grad', 104), 'gray', quality=90))
    scan = int(host(first)[1].scan_offset)
    m = markers(first, scan)
    assert len(m) == 89 and [first[i + 1] & 7 for i in m] == [k & 7 for k in range(89)]
    stuffed = sum(first[i] == 0xFF and first[i + 1] == 0 for i in range(scan, len(first) - 1))
    noise = out['jpg_72x80_444_noise_q100_rst1'].tobytes()
    print(f'first file: {len(first)} bytes, {len(m)} markers, {stuffed} stuffed pairs; noise file: {len(noise)} bytes, '
          f'{sum(noise[i] == 0xFF and noise[i + 1] == 0 for i in range(scan, len(noise) - 1))} stuffed pairs')
    add('72x80_444_grad_q90_rst1_fill', first[:m[37]] + b'\xff\xff' + first[m[37]:], rgb=decoded(first))

    b = bytearray(first)
    b[m[20] + 1], b[m[21] + 1] = b[m[21] + 1], b[m[20] + 1]
    add_damaged('swapped', bytes(b))
    add_damaged('removed', first[:m[30]] + first[m[30] + 2:])
    add_damaged('cut_mid', first[:(m[39] + 2 + m[40]) // 2])
    add_damaged('cut_last', first[:(m[88] + 2 + len(first) - 2) // 2])
    add_damaged('inserted', first[:m[50]] + b'\x55' + first[m[50]:])

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_entropy.npz')
    np.savez_compressed(path, names=np.array(names), damaged=np.array(damaged), **out)
    print(f'{len(names)} valid and {len(damaged)} damaged cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
    main()
