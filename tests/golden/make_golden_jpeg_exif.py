"""Writes tests/golden/jpeg_exif.npz: JPEG files that carry an EXIF orientation, and Pillow's oriented decode of them.

Run in the build container only (``python tests/golden/make_golden_jpeg_exif.py``); the tests read the .npz and never
need Pillow.  ``names`` lists the cases; per case ``jpg_<name>`` holds the file's bytes and ``rgb_<name>`` the (H, W, 3)
RGB picture ``ImageOps.exif_transpose`` makes of libjpeg-turbo's decode (a grayscale plane three times).
``orientation`` (parallel to ``names``) is what the header parse must report: the tag's value for the well-formed files, 0
for the malformed ones.  ``plain`` (parallel too) names the case whose ``rgb_`` is the file's decode WITHOUT the
orientation -- the ``_o1`` file of the same picture, whose scan is the same bytes.

Well-formed files: every size of SIZES with orientations 1 to 8, the APP1 segment written by Pillow (``save(exif=)``,
little-endian).  The sizes are the smallest at which the pixel stage's tiles can go wrong: one pixel, one row, one
column, odd sizes in 4:2:0 (chroma edges), 4:2:2, a grayscale file, 70 x 130 (more than one 32 x 32 tile in both
directions, ragged on both edges) and 5 x 300 (wider than the plain pixel kernel's 256-pixel tile).

Hand-made APP1 segments, all on the 13 x 29 picture:
  ``mm_o6``        big-endian TIFF header ("MM"), orientation 6: well-formed
  ``second_o8``    two Exif APP1 segments, 8 then 3: the first decides (Pillow reads the first TIFF header too)
  ``badifd``       the header puts IFD0 at offset 4096, far outside the segment: orientation 0
  ``o9``           the value 9: orientation 0
  ``long``         the tag typed LONG (value 1, so that Pillow's reading of it -- it accepts LONG -- is the identity as
                   well, and the expected pixels do not depend on which reader is asked): orientation 0
The script asserts that Pillow leaves the three malformed pictures as they are.
"""
import io
import os
import struct

import numpy as np
from PIL import Image, ImageOps, features

SIZES = [(1, 1, '444'), (1, 17, '444'), (17, 1, '444'), (13, 29, '420'), (48, 64, '422'), (9, 20, 'gray'),
         (70, 130, '444'), (5, 300, '420')]      # (h, w, sampling)
SAMPLINGS = {'444': 0, '422': 1, '420': 2}


def picture(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 255 * (xx + 2 * yy) / max(2 * h + w - 3, 1)], -1)
    return np.clip(grad + (rng.integers(0, 256, (h, w, 3)) - 128) * 0.2, 0, 255).astype(np.uint8)


def encode(rgb, sampling, exif=None):
    buf = io.BytesIO()
    kw = {} if exif is None else dict(exif=exif)
    if sampling == 'gray':
        Image.fromarray(rgb).convert('L').save(buf, 'JPEG', quality=90, **kw)
    else:
        Image.fromarray(rgb).save(buf, 'JPEG', quality=90, subsampling=SAMPLINGS[sampling], **kw)
    return buf.getvalue()


def transposed(data):
    im = ImageOps.exif_transpose(Image.open(io.BytesIO(data)))
    a = np.asarray(im)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else a)


def tiff(order, entries, ifd=8):
    """A TIFF header and IFD0 of ``entries`` ((tag, type, count, 4 value bytes)); ``ifd``: where the header says IFD0 is."""
    e = '<' if order == 'II' else '>'
    body = struct.pack(e + 'H', len(entries))
    for tag, typ, n, value in entries:
        body += struct.pack(e + 'HHI', tag, typ, n) + value
    return order.encode() + struct.pack(e + 'HI', 42, ifd) + body + struct.pack(e + 'I', 0)


def with_app1(data, *payloads):
    """``data`` (a file without EXIF) with Exif APP1 segments after its APP0."""
    assert data[:4] == b'\xff\xd8\xff\xe0'
    cut = 4 + struct.unpack('>H', data[4:6])[0]
    segs = b''.join(b'\xff\xe1' + struct.pack('>H', len(p) + 8) + b'Exif\0\0' + p for p in payloads)
    return data[:cut] + segs + data[cut:]


def short(order, v):
    return struct.pack(('<' if order == 'II' else '>') + 'HH', v, 0)


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures must come from libjpeg-turbo'
    out, names, orient, plain = {}, [], [], []

    def add(name, data, o, base):
        names.append(name)
        orient.append(o)
        plain.append(base)
        out['jpg_' + name] = np.frombuffer(data, np.uint8)
        out['rgb_' + name] = transposed(data)

    for i, (h, w, samp) in enumerate(SIZES):
        rgb = picture(h, w, 100 + i)
        for o in range(1, 9):
            exif = Image.Exif()
            exif[0x0112] = o
            add(f'{h}x{w}_{samp}_o{o}', encode(rgb, samp, exif.tobytes()), o, f'{h}x{w}_{samp}_o1')
    bare = encode(picture(13, 29, 103), '420')
    base = '13x29_420_o1'
    add('13x29_420_mm_o6', with_app1(bare, tiff('MM', [(0x0112, 3, 1, short('MM', 6))])), 6, base)
    add('13x29_420_second_o8', with_app1(bare, tiff('II', [(0x0112, 3, 1, short('II', 8))]),
                                         tiff('II', [(0x0112, 3, 1, short('II', 3))])), 8, base)
    add('13x29_420_badifd', with_app1(bare, tiff('II', [(0x0112, 3, 1, short('II', 6))], ifd=4096)), 0, base)
    add('13x29_420_o9', with_app1(bare, tiff('II', [(0x0112, 3, 1, short('II', 9))])), 0, base)
    add('13x29_420_long', with_app1(bare, tiff('II', [(0x0112, 4, 1, struct.pack('<I', 1))])), 0, base)
    for n, o, b in zip(names, orient, plain):
        if o in (0, 1):
            assert np.array_equal(out['rgb_' + n], out['rgb_' + b]), f'Pillow changed {n}'
    out['names'] = np.array(names)
    out['orientation'] = np.array(orient, np.int32)
    out['plain'] = np.array(plain)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_exif.npz')
    np.savez_compressed(path, **out)
    print(f'{len(names)} files -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
