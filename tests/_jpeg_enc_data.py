"""What the JPEG encoder's host and GPU tests share: the cases of tests/golden/jpeg_encode.npz and a table whose regions
lie apart, behind guard bytes."""
import numpy as np

GUARD_BYTE = 0x5A
GAP = 192            # bytes between two regions (a multiple of 64: coefficient offsets stay on a block, work offsets aligned)
PAD_COLS = 5         # guard columns behind every row of the input


def case_of(name):
    """``'37x53_420_grad_q90'`` -> ``(quality, subsampling)``."""
    parts = name.split('_')
    return int(parts[-1][1:]), parts[1]


def load_cases(golden):
    g = golden('jpeg_encode')
    names = [str(n) for n in g['names']]
    return names, [g['src_' + n] for n in names], [g['jpg_' + n].tobytes() for n in names], \
        [case_of(n)[0] for n in names], [case_of(n)[1] for n in names]


def spread(et):
    """Moves every region of ``et``'s table apart (``GAP`` guard bytes in front of and behind each; the rows of the input
    at a wider pitch) -> ``(pixel bytes, coefficient elements, work bytes, output bytes)`` of the buffers to make."""
    pix = coef = work = out = GAP
    for n, t in enumerate(et.table):
        t.src_pitch = t.channels * t.width + PAD_COLS
        t.src_off = pix
        pix += t.src_pitch * t.height + GAP
        t.coef_off = coef // 2 // 64 * 64 + 64
        coef = 2 * (t.coef_off + t.nblocks * 64) + GAP
        t.work_off = (work + 7) // 8 * 8
        work = t.work_off + et.work_region_bytes(n) + GAP
        t.out_off = out
        out += t.out_cap + GAP
    return pix, coef // 2 + 64, work, out


def place_pixels(et, srcs, pixel_bytes):
    """The flat input: every image at its offset and pitch, guard bytes everywhere else."""
    pix = np.full(pixel_bytes, GUARD_BYTE, np.uint8)
    for t, a in zip(et.table, srcs):
        row = t.channels * t.width
        for y in range(t.height):
            o = t.src_off + y * t.src_pitch
            pix[o:o + row] = a[y].reshape(-1)
    return pix


def assert_guards(buf, regions, what):
    """Every byte of the uint8 array ``buf`` outside ``regions`` (``(offset, length)`` in bytes) still holds the guard."""
    mask = np.ones(buf.size, bool)
    for off, length in regions:
        mask[off:off + length] = False
    bad = np.flatnonzero(mask & (buf != GUARD_BYTE))
    assert bad.size == 0, f'{what}: {bad.size} guard bytes overwritten, the first at {int(bad[0])}'
