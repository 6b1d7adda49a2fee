"""Shared by the pack / interleave tests (emulator and GPU): the case grids and the canary-checked layout of a pack call."""
import numpy as np

CANARY = 0xA7
SMALL = (0, 1, 15, 16, 17, 31, 32, 33, 4095)             # every pair of source / destination misalignment 0..15
LARGE = (65536, 65537, (4 << 20) + 32)                    # four pairs
FEW_PAIRS = ((0, 0), (0, 7), (9, 0), (5, 11))
ERR_INVALID_PARAM = -12

# the grid of tests/test_deinterleave.py
INTERLEAVE_CASES = [(nch, ts, npix) for nch in (1, 2, 3, 4, 5, 9) for ts in (1, 2, 4, 8)
                    for npix in (0, 1, 7, 15, 16, 17, 255, 1000, 4096, 4099)]


def grid():
    """(size, source misalignment, destination misalignment) of every case of the grid"""
    for n in SMALL:
        for sm in range(16):
            for dm in range(16):
                yield n, sm, dm
    for n in LARGE:
        for sm, dm in FEW_PAIRS:
            yield n, sm, dm


def layout(cases, gap=48):
    """One call for a list of (size, src misalignment, dst misalignment): offsets into a source and a destination buffer whose base
    is 16-byte aligned, every piece at its misalignment with at least `gap` canary bytes in front of it and behind the last.
    Returns (src_off, dst_off, bytes, src_size, dst_size)."""
    so, do, nb = [], [], []
    s = d = gap
    for n, sm, dm in cases:
        s = ((s + 15) & ~15) + sm
        d = ((d + 15) & ~15) + dm
        so.append(s); do.append(d); nb.append(n)
        s += n + gap
        d += n + gap
    return np.array(so, np.int64), np.array(do, np.int64), np.array(nb, np.int32), s + 16, d + 16


def expected(src, src_off, dst_off, nbytes, dst_size):
    want = np.full(dst_size, CANARY, np.uint8)
    for s, d, n in zip(src_off, dst_off, nbytes):
        want[d:d + n] = src[s:s + n]
    return want


def interleaved(planes, nch, ts):
    """planes: (nch, npix * ts) uint8 -> the interleaved bytes"""
    npix = planes.shape[1] // ts
    return planes.reshape(nch, npix, ts).transpose(1, 0, 2).reshape(-1)
