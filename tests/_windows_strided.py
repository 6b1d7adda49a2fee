"""Helpers of the strided window tests (test_emu_windows_strided.py, test_gpu_windows_strided.py): the cimg_window_strided struct,
the window shapes every matrix case runs, the expected output of a strided call -- numpy indexing into the decoded plane -- and
the brute-force count of the blocks that hold a byte of a sampled element."""
import ctypes as C

import numpy as np

from _windows import CANARY


class StridedWindow(C.Structure):
    _fields_ = [("chunk_first", C.c_int32), ("chunk_count", C.c_int32), ("origin", C.c_int64), ("row_pitch", C.c_int64),
                ("col_pitch", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("out_off", C.c_int64), ("out_pitch", C.c_int64)]


def swindows(specs):
    arr = (StridedWindow * max(len(specs), 1))()
    for i, s in enumerate(specs):
        for k, v in s.items():
            setattr(arr[i], k, int(v))
    return arr


def element_index(s):
    """plane element index of every sampled element of window s: (height, width) int64"""
    rp = s["row_pitch"] if s["height"] > 1 else 0
    cp = s["col_pitch"] if s["width"] > 1 else 0
    return s["origin"] + np.arange(s["height"], dtype=np.int64)[:, None] * rp + np.arange(s["width"], dtype=np.int64)[None, :] * cp


def expected(planes, specs, ts, size):
    """planes[k]: the decoded bytes of window k's plane (uint8); every byte outside the sampled elements keeps the canary"""
    out = np.full(size, CANARY, np.uint8)
    for plane, s in zip(planes, specs):
        if s["width"] == 0 or s["height"] == 0:
            continue
        e = element_index(s)
        px = plane[:plane.size // ts * ts].reshape(-1, ts)[e]                      # (height, width, ts)
        for r in range(s["height"]):
            o = s["out_off"] + r * s["out_pitch"]
            out[o:o + s["width"] * ts] = px[r].ravel()
    return out


def sampled_blocks(specs, nbytes, blocksize, ts):
    """Brute force, byte by byte: (the number of (window, chunk, block) triples such that the block holds at least one byte of a
    sampled element of the window, the set of chunks that hold such a block)."""
    count, chunks = 0, set()
    for s in specs:
        if s["width"] == 0 or s["height"] == 0:
            continue
        cf, cn = s["chunk_first"], s["chunk_count"]
        start = np.concatenate([[0], np.cumsum(np.asarray(nbytes[cf:cf + cn], np.int64))])
        pos = (element_index(s).ravel()[:, None] * ts + np.arange(ts, dtype=np.int64)[None, :]).ravel()
        c = np.searchsorted(start, pos, side="right") - 1
        b = (pos - start[c]) // np.asarray(blocksize[cf:cf + cn], np.int64)[c]
        pairs = np.unique(np.stack([c, b]), axis=1)
        count += pairs.shape[1]
        chunks |= {cf + int(x) for x in pairs[0]}
    return count, chunks


def strided_windows(elems, chunk_elems, nchunks, epb):
    """The strided shapes every matrix case runs in ONE call (steps 1 and > 1 mixed), over a plane of `elems` elements in chunks of
    chunk_elems with epb elements per block: col_pitch 1, 2, 3, 7, epb - 1, epb, 3 * epb and more than a chunk; single rows and
    several rows over every chunk, row_pitch > span."""
    s = []
    for cp in (1, 2, 3, 7):
        s.append(dict(origin=5, row_pitch=1, col_pitch=cp, width=min(211, (elems - 6) // cp + 1), height=1))
        span = 28 * cp + 1
        rp = max(span + 13, 700)
        s.append(dict(origin=chunk_elems - 2 * rp - 17, row_pitch=rp, col_pitch=cp, width=29, height=6))      # over the chunk boundary
        s.append(dict(origin=11, row_pitch=rp, col_pitch=cp, width=29, height=(elems - 11 - span) // rp + 1))  # every chunk
    for cp in (epb - 1, epb, 3 * epb):
        s.append(dict(origin=7, row_pitch=1, col_pitch=cp, width=(elems - 8) // cp + 1, height=1))             # a row over the plane
        span = 2 * cp + 1
        if epb - 2 + span <= elems:                                                                             # (where three samples fit)
            s.append(dict(origin=epb - 2, row_pitch=span + 5, col_pitch=cp, width=3, height=min(4, (elems - epb - span) // (span + 5) + 1)))
    far = chunk_elems + 77
    s.append(dict(origin=3, row_pitch=far + 1, col_pitch=far, width=2, height=2))
    s.append(dict(origin=elems - 1, row_pitch=1, col_pitch=9, width=1, height=1))                               # the last element
    s.append(dict(origin=elems - 1 - 4 * 7, row_pitch=1, col_pitch=7, width=5, height=1))                       # ... as a last sample
    for d in s:
        d["chunk_first"], d["chunk_count"] = 0, nchunks
        assert d["width"] > 0 and d["height"] > 0, d
    return s
