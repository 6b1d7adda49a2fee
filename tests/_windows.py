"""Helpers of the window tests (test_emu_windows.py, test_gpu_windows.py): the cimg_window struct, chunk sets, and the expected
output of a window call -- a canary-filled buffer with each window's rows cut out of the decoded plane (numpy slices)."""
import ctypes as C

import numpy as np

import _oracle as O

CANARY = 0xA5
ERR_READ_BUFFER, ERR_WRITE_BUFFER, ERR_INVALID_PARAM, ERR_NULL_POINTER = -5, -6, -12, -23


class Window(C.Structure):
    _fields_ = [("chunk_first", C.c_int32), ("chunk_count", C.c_int32), ("origin", C.c_int64), ("row_pitch", C.c_int64),
                ("width", C.c_int32), ("height", C.c_int32), ("out_off", C.c_int64), ("out_pitch", C.c_int64)]


def windows(specs):
    """specs: dicts with chunk_first, chunk_count, origin, row_pitch, width, height, out_off, out_pitch -> ctypes array"""
    arr = (Window * max(len(specs), 1))()
    for i, s in enumerate(specs):
        for k, v in s.items():
            setattr(arr[i], k, int(v))
    return arr


def pack(specs, ts, gap=7):
    """Give each window an out_off / out_pitch with `gap` canary bytes after every row; returns (specs, output size)."""
    at = 0
    out = []
    for s in specs:
        s = dict(s)
        s.setdefault("out_pitch", s["width"] * ts + gap)
        s["out_off"] = at + 3
        at += 3 + s["out_pitch"] * max(s["height"], 1) + 16
        out.append(s)
    return out, at + 64


def expected(planes, specs, ts, size):
    """planes[k]: the decoded bytes of window k's plane (uint8)."""
    out = np.full(size, CANARY, np.uint8)
    for plane, s in zip(planes, specs):
        rp = s["row_pitch"] if s["height"] > 1 else 0
        for r in range(s["height"]):
            a = (s["origin"] + r * rp) * ts
            o = s["out_off"] + r * s["out_pitch"]
            out[o:o + s["width"] * ts] = plane[a:a + s["width"] * ts]
    return out


def oracle_chunks(p, raw, chunk_bytes):
    """raw (uint8) cut into chunks of chunk_bytes, each compressed by the oracle -> list of bytes"""
    out = []
    for o in range(0, raw.size, chunk_bytes):
        piece = raw[o:o + chunk_bytes]
        r, c = O.compress(p, piece, destsize=piece.size + 64)
        assert r > 0, r
        out.append(c)
    return out


def sizes(chunks):
    hdr = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8)) for c in chunks]
    return np.array([h[0] for h in hdr], np.int32), np.array([h[2] for h in hdr], np.int32)


def concat(chunks, align=64):
    offs, at = [], 0
    for c in chunks:
        offs.append(at)
        at += (len(c) + align - 1) // align * align
    buf = np.zeros(at + 64, np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = np.frombuffer(c, np.uint8)
    return buf, np.array(offs, np.int64), np.array([len(c) for c in chunks], np.int32)


def plane_of(chunks):
    return np.concatenate([O.decompress(c)[1] for c in chunks])


def standard_windows(elems, W, chunk_elems, nchunks):
    """The window shapes every matrix case runs, over a plane of `elems` elements seen as rows of W."""
    H = elems // W
    mid = chunk_elems // W                     # the row in which chunk 1 starts
    s = [
        dict(origin=elems // 2 + 5, row_pitch=1, width=1, height=1),                 # one element
        dict(origin=3 * W, row_pitch=W, width=W, height=1),                          # one full row
        dict(origin=0, row_pitch=elems, width=elems, height=1),                      # the whole plane
        dict(origin=max(mid - 2, 0) * W + W - 37, row_pitch=W, width=53, height=5),  # straddles blocks and the chunk boundary
        dict(origin=11, row_pitch=W + 3, width=29, height=min(H - 1, (elems - 40) // (W + 3))),   # row_pitch > width, every chunk
    ]
    for d in s:
        d["chunk_first"], d["chunk_count"] = 0, nchunks
    return s
