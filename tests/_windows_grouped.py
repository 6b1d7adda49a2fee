"""Helpers of the grouped window tests (test_emu_windows_grouped.py, test_gpu_windows_grouped.py): the build of
tests/emu/window_grouped_emu.cpp, the small planes every case runs on, rectangles as cimg_window_strided specs, and the brute-force
count of the distinct blocks a set of windows meets.

Expectations never come from the code under test: pixels are numpy indexing into the oracle's decode (_windows_strided.expected),
block counts are counted byte by byte from the geometry."""
import ctypes as C
import os
import subprocess

import numpy as np

from cimg import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
FLAGS = ["-std=c++17", "-fPIC", "-Wall", "-Wextra", "-fno-strict-aliasing", "-I", CSRC]
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_grouped_emu.cpp")]

BLOSCLZ, LZ4, ZSTD = 0, 1, 5
W, H = 512, 130                                   # the plane of every case: 66 560 elements
# typesize -> (chunk bytes, block bytes): >= 3 chunks and >= 9 blocks a plane, a short last chunk; for typesizes 2 and 4 every
# chunk ends in a leftover block (7.5 blocks a chunk), for typesize 3 elements straddle blocks (8192 % 3 != 0)
GEOMETRY = {1: (16384, 4096), 2: (30720, 4096), 3: (49152, 8192), 4: (61440, 8192), 8: (65536, 32768)}


class EmuCParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32), ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


def build_emu(out_dir, sanitize=False):
    """tests/emu/window_grouped_emu.cpp with emu.cpp and wide_emu.cpp as a library (or, sanitize: with window_grouped_asan_main.cpp
    as a stand-alone program under ASan / UBSan, LDS modelled with zero slack)"""
    if sanitize:
        out = os.path.join(str(out_dir), "window_grouped_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                               os.path.join(EMU, "window_grouped_asan_main.cpp"), *SOURCES, "-o", out])
        return out
    out = os.path.join(str(out_dir), "libwindow_grouped_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    dev = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    host = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.wnemu_windows_strided_device.argtypes = L.wnemu_windows_grouped_device.argtypes = dev
    L.wnemu_windows_strided_host.argtypes = L.wnemu_windows_grouped_host.argtypes = host
    L.wnemu_window_stats.argtypes = [vp]
    L.wnemu_group_items.argtypes = [C.c_int, vp, vp, vp, vp]
    L.wemu_compress_batch.argtypes = [C.POINTER(EmuCParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.emu_set_write_order.argtypes = [C.c_int]
    return L


_planes = {}


def plane(ts, seed=0):
    """the W x H plane of typesize ts: tiled pixels with some entropy, still compressible (read-only, shared)"""
    key = (ts, seed)
    if key not in _planes:
        rng = np.random.default_rng(100 + seed)
        base = synth.tiled_channel(np.float16, 64, W * H * ts // 128 + 1).view(np.uint8).ravel()
        raw = base[:W * H * ts].copy()
        raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)
        raw.setflags(write=False)
        _planes[key] = raw
    return _planes[key]


def rect(x, y, w, h, sx=1, sy=1, nchunks=0, chunk_first=0, row_len=W, base=0):
    """the rectangle (x, y, w, h) of a row_len-wide plane, every sy-th row and sx-th element, as a cimg_window_strided spec
    (base: the plane's element offset of row 0, for a plane that starts inside its first chunk)"""
    return dict(chunk_first=chunk_first, chunk_count=nchunks, origin=base + y * row_len + x, row_pitch=sy * row_len, col_pitch=sx,
                width=(w + sx - 1) // sx if w else 0, height=(h + sy - 1) // sy if h else 0)


def matrix_windows(nchunks):
    """The windows every matrix case runs in ONE call: a row of tiles (shared rows, disjoint columns), overlapping windows, col_pitch
    1 and > 1 mixed, the whole plane, the last row and the last element, 1 x 1 windows, and windows of width or height 0."""
    r = [rect(128 * k, 10, 128, 40) for k in range(4)]
    r += [rect(100, 20, 200, 30), rect(150, 25, 200, 30), rect(150, 25, 200, 30)]              # overlapping; one twice
    r += [rect(3, 1, 500, 128, 7, 5), rect(5, 60, 300, 50, 3, 1), rect(0, 0, W, H, 1, 9), rect(0, 0, W, H)]
    r += [rect(0, H - 1, W, 1), rect(W - 1, H - 1, 1, 1), rect(0, 0, 1, 1)]
    r += [rect(17 * k % W, 13 * k % H, 1, 1) for k in range(9)]
    r += [rect(40, 40, 0, 5), rect(40, 40, 5, 0), rect(40, 40, 0, 0, 3, 2)]
    for d in r:
        d["chunk_count"] = nchunks
    return r


def touched_blocks(specs, nbytes, blocksize, ts):
    """Brute force, byte by byte: the set of (batch chunk, block) that hold a byte of a sampled element of some window"""
    from _windows_strided import element_index
    out = set()
    for s in specs:
        if s["width"] == 0 or s["height"] == 0:
            continue
        cf, cn = s["chunk_first"], s["chunk_count"]
        start = np.concatenate([[0], np.cumsum(np.asarray(nbytes[cf:cf + cn], np.int64))])
        pos = (element_index(s).ravel()[:, None] * ts + np.arange(ts, dtype=np.int64)[None, :]).ravel()
        c = np.searchsorted(start, pos, side="right") - 1
        b = (pos - start[c]) // np.asarray(blocksize[cf:cf + cn], np.int64)[c]
        out |= {(cf + int(x), int(y)) for x, y in np.unique(np.stack([c, b]), axis=1).T}
    return out
