#!/usr/bin/env python3
"""Generate tests/golden/zstd_wide_kat.npz: blosc2 chunks with blocks of 160, 192 and 256 KiB whose streams are frames the system
libzstd (ZSTD_compress) wrote, framed the way c-blosc2 frames a zstd chunk (make_zstd_golden.frame: codec format 4; one frame per
byte plane for clevel <= 5 with the shuffle, one frame per block otherwise).  Streams above 128 KiB are frames of more than one
zstd block.

The expected answer of every chunk is its input.  The inputs are not stored: they are rebuilt from cimg.synth by inputs() below
and checked against the sha256 digests in the file, so the file stays small and the GPU machines need no libzstd.

Run:  python tests/golden/make_zstd_wide_golden.py      (needs libzstd.so.1; output committed)
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "compressed-image_amd"))
from cimg import synth  # noqa: E402
import make_zstd_golden as G  # noqa: E402


def _make(kind, dtype, width, height, nbytes):
    """natural: a synth.natural_channel image; tiled: a 256 x 40 synth.tiled_channel tile repeated (matches up to ~100 KiB back)"""
    if kind == "natural":
        raw = np.ascontiguousarray(synth.natural_channel(dtype, width, height)).view(np.uint8).ravel()
    else:
        tile = np.ascontiguousarray(synth.tiled_channel(dtype, 256, 40)).view(np.uint8).ravel()
        raw = np.tile(tile, -(-nbytes // tile.size))
    return raw[:nbytes].copy()


# name -> (family, dtype, width, height, bytes kept, typesize, blocksize, clevel, filter)
CASES = {}
for _bs in (163840, 196608, 262144):
    for _dt, _ts in ((np.uint8, 1), (np.uint16, 2), (np.float32, 4)):
        for _cl in (3, 9):
            _n = _bs + _bs // 2 + 4 * _ts                       # a full block and a ragged second
            _h = -(-_n // (1024 * _ts))
            CASES[f"tiled_{np.dtype(_dt).name}_b{_bs}_c{_cl}"] = ("tiled", _dt, 1024, _h, _n, _ts, _bs, _cl, "shuffle")
for _bs in (163840, 262144):
    _n = _bs
    CASES[f"natural_float32_b{_bs}_c3"] = ("natural", np.float32, 512, -(-_n // 2048), _n, 4, _bs, 3, "shuffle")
    CASES[f"natural_uint16_b{_bs}_c9_none"] = ("natural", np.uint16, 512, -(-_n // 1024), _n, 2, _bs, 9, "none")
CASES["tiled_float16_b196608_c9_none"] = ("tiled", np.float16, 1024, 384, 3 * 196608, 2, 196608, 9, "none")
CASES["tiled_float32_b262144_c9_bitshuffle"] = ("tiled", np.float32, 1024, 192, 3 * 262144 - 4000, 4, 262144, 9, "bitshuffle")


def inputs():
    """name -> (uint8 input, typesize, blocksize, clevel, filter), rebuilt from cimg.synth"""
    out = {}
    for name, (kind, dt, w, h, n, ts, bs, cl, filt) in CASES.items():
        src = _make(kind, dt, w, h, n)
        assert src.size == n, name
        out[name] = (src, ts, bs, cl, filt)
    return out


def main():
    z = C.CDLL("libzstd.so.1")
    z.ZSTD_versionString.restype = C.c_char_p
    z.ZSTD_compressBound.restype = C.c_size_t
    z.ZSTD_compressBound.argtypes = [C.c_size_t]
    z.ZSTD_compress.restype = C.c_size_t
    z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    z.ZSTD_maxCLevel.restype = C.c_int
    store = {"zstd_version": np.array(z.ZSTD_versionString().decode())}
    names = []
    for name, (src, ts, bs, cl, filt) in inputs().items():
        chunk = G.frame(z, src, ts, bs, cl, filt)
        store["in_sha256|" + name] = np.array(hashlib.sha256(src.tobytes()).hexdigest())
        store["chunk|" + name] = np.frombuffer(chunk, np.uint8)
        names.append(name)
        print(name, src.size, "->", len(chunk))
    store["chunks"] = np.array(names)
    path = os.path.join(HERE, "zstd_wide_kat.npz")
    np.savez_compressed(path, **store)
    print(len(names), "chunks;", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
