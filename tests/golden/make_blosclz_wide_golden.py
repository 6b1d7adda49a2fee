#!/usr/bin/env python3
"""Generate tests/golden/blosclz_wide_kat.npz from the SYSTEM c-blosc 1.21 (BloscLZ 2.3.0, the pin of oracle/blosclz.c): BloscLZ
payloads of streams of 65 535 bytes and more, i.e. around and beyond the uint16 position table of the normal-path encoder.

Streams this long are what c-blosc2 hands to BloscLZ for blocks above 64 KiB (128 / 256 KiB blocks of 1- and 2-byte types, the
65 536-byte planes of float32 with 256 KiB blocks, unsplit leftover blocks).  The vectors pin the wide-block encoder
(compressed-image_amd/csrc/wide_kernel.h: blosclz_wide_encode) byte for byte.  A payload is obtained as make_blosclz_golden.py
obtains it: blosc_compress_ctx(clevel, no shuffle, typesize 1, n, ..., "blosclz", blocksize = n) makes one block with one stream
and calls blosclz_compress(clevel, src, n, dest, maxout = n); csize == n means the codec gave up and the stream was stored raw
(recorded as length 0).

The inputs are not stored: the tests rebuild them with stream_inputs() below and check them against the sha256 the file holds.
The payloads are stored as sha256 + length.  The generator refuses to write unless oracle/blosclz.c's orc_blosclz_compress gives
the same bytes for every vector: nobody had compared the two above 65 535 bytes before this file.

The far-limit streams ("far|n|d"): n zero bytes, the same 200 nonzero bytes at [100, 300) and at [100 + d, 300 + d), noise in the
last 5000 bytes.  The zero run is one match of tens of kilobytes that enters next to nothing into the table, so the first copy's
slots survive until the second copy is probed: the second copy is coded as a match while d stays below MAX_FARDISTANCE
(65 535 + 8191 - 1 = 73 725) and as literals from there on, and the offset changes from the two-byte to the four-byte form
between d = 8191 and 8192.

Run:  python tests/golden/make_blosclz_wide_golden.py      (needs /opt/conda/lib/libblosc.so.1; the output is committed)
"""
import ctypes as C
import hashlib
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "compressed-image_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cimg import synth  # noqa: E402

CLEVELS = (1, 5, 9)
BOUNDARY = (65535, 65536, 65537)
SIZES = (98304, 131072, 200001, 262144)
FAR_D = (8190, 8191, 8192, 8193, 65535, 65536, 73722, 73723, 73724, 73725, 73726, 73727, 73728, 90000)
FAR_D_LONG = (65536, 73724, 73725, 90000)          # the same with n = 262 144


def prng(seed, n):
    """n pseudo-random uint64 values: splitmix64 of a counter, in plain numpy integer arithmetic (no library RNG stream to
    change under the vectors)."""
    x = np.arange(n, dtype=np.uint64) + np.full(n, seed, np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def prng_bytes(seed, n, mod=256):
    return ((prng(seed, n) >> np.uint64(32)) % np.uint64(mod)).astype(np.uint8)


def _plane(dtype, plane, natural, n):
    fn = synth.natural_channel if natural else synth.tiled_channel
    a = fn(dtype, 4096, max(1, -(-n // 4096) + 1)).view(np.uint8).reshape(-1, np.dtype(dtype).itemsize)
    return np.ascontiguousarray(a[:n, plane])


def _period(seed, n):
    p = 1 + int(prng(seed, 1)[0] % np.uint64(299))
    return np.tile(prng_bytes(seed + 1, p), n // p + 1)[:n].copy()


def _steps(seed, n):
    rep = 1 + int(prng(seed, 1)[0] % np.uint64(32))
    return np.resize(np.repeat(prng_bytes(seed + 1, n // 8 + 1), rep), n).astype(np.uint8)


def _walk(seed, n):
    return (np.cumsum(prng_bytes(seed, n, 5).astype(np.int64) - 2) & 0xFF).astype(np.uint8)


def far_stream(n, d):
    a = np.zeros(n, np.uint8)
    pat = prng_bytes(700, 200, 255) + np.uint8(1)       # nonzero
    a[100:300] = pat
    a[100 + d:300 + d] = pat
    a[n - 5000:] = prng_bytes(701, 5000)
    return a


def stream_inputs():
    """The stream vectors, (name, uint8 array).  Rebuilt by the tests from this function (the file holds their digests, not the
    bytes): counter-hash noise (prng) and the project's seeded synth channels."""
    out = []
    for n in BOUNDARY:                                   # (a) the lengths around the uint16 table's limit, a coded family
        out.append((f"steps|{n}", _steps(800 + n, n)))
    for k, n in enumerate(SIZES):                        # (b) what byte planes of images look like
        out.append((f"tiled_u16_hi|{n}", _plane(np.uint16, 1, False, n)))
        out.append((f"tiled_u16_lo|{n}", _plane(np.uint16, 0, False, n)))
        out.append((f"natural_u16_hi|{n}", _plane(np.uint16, 1, True, n)))
        out.append((f"natural_u16_lo|{n}", _plane(np.uint16, 0, True, n)))
        out.append((f"period|{n}", _period(900 + 10 * k, n)))
        out.append((f"steps|{n}", _steps(1000 + 10 * k, n)))
        out.append((f"walk|{n}", _walk(1100 + k, n)))
    out.append(("random|131072", prng_bytes(1200, 131072)))          # (c) the probe gives up; one match from end to end
    out.append(("constant|131072", np.full(131072, 7, np.uint8)))
    for d in FAR_D:                                      # (d) the far-distance limits
        out.append((f"far|100000|{d}", far_stream(100000, d)))
    for d in FAR_D_LONG:
        out.append((f"far|262144|{d}", far_stream(262144, d)))
    return out


def main():
    import _oracle as O
    b = C.CDLL("/opt/conda/lib/libblosc.so.1")
    b.blosc_get_version_string.restype = C.c_char_p
    ver = b.blosc_get_version_string().decode()
    lz_name, lz_ver = C.c_char_p(), C.c_char_p()
    b.blosc_get_complib_info(b"blosclz", C.byref(lz_name), C.byref(lz_ver))
    b.blosc_compress_ctx.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    b.blosc_compress_ctx.restype = C.c_int
    store = {"blosc_version": np.array(ver), "blosclz_version": np.array(lz_ver.value.decode())}
    names, coded, raw = [], 0, 0
    for name, src in stream_inputs():
        src = np.ascontiguousarray(src, dtype=np.uint8)
        n = src.size
        assert n == int(name.split("|")[1]), name
        store["in_sha256|" + name] = np.array(hashlib.sha256(src.tobytes()).hexdigest())
        for clevel in CLEVELS:
            dst = np.zeros(n + 4096, np.uint8)
            r = b.blosc_compress_ctx(clevel, 0, 1, n, src.ctypes.data, dst.ctypes.data, dst.size, b"blosclz", n, 1)
            assert r > 0
            head = dst[:32].tobytes()
            nbytes, blocksize, cbytes = struct.unpack_from("<iii", head, 4)
            assert nbytes == n and blocksize == n and cbytes == r and not int(dst[2]) & 0x2, (name, clevel)
            (bstart,) = struct.unpack_from("<i", head, 16)
            (csize,) = struct.unpack_from("<i", dst[bstart:bstart + 4].tobytes(), 0)
            assert bstart + 4 + csize == r
            payload = b"" if csize == n else dst[bstart + 4:bstart + 4 + csize].tobytes()
            ro, oracle, need = O.blosclz_compress(src, clevel=clevel, want_need=True)
            if oracle != payload or ro != len(payload):
                raise SystemExit(f"oracle/blosclz.c differs from BloscLZ {lz_ver.value.decode()} on {name} clevel {clevel}: "
                                 f"{ro} vs {len(payload)} bytes -- nothing written")
            key = f"{name}|{clevel}"
            names.append(key)
            store["len|" + key] = np.int32(len(payload))
            store["sha256|" + key] = np.array(hashlib.sha256(payload).hexdigest())
            coded += bool(payload)
            raw += not payload
    store["cases"] = np.array(names)
    path = os.path.join(HERE, "blosclz_wide_kat.npz")
    np.savez_compressed(path, **store)
    print(f"c-blosc {ver} / BloscLZ {lz_ver.value.decode()}: {len(names)} vectors ({coded} coded, {raw} raw), all equal to the oracle's "
          f"-> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
