#!/usr/bin/env python3
"""Generate tests/golden/lz4_u32_kat.npz from the SYSTEM liblz4 (1.9.3): LZ4_compress_fast on streams of 65 546 bytes and
more, i.e. around and beyond liblz4's byU16 / byU32 switch (LZ4_64Klimit = 65 547).

Streams this long are what c-blosc2 hands to LZ4 for blocks above 64 KiB (128 / 256 KiB blocks of 1- and 2-byte types, and
unsplit leftover blocks).  The vectors pin the wide-block encoder (compressed-image_amd/csrc/wide_kernel.h) byte for byte,
together with liblz4's return value under tight capacities and the smallest capacity that still succeeds (`need`).
The inputs are not stored: the tests rebuild them with stream_inputs() below and check them against the sha256 the file holds.
The compressed streams are stored as sha256 + length too (most are nearly all literals, i.e. as large as their input).

Besides the stream vectors the file holds chunk digests: seeded synth channels compressed into blosc2 chunks with 128 and
256 KiB blocks.  The chunk layer is the oracle's (oracle/chunk.c: geometry, shuffle, stream rules, running destsize), built
here with its LZ4 stream layer replaced by calls into liblz4 -- so every stream's bytes, byU32 ones included, are liblz4's.
The generator checks itself first: on inputs whose streams all stay in the byU16 regime its chunks must equal
orc_blosc2_compress byte for byte.

Run:  python tests/golden/make_lz4_u32_golden.py      (needs liblz4.so.1 and a C compiler; the output is committed)
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
sys.path.insert(0, os.path.join(ROOT, "compressed-image_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cimg import synth  # noqa: E402

SIZES = [65546, 65547, 65548, 98304, 131072, 262144]

# the LZ4 stream layer of the oracle, answered by liblz4 (need: the smallest capacity liblz4 still succeeds with)
_LZ4_SHIM = r"""
#include <stdint.h>
int LZ4_compress_fast(const char*, char*, int, int, int);
int LZ4_decompress_safe(const char*, char*, int, int);
static int bound(int n) { return n + n / 255 + 16; }
int orc_lz4_compress_fast(const uint8_t* src, int n, uint8_t* dst, int cap, int accel, int* need)
{
    int r = LZ4_compress_fast((const char*)src, (char*)dst, n, cap, accel);
    if (need && r > 0) {
        static char tmp[1 << 20];
        int lo = 1, hi = cap < bound(n) ? cap : bound(n);
        while (lo < hi) { int mid = (lo + hi) / 2; if (LZ4_compress_fast((const char*)src, tmp, n, mid, accel) > 0) hi = mid; else lo = mid + 1; }
        *need = lo;
    }
    return r;
}
int orc_lz4_decompress_safe(const uint8_t* src, int csize, uint8_t* dst, int cap)
{
    int r = LZ4_decompress_safe((const char*)src, (char*)dst, csize, cap);
    return r < 0 ? -1 : r;
}
"""


def build_liblz4_chunk_layer(tmp):
    shim = os.path.join(tmp, "lz4_shim.c")
    with open(shim, "w") as f:
        f.write(_LZ4_SHIM)
    out = os.path.join(tmp, "liborc_liblz4.so")
    srcs = [os.path.join(ORACLE, s) for s in ("blosclz.c", "filters.c", "chunk.c", "zstd_dl.c")]
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-fopenmp", "-I", ORACLE, shim] + srcs
                          + ["-o", out, "-l:liblz4.so.1", "-ldl"])
    return out


def prng(seed, n):
    """n pseudo-random uint64 values: splitmix64 of a counter, in plain numpy integer arithmetic (no library RNG stream to
    change under the vectors)."""
    x = np.arange(n, dtype=np.uint64) + np.full(n, seed, np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def prng_bytes(seed, n, mod=256):
    return ((prng(seed, n) >> np.uint64(32)) % np.uint64(mod)).astype(np.uint8)


def stream_inputs():
    """The stream vectors, (name, uint8 array).  Rebuilt by the tests from this function (the file holds their digests, not the
    bytes): counter-hash noise (prng) and the project's seeded synth channels."""
    out = []
    words = [b"lorem ", b"ipsum ", b"dolor ", b"sit ", b"amet, ", b"consectetur ", b"chunk ", b"image "]
    for k, n in enumerate(SIZES):
        out.append((f"zeros{n}", np.zeros(n, np.uint8)))
        out.append((f"ramp{n}", (np.arange(n) & 255).astype(np.uint8)))
        if n in (65547, 131072, 262144):
            out.append((f"rand{n}", prng_bytes(100 + k, n)))
        out.append((f"low{n}", prng_bytes(200 + k, n, 4)))
        txt = b"".join(words[i] for i in prng_bytes(300 + k, n // 3, len(words)))[:n]
        out.append((f"text{n}", np.frombuffer(txt.ljust(n, b"."), np.uint8).copy()))
        vals, lens = prng_bytes(400 + k, n // 40 + 1), prng_bytes(500 + k, n // 40 + 1, 79).astype(np.int64) + 1
        out.append((f"runs{n}", np.resize(np.repeat(vals, lens)[:n], n)))
    # synth planes: byte planes of 128 / 256 KiB blocks (2-byte types give 64 / 128 KiB planes, 1-byte types the whole block)
    for dt, ts, blk in [(np.float16, 2, 262144), (np.uint8, 1, 131072), (np.uint8, 1, 262144)]:
        for kind, fn in (("tiled", synth.tiled_channel), ("natural", synth.natural_channel)):
            raw = fn(dt, 1024, 1024).view(np.uint8).ravel()[:blk]
            for j, s in enumerate(raw.reshape(-1, ts).T):
                out.append((f"{kind}_{np.dtype(dt).name}_b{blk}_s{j}", np.ascontiguousarray(s)))
    # repeats just inside and just outside the 65 535-byte window of the byU32 regime
    for d in (65533, 65535, 65536, 65540):
        head = prng_bytes(600 + d, d)
        out.append((f"repeat_d{d}", np.concatenate([head, head[:98304 - d]])))
    return out


def chunk_inputs():
    cases = []
    for dt in (np.float16, np.uint8, np.float32):
        for kind, fn in (("tiled", synth.tiled_channel), ("natural", synth.natural_channel)):
            for blk in (131072, 262144):
                cases.append((f"{kind}_{np.dtype(dt).name}_b{blk}", fn(dt, 1024, 1024), blk))
    # a ragged last chunk: 2 MiB + 40 000 bytes of float16, 256 KiB blocks (a short, unsplit last block)
    ragged = synth.natural_channel(np.float16, 1024, 1044).view(np.uint8).ravel()[:2 * 1048576 + 40000].view(np.float16)
    cases.append(("ragged_float16_b262144", ragged, 262144))
    return cases


def main():
    lz4 = C.CDLL("liblz4.so.1")
    lz4.LZ4_versionString.restype = C.c_char_p
    ver = lz4.LZ4_versionString().decode()
    lz4.LZ4_compress_fast.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lz4.LZ4_compress_fast.restype = C.c_int
    store = {"lz4_version": np.array(ver)}
    names = []
    for name, src in stream_inputs():
        src = np.ascontiguousarray(src, dtype=np.uint8)
        n = src.size
        bound = n + n // 255 + 16
        for accel in (1, 5):
            dst = np.zeros(bound + 64, np.uint8)
            r = lz4.LZ4_compress_fast(src.ctypes.data, dst.ctypes.data, n, bound, accel)
            lo, hi = 1, bound                                   # smallest capacity that succeeds (success is monotone in cap)
            while lo < hi:
                mid = (lo + hi) // 2
                if lz4.LZ4_compress_fast(src.ctypes.data, dst.ctypes.data, n, mid, accel) > 0:
                    hi = mid
                else:
                    lo = mid + 1
            store[f"need|{name}|a{accel}"] = np.int32(lo)
            caps = sorted({bound, n, lo, lo - 1})               # generous, the stream size, and the edge on both sides
            for cap in caps:
                if cap < 1:
                    continue
                d2 = np.zeros(bound + 64, np.uint8)
                r = lz4.LZ4_compress_fast(src.ctypes.data, d2.ctypes.data, n, cap, accel)
                key = f"{name}|a{accel}|c{cap}"
                names.append(key)
                store[f"ret|{key}"] = np.int32(r)
                if cap == bound:                                # the bytes once per (input, accel): a success is the same at any cap
                    out = d2[:max(r, 0)].tobytes()            # (as a digest: most of these streams are literals, i.e. their input)
                    store[f"sha256|{name}|a{accel}"] = np.array(hashlib.sha256(out).hexdigest())
                    store[f"len|{name}|a{accel}"] = np.int32(len(out))
        store[f"in_sha256|{name}"] = np.array(hashlib.sha256(src.tobytes()).hexdigest())
    store["cases"] = np.array(names)

    # ---- chunk digests ----
    import _oracle as O
    with tempfile.TemporaryDirectory() as tmp:
        L = C.CDLL(build_liblz4_chunk_layer(tmp))
        L.orc_blosc2_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.orc_blosc2_compress.restype = C.c_int

        def chunk_with(lib, arr, blk, compcode):
            a = np.ascontiguousarray(arr)
            raw = a.view(np.uint8).ravel()
            p = O.cparams(a.dtype.itemsize, blocksize=blk, compcode=compcode)
            dst = np.zeros(raw.size + 64 + 32, np.uint8)
            r = lib.orc_blosc2_compress(C.byref(p), raw.ctypes.data, raw.size, dst.ctypes.data, dst.size)
            assert r > 0, (r, a.dtype, blk, compcode)
            return dst[:r].tobytes()

        # self-check: where every stream stays byU16 the liblz4-backed chunk layer equals the oracle's chunks
        # (lz4hc blocks are never split: their stream is the whole block)
        for dt, blk, cc in ((np.float32, 262144, O.LZ4), (np.float16, 131072, O.LZ4), (np.uint8, 65536, O.LZ4), (np.float32, 32768, O.LZ4),
                            (np.float32, 65536, O.LZ4HC), (np.uint8, 65536, O.LZ4HC), (np.float16, 32768, O.LZ4HC)):
            for fn in (synth.tiled_channel, synth.natural_channel):
                arr = fn(dt, 1024, 512)
                assert chunk_with(L, arr, blk, cc) == chunk_with(O.lib(), arr, blk, cc), (dt, blk, cc)
        chunk_names = []
        for name, arr, blk in chunk_inputs():
            for cc, ccn in ((O.LZ4, "lz4"), (O.LZ4HC, "lz4hc")):
                key = f"{name}|{ccn}"
                c = chunk_with(L, arr, blk, cc)
                chunk_names.append(key)
                store[f"chunk_sha256|{key}"] = np.array(hashlib.sha256(c).hexdigest())
                store[f"chunk_size|{key}"] = np.int64(len(c))
        store["chunk_cases"] = np.array(chunk_names)
    path = os.path.join(HERE, "lz4_u32_kat.npz")
    np.savez_compressed(path, **store)
    print(f"liblz4 {ver}: {len(names)} stream cases, {len(chunk_names)} chunk digests -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
