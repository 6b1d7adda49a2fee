"""Wide blocks (csrc/wide_kernel.h) against today's 32 KiB path: for 128 MiB of float16 / float32 / uint8 (tiled and natural), in
4 MiB chunks, LZ4 at clevel 9, block sizes 32 KiB (the normal kernels), 128 KiB and 256 KiB (the wide ones): encode and decode
kernel time per 128 MiB (device-resident, HIP events), compression ratio, round trip checked.  A last section decodes oracle-written
float32 BloscLZ chunks with 256 KiB blocks on the GPU and with the 16-thread CPU port (oracle/bench_cpu.c) on the same chunks.

--codec blosclz: the write side of BloscLZ instead -- clevel 9 on the same six data sets at 32 KiB (cimg_encode_streams_blosclz), 128 KiB
and 256 KiB blocks (cimg_encode_wide_blosclz): encode kernel us (HIP events, median of ten calls after a warm-up), beside it the lz4
encoder on the same data and block size, and the oracle's BloscLZ compress over the same chunks on 16 host threads (best of three);
every GPU chunk is compared with the oracle's.  --mib N: N MiB a data set instead of 128.
usage: python tools/diag_wide_blocks.py [--codec lz4|blosclz] [--mib N]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from cimg import hip, synth  # noqa: E402
import _oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--codec", choices=("lz4", "blosclz"), default="lz4")
ap.add_argument("--mib", type=int, default=128)
args = ap.parse_args()
CHUNK, N = 4 << 20, args.mib << 20
eng = hip.Engine(0)
nch = N // CHUNK
raw_off = np.arange(nch, dtype=np.int64) * CHUNK
dest = CHUNK + 32
comp_off = np.arange(nch, dtype=np.int64) * dest
d_raw, d_comp, d_out = eng.alloc(N), eng.alloc(nch * dest), eng.alloc(N)


def kernel_us(ids, reps):
    return sum(eng.kernel_time(k)[0] for k in ids) / reps * 1e3


ENC_IDS = [hip.K_ENCODE, hip.K_ENCODE_WIDE, hip.K_ENCODE_WIDE_BLOSCLZ, hip.K_LAYOUT, hip.K_EMIT]


def encode_median_us(p, calls=10):
    """kernel us of one compress call over the data in d_raw: median of `calls` after a warm-up -> (us, cbytes of the last call)"""
    cb = eng.compress_device(p, d_raw.ptr, raw_off, [CHUNK] * nch, d_comp.ptr, comp_off, [dest] * nch)
    eng.enable_timing(1)
    us = []
    for _ in range(calls):
        eng.reset_timing()
        cb = eng.compress_device(p, d_raw.ptr, raw_off, [CHUNK] * nch, d_comp.ptr, comp_off, [dest] * nch)
        us.append(kernel_us(ENC_IDS, 1))
    eng.enable_timing(False)
    return float(np.median(us)), cb


def blosclz_write_side():
    L = O.lib()
    L.orc_bench_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_int]
    L.orc_bench_compress.restype = C.c_int64
    ref = np.zeros(nch * dest, np.uint8)
    ref_cb = np.zeros(nch, np.int32)
    for dt in ("float16", "float32", "uint8"):
        dtype = np.dtype(dt)
        for fam in ("tiled", "natural"):
            host = np.ascontiguousarray(getattr(synth, fam + "_channel")(dtype.type, 4096, N // (4096 * dtype.itemsize))).view(np.uint8).ravel()
            d_raw.upload(host)
            for blk in (32768, 131072, 262144):
                blz, cb = encode_median_us(hip.cparams(dtype.itemsize, clevel=9, blocksize=blk, compcode=hip.BLOSCLZ))
                comp = d_comp.download()
                lz4, cb4 = encode_median_us(hip.cparams(dtype.itemsize, clevel=9, blocksize=blk))
                op = O.cparams(dtype.itemsize, clevel=9, blocksize=blk, compcode=O.BLOSCLZ)
                best = 1e9
                for _ in range(3):
                    t = time.perf_counter()
                    tot = L.orc_bench_compress(C.byref(op), host.ctypes.data, nch, CHUNK, ref.ctypes.data, dest, dest, ref_cb.ctypes.data, 16, 1)
                    best = min(best, time.perf_counter() - t)
                same = tot > 0 and np.array_equal(ref_cb, cb) and all(
                    np.array_equal(comp[i * dest:i * dest + cb[i]], ref[i * dest:i * dest + cb[i]]) for i in range(nch))
                print("%-8s %-8s block %6d: blosclz encode %10.1f us, lz4 encode %9.1f us, oracle 16 threads %10.1f us per %d MiB, "
                      "GPU / CPU %.2f, ratio %.3f (lz4 %.3f), %s" % (dt, fam, blk, blz, lz4, best * 1e6, args.mib, blz / (best * 1e6),
                                                                    N / float(np.asarray(cb).sum()), N / float(np.asarray(cb4).sum()),
                                                                    "chunks = oracle's" if same else "CHUNKS DIFFER"), flush=True)


if args.codec == "blosclz":
    blosclz_write_side()
    for d in (d_raw, d_comp, d_out):
        d.free()
    eng.close()
    sys.exit(0)


for dt in ("float16", "float32", "uint8"):
    dtype = np.dtype(dt)
    for fam in ("tiled", "natural"):
        host = np.ascontiguousarray(getattr(synth, fam + "_channel")(dtype.type, 4096, N // (4096 * dtype.itemsize))).view(np.uint8).ravel()
        d_raw.upload(host)
        for blk in (32768, 131072, 262144):
            p = hip.cparams(dtype.itemsize, clevel=9, blocksize=blk)

            def step():
                cb = eng.compress_device(p, d_raw.ptr, raw_off, [CHUNK] * nch, d_comp.ptr, comp_off, [dest] * nch)
                eng.decompress_device(d_comp.ptr, comp_off, [CHUNK] * nch, [blk] * nch, d_out.ptr, raw_off, comp_size=cb)
                return cb
            cb = step()
            ok = np.array_equal(d_out.download(), host)
            eng.enable_timing(1)
            eng.reset_timing()
            reps = 3
            for _ in range(reps):
                step()
            enc = kernel_us([hip.K_ENCODE, hip.K_ENCODE_WIDE, hip.K_LAYOUT, hip.K_EMIT], reps)
            dec = kernel_us([hip.K_DECODE, hip.K_DECODE_WIDE], reps)
            eng.enable_timing(False)
            print("%-8s %-8s block %6d: encode %9.1f us, decode %8.1f us per 128 MiB, ratio %.3f, %s" % (
                dt, fam, blk, enc, dec, N / float(np.asarray(cb).sum()), "round trip exact" if ok else "DIFFER"), flush=True)

# float32, BloscLZ, 256 KiB blocks: chunks the oracle writes, decoded on the GPU and by the 16-thread CPU port
L = O.lib()
L.orc_bench_decompress.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int]
L.orc_bench_decompress.restype = C.c_int64
for fam in ("tiled", "natural"):
    arr = getattr(synth, fam + "_channel")(np.float32, 4096, N // (4096 * 4))
    host = np.ascontiguousarray(arr).view(np.uint8).ravel()
    comp = np.zeros(nch * dest, np.uint8)
    cb = np.zeros(nch, np.int32)
    for i in range(nch):
        r, c = O.compress(O.cparams(4, blocksize=262144, compcode=O.BLOSCLZ), host[i * CHUNK:(i + 1) * CHUNK], destsize=dest)
        assert r > 0
        comp[i * dest:i * dest + r] = np.frombuffer(c, np.uint8)
        cb[i] = r
    out = np.zeros(N, np.uint8)
    best = 1e9
    for _ in range(3):
        t = time.perf_counter()
        assert L.orc_bench_decompress(comp.ctypes.data, nch, dest, cb.ctypes.data, out.ctypes.data, CHUNK, 16, 1) == N
        best = min(best, time.perf_counter() - t)
    assert np.array_equal(out, host)
    d_comp.upload(comp)
    eng.decompress_device(d_comp.ptr, comp_off, [CHUNK] * nch, [262144] * nch, d_out.ptr, raw_off, comp_size=cb)
    ok = np.array_equal(d_out.download(), host)
    eng.enable_timing(1)
    eng.reset_timing()
    for _ in range(3):
        eng.decompress_device(d_comp.ptr, comp_off, [CHUNK] * nch, [262144] * nch, d_out.ptr, raw_off, comp_size=cb)
    dec = kernel_us([hip.K_DECODE, hip.K_DECODE_WIDE], 3)
    eng.enable_timing(False)
    print("float32  %-8s blosclz block 262144 (oracle-written): GPU decode %8.1f us, CPU 16 threads %9.1f us per 128 MiB, ratio %.3f, %s" % (
        fam, dec, best * 1e6, N / float(cb.sum()), "exact" if ok else "DIFFER"), flush=True)
for d in (d_raw, d_comp, d_out):
    d.free()
eng.close()
