"""zstd at wide blocks against the 32 KiB path: for 128 MiB of float16 / float32 / uint8 (tiled and natural), in 4 MiB chunks,
zstd at clevel 9, block sizes 32 KiB (the normal kernels), 128 KiB (wide encoder, normal read path) and 256 KiB (wide encoder,
cimg_decode_wide + cimg_zstd_walk + cimg_zstd_replay_wide): encode and decode kernel time per 128 MiB (device-resident, HIP
events), compression ratio, round trip checked.  Where the oracle's CPU port can read zstd (it needs libzstd), the same chunks are
also decoded by it with 16 threads.
usage: python tools/diag_wide_zstd.py"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from cimg import hip, synth  # noqa: E402
import _oracle as O  # noqa: E402

CHUNK, N = 4 << 20, 128 << 20
eng = hip.Engine(0)
nch = N // CHUNK
raw_off = np.arange(nch, dtype=np.int64) * CHUNK
dest = CHUNK + 32
comp_off = np.arange(nch, dtype=np.int64) * dest
d_raw, d_comp, d_out = eng.alloc(N), eng.alloc(nch * dest), eng.alloc(N)
L = O.lib()
L.orc_bench_decompress.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int]
L.orc_bench_decompress.restype = C.c_int64


def kernel_us(ids, reps):
    return sum(eng.kernel_time(k)[0] for k in ids) / reps * 1e3


def cpu_us(cb, host):
    comp = d_comp.download(nch * dest)
    out = np.zeros(N, np.uint8)
    best = None
    for _ in range(3):
        t = time.perf_counter()
        if L.orc_bench_decompress(comp.ctypes.data, nch, dest, np.asarray(cb, np.int32).ctypes.data, out.ctypes.data, CHUNK, 16, 1) != N:
            return None
        best = min(best or 1e9, time.perf_counter() - t)
    return best * 1e6 if np.array_equal(out, host) else None


for dt in ("float16", "float32", "uint8"):
    dtype = np.dtype(dt)
    for fam in ("tiled", "natural"):
        host = np.ascontiguousarray(getattr(synth, fam + "_channel")(dtype.type, 4096, N // (4096 * dtype.itemsize))).view(np.uint8).ravel()
        d_raw.upload(host)
        for blk in (32768, 131072, 262144):
            p = hip.cparams(dtype.itemsize, clevel=9, blocksize=blk, compcode=hip.ZSTD)

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
            enc = kernel_us([hip.K_ENCODE_ZSTD, hip.K_ENCODE_WIDE_ZSTD, hip.K_LAYOUT, hip.K_EMIT], reps)
            # (K_DECODE_ZSTD is a batch's zstd read path as a whole, the normal one or the wide one behind cimg_decode_wide)
            dec = kernel_us([hip.K_DECODE, hip.K_DECODE_WIDE, hip.K_DECODE_ZSTD], reps)
            eng.enable_timing(False)
            cpu = cpu_us(cb, host)
            print("%-8s %-8s block %6d: encode %9.1f us, decode %8.1f us per 128 MiB, ratio %.3f, %s; CPU port decode (16 threads) %s" % (
                dt, fam, blk, enc, dec, N / float(np.asarray(cb).sum()), "round trip exact" if ok else "DIFFER",
                "%.1f us" % cpu if cpu else "n/a"), flush=True)
for d in (d_raw, d_comp, d_out):
    d.free()
eng.close()
