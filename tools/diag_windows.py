"""Windows (csrc/window_kernel.h) against whole decodes, the two measurements of DESIGN.md section 9:
  (1) a device-resident 1 GiB float32 plane (16384^2, tiled family, lz4 level 9, 4 MiB chunks of 32 KiB blocks): the full-plane
      decode (cimg_decompress_batch_device_sized) against one 1024^2 window (cimg_decompress_windows_device) -- kernel time from HIP
      events (K_DECODE + K_DECODE_ZSTD / K_DECODE_WINDOW) and wall time of the call, medians of REPS;
  (2) the Python module: Channel.get_region(1024, 1024, 512, 512) on a 4096^2 float16 channel (4 MiB chunks) against
      get_decompressed()[1024:1536, 1024:1536], wall time, medians of REPS.
Prints one JSON line.  usage: python tools/diag_windows.py [--out file]"""
import importlib.util
import json
import os
import sys
import sysconfig
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from cimg import hip, synth  # noqa: E402

REPS = 10
res = {}
eng = hip.Engine(0)
n, chunk = 16384, 4 << 20
img = synth.tiled_channel(np.float32, n, n)
raw = np.ascontiguousarray(img).view(np.uint8).ravel()
nch = raw.size // chunk
dest = chunk + 64
raw_off = np.arange(nch, dtype=np.int64) * chunk
comp_off = np.arange(nch, dtype=np.int64) * dest
d_raw, d_comp = eng.alloc(raw.size), eng.alloc(nch * dest)
d_raw.upload(raw)
cb = eng.compress_device(hip.cparams(4), d_raw.ptr, raw_off, [chunk] * nch, d_comp.ptr, comp_off, [dest] * nch)
res["plane_ratio"] = round(raw.size / float(cb.sum()), 3)
w = 1024
x0, y0 = 5000, 7000
d_win = eng.alloc(w * w * 4)
spec = dict(chunk_first=0, chunk_count=nch, origin=y0 * n + x0, row_pitch=n, width=w, height=w, out_off=0, out_pitch=w * 4)


def timed(fn, kernels):
    fn()                                                   # warm-up (allocations, LDS attributes)
    eng.enable_timing(1)
    eng.reset_timing()
    walls, kus = [], []
    for _ in range(REPS):
        eng.reset_timing()
        t = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t) * 1e6)
        kus.append(sum(eng.kernel_time(k)[0] for k in kernels) * 1e3)
    eng.enable_timing(0)
    return float(np.median(kus)), float(np.median(walls))


full_k, full_w = timed(lambda: eng.decompress_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, d_raw.ptr, raw_off, comp_size=cb),
                       (hip.K_DECODE, hip.K_DECODE_ZSTD))
win_k, win_w = timed(lambda: eng.decompress_windows_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, 4, [spec], d_win.ptr, comp_size=cb),
                     (hip.K_DECODE_WINDOW,))
got = d_win.download().view(np.float32).reshape(w, w)
assert np.array_equal(got, img[y0:y0 + w, x0:x0 + w])
res.update(full_decode_kernel_us=round(full_k, 1), full_decode_wall_us=round(full_w, 1), window_kernel_us=round(win_k, 1),
           window_wall_us=round(win_w, 1), window_blocks=eng.window_stats()["blocks_decoded"], plane_blocks=nch * (chunk // 32768),
           kernel_ratio=round(full_k / win_k, 2), wall_ratio=round(full_w / win_w, 2))
d_raw.free(); d_comp.free(); d_win.free()
eng.close()

path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
spec_m = importlib.util.spec_from_file_location("compressed_image", path)
ci = importlib.util.module_from_spec(spec_m)
spec_m.loader.exec_module(ci)
arr = synth.tiled_channel(np.float16, 4096, 4096)
ch = ci.Channel(arr, 4096, 4096)


def wall(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t) * 1e6)
    return float(np.median(ts)), r


reg_us, a = wall(lambda: ch.get_region(1024, 1024, 512, 512))
dec_us, b = wall(lambda: ch.get_decompressed()[1024:1536, 1024:1536].copy())
assert np.array_equal(a, b) and np.array_equal(a, arr[1024:1536, 1024:1536])
res.update(region_wall_us=round(reg_us, 1), decompressed_slice_wall_us=round(dec_us, 1), region_speedup=round(dec_us / reg_us, 2))
line = json.dumps(res)
print(line)
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    open(sys.argv[2], "w").write(line + "\n")
