"""Blank device-resident channels (compressed/device_channel.h: full; csrc/special_plan.h) on one MI355X.
Medians of REPS calls after warm-up, everything in ONE process, torch imported first:
  (1) get_decompressed(out=) of a DeviceChannel.full of 4096^2 float32 -- the pattern fill of cimg_decode_blocks, 64 MiB written --
      against a torch device-to-device copy of the same bytes (the yardstick of sections 9e / 9f) and against the same call on a
      DeviceChannel.zeros (special-zero chunks, wave_fill_global);
  (2) the time to make the channel: DeviceChannel.full against DeviceChannel(...) over constant pixels in device memory;
  (3) device memory held by each.
Prints one JSON line.  usage: python tools/diag_special.py [--out file]"""
import importlib.util
import json
import os
import sys
import sysconfig
import time

import torch  # (first: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

spec = importlib.util.spec_from_file_location("compressed_image", os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX")))
ci = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ci)

REPS = 10
N = 4096
VALUE = -2.75


def med(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    res = {"pixels_bytes": N * N * 4, "reps": REPS}
    out = torch.empty((N, N), dtype=torch.float32, device="cuda")
    src = torch.full((N, N), VALUE, dtype=torch.float32, device="cuda")
    full = ci.DeviceChannel.full(np.float32, VALUE, N, N)
    zeros = ci.DeviceChannel.zeros(np.float32, N, N)
    packed = ci.DeviceChannel(src, N, N)
    full.get_decompressed(out=out)
    assert bool((out == VALUE).all())
    t_copy = med(lambda: out.copy_(src))
    t_full = med(lambda: full.get_decompressed(out=out))
    t_zero = med(lambda: zeros.get_decompressed(out=out))
    t_packed = med(lambda: packed.get_decompressed(out=out))
    gb = res["pixels_bytes"] / 1e9
    res["copy_us"], res["copy_GBps_written"] = t_copy * 1e6, gb / t_copy
    res["full_decode_us"], res["full_decode_GBps"] = t_full * 1e6, gb / t_full
    res["zeros_decode_us"], res["zeros_decode_GBps"] = t_zero * 1e6, gb / t_zero
    res["constant_pixels_decode_us"] = t_packed * 1e6
    res["full_over_copy"] = t_full / t_copy
    res["make_full_us"] = med(lambda: ci.DeviceChannel.full(np.float32, VALUE, N, N)) * 1e6
    res["make_from_constant_pixels_us"] = med(lambda: ci.DeviceChannel(src, N, N)) * 1e6
    res["device_bytes"] = {"full": full.device_bytes(), "zeros": zeros.device_bytes(), "constant_pixels": packed.device_bytes(), "chunks": full.num_chunks()}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
