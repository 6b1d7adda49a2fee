"""Device-resident objects (compressed/device_channel.h, device_image.h) on one MI355X.  Medians of REPS calls
after warm-up; kernel times from the engine's HIP-event slots; everything in ONE process, torch imported first:
  (1) DeviceImage(...) + get_decompressed(out=) for 4 x 4096^2 float16 (lz4 + shuffle, defaults) in GB/s of pixels, against
      Image(...) + get_decompressed() of the host classes on the same pixels, and against the raw device-resident round trip
      (cimg_compress_batch_device + cimg_decompress_batch_device_sized) of the same geometry; where the difference goes: the pack
      launch, the store's allocation, the rest;
  (2) cimg_pack_chunks (K_PACK) and cimg_interleave (K_INTERLEAVE) in us and GB/s (read + written) against a torch device-to-device
      copy of the same byte count;
  (3) device memory held: device_bytes() against uncompressed_size() and against the unpacked cimg_compress_batch_device layout,
      for the headline image and the "natural" family;
  (4) set_region of a 1024^2 window into a 1 GiB float32 plane: total time, the update's and the repack's kernel time.
Prints one JSON line.  usage: python tools/diag_device_resident.py [--out file]"""
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
from cimg import hip, synth  # noqa: E402

spec = importlib.util.spec_from_file_location("compressed_image", os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX")))
ci = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ci)

REPS = 10
res = {}
L = hip.load()
L.cimg_shared_engine.restype = hip.C.c_void_p
shared = hip.Engine.__new__(hip.Engine)                      # the engine the module's objects run on (never closed from here)
shared.handle, shared._buffers = hip.C.c_void_p(L.cimg_shared_engine()), set()


def med(fn, reps=REPS, warm=2):
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


def kernel_us(fn, kernels):
    """median over REPS calls of the summed event time of `kernels` on the shared engine"""
    fn()
    shared.enable_timing(1)
    out = []
    for _ in range(REPS):
        shared.reset_timing()
        fn()
        out.append([shared.kernel_time(k)[0] * 1e3 for k in kernels])
    shared.enable_timing(0)
    return [float(x) for x in np.median(np.array(out), axis=0)]


def torch_copy_us(nbytes):
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(7)
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a)
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


# ---- (1) the object layer against the host classes and the raw calls ---------------------------------------------------------
n = 4096
planes = np.stack([synth.tiled_channel(np.float16, n, n) for _ in range(4)])
t = torch.from_numpy(planes.view(np.int16)).cuda().view(torch.float16)
out = torch.empty_like(t)
pix = planes.nbytes
holder = {}


def dev_make():
    holder["img"] = ci.DeviceImage(np.float16, t, n, n)


def dev_read():
    holder["img"].get_decompressed(out=out)


t_make, t_read = med(dev_make), med(dev_read)
assert torch.equal(out.view(torch.int16), t.view(torch.int16))
res["device_image"] = {"construct_ms": round(t_make * 1e3, 3), "decompress_ms": round(t_read * 1e3, 3),
                       "round_trip_gbps": round(2 * pix / (t_make + t_read) / 1e9, 1)}
enc_us, pack_us = kernel_us(dev_make, [hip.K_ENCODE, hip.K_PACK])
res["device_image"].update(encode_kernel_us=round(enc_us, 1), pack_kernel_us=round(pack_us, 1))
alloc_t = med(lambda: torch.cuda.synchronize() or shared.alloc(holder["img"].device_bytes()).free())
res["device_image"]["store_alloc_free_us"] = round(alloc_t * 1e6, 1)
hostp = [planes[c] for c in range(4)]


def host_make():
    holder["himg"] = ci.Image(np.float16, hostp, n, n)


t_hmake, t_hread = med(host_make, reps=5, warm=1), med(lambda: holder["himg"].get_decompressed(), reps=5, warm=1)
res["host_image"] = {"construct_ms": round(t_hmake * 1e3, 2), "decompress_ms": round(t_hread * 1e3, 2),
                     "round_trip_gbps": round(2 * pix / (t_hmake + t_hread) / 1e9, 1)}
chunk = 4 << 20
nch = pix // chunk
roff = np.arange(nch, dtype=np.int64) * chunk
coff = np.arange(nch, dtype=np.int64) * (chunk + 64)
d_comp = torch.empty(nch * (chunk + 64), dtype=torch.uint8, device="cuda")
p = hip.cparams(2)
nb, ds, bs = [chunk] * nch, [chunk + 32] * nch, [32768] * nch
raw = {}


def raw_rt():
    raw["cb"] = shared.compress_device(p, t.data_ptr(), roff, nb, d_comp.data_ptr(), coff, ds)
    shared.decompress_device(d_comp.data_ptr(), coff, nb, bs, out.data_ptr(), roff, comp_size=raw["cb"])


t_raw = med(raw_rt)
res["raw_calls"] = {"round_trip_ms": round(t_raw * 1e3, 3), "round_trip_gbps": round(2 * pix / t_raw / 1e9, 1)}
img = holder["img"]
res["hbm_held"] = {"headline": {"pixels": pix, "device_bytes": img.device_bytes(), "unpacked_layout": int(nch * (chunk + 32))}}

# ---- (2) the two copy kernels against a plain copy ------------------------------------------------------------------------------
packed = img.device_bytes()
us_pack = kernel_us(dev_make, [hip.K_PACK])[0]
us_copy = torch_copy_us(packed)
res["pack_kernel"] = {"bytes": packed, "us": round(us_pack, 1), "gbps": round(2 * packed / us_pack / 1e3, 1), "torch_copy_us": round(us_copy, 1),
                      "fraction_of_copy": round(us_copy / us_pack, 3)}
crop = torch.empty((2048, 2048, 4), dtype=torch.float16, device="cuda")
us_il = kernel_us(lambda: img.get_region(1024, 1024, 2048, 2048, out=crop, interleaved=True), [hip.K_INTERLEAVE])[0]
us_copy = torch_copy_us(crop.numel() * 2)
res["interleave_kernel"] = {"bytes": crop.numel() * 2, "us": round(us_il, 1), "gbps": round(2 * crop.numel() * 2 / us_il / 1e3, 1),
                            "torch_copy_us": round(us_copy, 1), "fraction_of_copy": round(us_copy / us_il, 3)}
big = torch.empty((4, n, n), dtype=torch.float16, device="cuda")
bigil = torch.empty((n, n, 4), dtype=torch.float16, device="cuda")
shared.enable_timing(1)
samples = []
for _ in range(REPS + 1):
    shared.reset_timing()
    shared.interleave_device(t.data_ptr(), n * n * 2, 4, 2, n * n, bigil.data_ptr())
    samples.append(shared.kernel_time(hip.K_INTERLEAVE)[0] * 1e3)
shared.enable_timing(0)
us_il = float(np.median(samples[1:]))
us_copy = torch_copy_us(pix)
assert torch.equal(bigil.view(torch.int16), t.view(torch.int16).permute(1, 2, 0).contiguous())
res["interleave_kernel_128MiB"] = {"bytes": pix, "us": round(us_il, 1), "gbps": round(2 * pix / us_il / 1e3, 1), "torch_copy_us": round(us_copy, 1),
                                   "fraction_of_copy": round(us_copy / us_il, 3)}
del big, bigil, crop

# ---- (3) the natural family ------------------------------------------------------------------------------------------------------
nat = np.stack([synth.natural_channel(np.float16, n, n, seed=c) for c in range(4)]) if hasattr(synth, "natural_channel") else None
if nat is not None:
    tn = torch.from_numpy(nat.view(np.int16)).cuda().view(torch.float16)
    ni = ci.DeviceImage(np.float16, tn, n, n)
    res["hbm_held"]["natural"] = {"pixels": nat.nbytes, "device_bytes": ni.device_bytes(), "unpacked_layout": int(nch * (chunk + 32))}
    del ni, tn
del holder["img"], img, holder["himg"]

# ---- (4) a window write into a 1 GiB plane ------------------------------------------------------------------------------------------
N = 16384
plane = torch.from_numpy(synth.tiled_channel(np.float32, N, N).view(np.int32)).cuda().view(torch.float32)
ch = ci.DeviceChannel(plane, N, N)
patch = torch.rand((1024, 1024), dtype=torch.float32, device="cuda")
t_set = med(lambda: ch.set_region(5000, 7000, patch), reps=REPS, warm=1)
ks = kernel_us(lambda: ch.set_region(5000, 7000, patch), [hip.K_UPDATE_PATCH, hip.K_UPDATE_LAYOUT, hip.K_UPDATE_EMIT, hip.K_ENCODE, hip.K_PACK])
res["set_region_1GiB"] = {"total_ms": round(t_set * 1e3, 3), "update_kernels_us": round(sum(ks[:4]), 1), "repack_kernel_us": round(ks[4], 1),
                          "store_bytes": ch.device_bytes(), "repack_share_of_total": round(ks[4] / (t_set * 1e6), 3)}
got = torch.as_tensor(ch.get_region(5000, 7000, 1024, 1024), device="cuda")
assert torch.equal(got, patch)

line = json.dumps(res)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
