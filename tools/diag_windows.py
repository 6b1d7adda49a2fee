"""Windows (csrc/window_kernel.h) against whole decodes, the two measurements of DESIGN.md section 9:
  (1) a device-resident 1 GiB float32 plane (16384^2, tiled family, lz4 level 9, 4 MiB chunks of 32 KiB blocks): the full-plane
      decode (cimg_decompress_batch_device_sized) against one 1024^2 window (cimg_decompress_windows_device) -- kernel time from HIP
      events (K_DECODE + K_DECODE_ZSTD / K_DECODE_WINDOW) and wall time of the call, medians of REPS;
  (2) the Python module: Channel.get_region(1024, 1024, 512, 512) on a 4096^2 float16 channel (4 MiB chunks) against
      get_decompressed()[1024:1536, 1024:1536], wall time, medians of REPS.
Write legs, each against what it replaces, the chunk round trip on the same chunks:
  (3) one 1024^2 window written into the device-resident plane of (1) (cimg_update_windows_device, 17 chunks touched) against a
      decode of those 17 chunks plus their compress (cimg_decompress_batch_device_sized + cimg_compress_batch_device) -- kernel and
      wall time; the stats of the update (blocks staged / re-encoded);
  (4) the Python module: Channel.set_region of a 64^2 and a 512^2 window at (1024, 1024) into a 4096^2 float16 channel against
      get_chunk(2) + numpy edit + set_chunk(2), wall time; and the bytes the host call uploads (cimg_update_windows_host).
Strided leg (second table), against the route it replaces:
  (5) the 16 x 16 subsample of the device-resident plane of (1) (cimg_decompress_windows_strided_device: 1024 rows of 1024 elements,
      2048 blocks) against cimg_decompress_batch_device_sized of the whole plane plus a device strided copy of the same subsample
      (torch: full[::16, ::16].contiguous()) -- kernel time (HIP events of the engine, torch events for the copy) and wall time.
      It runs in a child process (`--strided-leg`) that imports torch first, so that torch and the engine share one HIP runtime;
      and the Python module: Channel.get_region(0, 0, 4096, 4096, step_x=8, step_y=8) on the 4096^2 float16 channel of (2) against
      get_decompressed()[::8, ::8], wall time.
Grouped leg (third table): many regions a call on the plane of (1), in a child process (`--grouped-leg`, torch
first) that can also be run on its own -- `python tools/diag_windows.py --grouped-leg` writes profiles/grouped/diag_windows_grouped.json:
  (6) sixteen 1024^2 tiles in a row, 64 seeded random 256^2 crops, 4096 seeded random pixels and 64 disjoint windows that share no
      block, each through cimg_decompress_windows_grouped_device against the strided multi-window call over the same windows
      (kernel time, wall time with its spread over the REPS runs, both block counts), against the whole decode followed by torch
      indexing (its kernel time: K_DECODE plus torch's indexing between two events), and against N single get_region calls through DeviceChannel (and DeviceChannel.get_regions / get_pixels itself).
Strided write leg, in a child process (`--write-strided-leg`, torch first) that can also be run on its own:
  (7) the 1024^2 window of (3) through cimg_update_windows_strided_device with col_pitch 1 against cimg_update_windows_device,
      alternating (wall medians, the plain call's max - min, each patch kernel's time); 4096 distinct seeded random pixels written
      into a device-resident 4096^2 float16 plane (lz4 + shuffle, 32 KiB blocks) through the strided call against the same 4096
      1 x 1 windows through the plain call; every 4th pixel in x and y of a 2048^2 region of that plane through
      DeviceChannel.set_region(..., step_x=4, step_y=4) against get_region of the rectangle + a torch scatter + set_region.
Typed leg, a process of its own (`python tools/diag_windows.py --typed-leg [--out file]`, torch first; it does
not build the plane of (1)) that writes profiles/typed/diag_windows_typed.json:
  (8) 256 seeded random 224^2 crops of a 3 x 4096^2 uint8 DeviceImage (lz4 + shuffle) as float32 with per-channel scale / offset,
      planar and pixel-major, through get_regions(dtype=, scale=, offset=[, interleaved=True]) against get_regions followed by
      torch's .float().mul_().add_() (and .permute().contiguous()); one 2048^2 crop of a 4 x 4096^2 float16 DeviceImage pixel-major
      in its own type through get_region(dtype=float16, interleaved=True) against get_region(interleaved=True).  The two routes
      alternate; kernel time (the shared engine's HIP events plus torch events around torch's part) and wall time, medians of REPS.
Typed write leg, a process of its own (`python tools/diag_windows.py --typed-write-leg [--out file]`, torch
first) that writes profiles/typed/diag_windows_typed_write.json:
  (9) 256 seeded random 224^2 crops written into a 3 x 4096^2 uint8 DeviceImage (lz4 + shuffle) from float32 tensors with per-channel
      scale / offset, planar and pixel-major, through set_regions(dtype=float32, scale=, offset=[, interleaved=True]) against the
      route without it: torch's sub / div / round / clamp / to(uint8) (after .permute().contiguous() for pixel-major) followed by
      set_regions.  The two routes alternate in one process; kernel time (every launch of the shared engine, HIP events, plus torch
      events around torch's part) and wall time, medians of REPS after a warm-up.  Then the patch launch alone on an all-identity
      call: set_regions(dtype=uint8) (cimg_update_patch_typed) against set_regions (cimg_update_patch_strided), same windows.
Masked leg, a process of its own (`python tools/diag_windows.py --masked-leg [--out file]`, torch first) that
writes profiles/masked/diag_windows_masked.json:
  (10) DeviceChannel.fill_region against set_region with a materialised constant tensor, and set_region(mask=) under a 50 % mask
      against get_region + torch.where + set_region; the same on Channel with numpy arrays (np.full, np.where): a 1024^2 region of a 16384^2 float32 lz4 plane, and the whole of a 4096^2 uint8
      plane.  The routes alternate in one process; wall time and kernel time (every launch of the shared engine, HIP events, plus
      torch events around torch's part), medians of REPS after a warm-up, with min and max.
Prints one JSON line.  usage: python tools/diag_windows.py [--out file]"""
import importlib.util
import json
import os
import subprocess
import sys
import sysconfig
import time

STRIDED_LEG = "--strided-leg" in sys.argv
GROUPED_LEG = "--grouped-leg" in sys.argv
WRITE_STRIDED_LEG = "--write-strided-leg" in sys.argv
TYPED_LEG = "--typed-leg" in sys.argv
TYPED_WRITE_LEG = "--typed-write-leg" in sys.argv
MASKED_LEG = "--masked-leg" in sys.argv
if STRIDED_LEG or GROUPED_LEG or WRITE_STRIDED_LEG or TYPED_LEG or TYPED_WRITE_LEG or MASKED_LEG:
    import torch  # noqa: F401  (first: one HIP runtime in the process, torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from cimg import hip, synth  # noqa: E402

REPS = 10


def typed_leg():
    """(8): typed reads of the device classes against the routes they replace"""
    import ctypes as C
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec_m = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec_m)
    spec_m.loader.exec_module(ci)
    m = 4096
    planes8 = np.stack([synth.tiled_channel(np.uint8, m, m, c=k) for k in range(3)])
    img8 = ci.DeviceImage(np.uint8, torch.from_numpy(planes8).cuda(), m, m)
    planes16 = np.stack([synth.tiled_channel(np.float16, m, m, c=k) for k in range(4)])
    img16 = ci.DeviceImage(np.float16, torch.from_numpy(planes16).cuda(), m, m)
    L = hip.load()
    L.cimg_shared_engine.restype = C.c_void_p
    se = hip.Engine.__new__(hip.Engine)                    # the module's engine, for its kernel times
    se.handle = C.c_void_p(L.cimg_shared_engine())
    windows = (hip.K_DECODE_WINDOW, hip.K_DECODE_WINDOW_STRIDED, hip.K_DECODE_WINDOW_GROUPED, hip.K_DECODE_WINDOW_TYPED, hip.K_INTERLEAVE)
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def alternating(old, new, old_has_torch):
        old(); new()
        torch.cuda.synchronize()
        se.enable_timing(1)
        rows = {"old": ([], []), "typed": ([], [])}
        for _ in range(REPS):
            for name, f in (("old", old), ("typed", new)):
                se.reset_timing()
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                rows[name][0].append((time.perf_counter() - t) * 1e6)
                k = sum(se.kernel_time(kid)[0] for kid in windows) * 1e3
                rows[name][1].append(k + (ev_a.elapsed_time(ev_b) * 1e3 if name == "old" and old_has_torch else 0.0))
        se.enable_timing(0)
        return {name: dict(wall_us=round(float(np.median(wl)), 1), wall_min_us=round(float(np.min(wl)), 1), wall_max_us=round(float(np.max(wl)), 1),
                           kernel_us=round(float(np.median(kl)), 1)) for name, (wl, kl) in rows.items()}

    out = {}
    rng = np.random.default_rng(8)
    N, c = 256, 224
    xs, ys = rng.integers(0, m - c, N), rng.integers(0, m - c, N)
    scale, offset = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]
    sc_t = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    of_t = torch.tensor(offset, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    u8 = torch.empty((N, 3, c, c), dtype=torch.uint8, device="cuda")
    for il in (False, True):
        res_new = torch.empty((N, c, c, 3) if il else (N, 3, c, c), dtype=torch.float32, device="cuda")
        kept = []

        def old():
            img8.get_regions(xs, ys, c, c, out=u8)
            ev_a.record()
            f = u8.float().mul_(sc_t).add_(of_t)
            kept[:] = [f.permute(0, 2, 3, 1).contiguous() if il else f]
            ev_b.record()

        def new():
            img8.get_regions(xs, ys, c, c, out=res_new, dtype=np.float32, scale=scale, offset=offset, interleaved=il)

        r = alternating(old, new, True)
        r["bit_equal"] = bool(torch.equal(kept[0].view(torch.int32), res_new.view(torch.int32)))
        r["result_bytes"] = res_new.numel() * 4
        r["old_temporary_bytes"] = u8.numel() + (res_new.numel() * 4 if il else 0)       # the uint8 crops; and the planar floats under permute
        out["crops256_224_u8_f32_" + ("pixel_major" if il else "planar")] = r
        del kept[:]
    x0, y0, w2 = 1000, 1500, 2048
    a16 = torch.empty((w2, w2, 4), dtype=torch.float16, device="cuda")
    b16 = torch.empty((w2, w2, 4), dtype=torch.float16, device="cuda")
    r = alternating(lambda: img16.get_region(x0, y0, w2, w2, out=a16, interleaved=True),
                    lambda: img16.get_region(x0, y0, w2, w2, out=b16, interleaved=True, dtype=np.float16), False)
    r["bit_equal"] = bool(torch.equal(a16.view(torch.int16), b16.view(torch.int16)))
    r["result_bytes"] = a16.numel() * 2
    r["old_temporary_bytes"] = a16.numel() * 2                                            # the scratch planes the interleave launch reads
    out["crop_2048_f16x4_pixel_major"] = r
    return out


def typed_write_leg():
    """(9): typed writes of the device classes against the route without them"""
    import ctypes as C
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec_m = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec_m)
    spec_m.loader.exec_module(ci)
    m = 4096
    planes8 = np.stack([synth.tiled_channel(np.uint8, m, m, c=k) for k in range(3)])
    dev8 = torch.from_numpy(planes8).cuda()
    L = hip.load()
    L.cimg_shared_engine.restype = C.c_void_p
    se = hip.Engine.__new__(hip.Engine)                    # the module's engine, for its kernel times
    se.handle = C.c_void_p(L.cimg_shared_engine())
    every = range(len(hip.KERNELS))
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def alternating(old, new, old_has_torch, patch=None):
        old(); new()
        torch.cuda.synchronize()
        se.enable_timing(1)
        rows = {"old": ([], [], []), "typed": ([], [], [])}
        for _ in range(REPS):
            for name, f in (("old", old), ("typed", new)):
                se.reset_timing()
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                rows[name][0].append((time.perf_counter() - t) * 1e6)
                k = sum(se.kernel_time(kid)[0] for kid in every) * 1e3
                rows[name][1].append(k + (ev_a.elapsed_time(ev_b) * 1e3 if name == "old" and old_has_torch else 0.0))
                rows[name][2].append(sum(se.kernel_time(kid)[0] for kid in (hip.K_UPDATE_PATCH_STRIDED, hip.K_UPDATE_PATCH_TYPED)) * 1e3)
        se.enable_timing(0)
        return {name: dict(wall_us=round(float(np.median(wl)), 1), wall_min_us=round(float(np.min(wl)), 1), wall_max_us=round(float(np.max(wl)), 1),
                           kernel_us=round(float(np.median(kl)), 1), patch_kernel_us=round(float(np.median(pl)), 1))
                for name, (wl, kl, pl) in rows.items()}

    out = {}
    rng = np.random.default_rng(9)
    N, c = 256, 224
    xs, ys = rng.integers(0, m - c, N), rng.integers(0, m - c, N)
    scale, offset = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]
    sc_t = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    of_t = torch.tensor(offset, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    # the source: what a network hands back -- normalised floats around the crops' own pixels, some out of range
    noise = torch.from_numpy(rng.normal(0.0, 0.02, (N, 3, c, c)).astype(np.float32)).cuda()
    for il in (False, True):
        img_old = ci.DeviceImage(np.uint8, dev8, m, m)
        img_new = ci.DeviceImage(np.uint8, dev8, m, m)
        planar = img_old.get_regions(xs, ys, c, c, dtype=np.float32, scale=scale, offset=offset)
        planar = torch.as_tensor(planar, device="cuda") + noise
        src = planar.permute(0, 2, 3, 1).contiguous() if il else planar
        kept = []

        def old():
            ev_a.record()
            p = src.permute(0, 3, 1, 2).contiguous() if il else src
            u = p.sub(of_t).div_(sc_t).round_().clamp_(0, 255).to(torch.uint8)
            kept[:] = [u]
            ev_b.record()
            img_old.set_regions(xs, ys, u)

        def new():
            img_new.set_regions(xs, ys, src, dtype=np.float32, scale=scale, offset=offset, interleaved=il)

        r = alternating(old, new, True)
        r["pixels_equal"] = bool(torch.equal(torch.as_tensor(img_old.get_decompressed(), device="cuda"), torch.as_tensor(img_new.get_decompressed(), device="cuda")))
        r["source_bytes"] = src.numel() * 4
        r["old_temporary_bytes"] = kept[0].numel() * (1 + 4) + (src.numel() * 4 if il else 0)     # the float result of sub and the uint8 copy; and the planar floats under permute
        out["crops256_224_f32_u8_" + ("pixel_major" if il else "planar")] = r
        del kept[:], img_old, img_new
    # the patch launch alone: an all-identity call through both kernels
    img_a = ci.DeviceImage(np.uint8, dev8, m, m)
    img_b = ci.DeviceImage(np.uint8, dev8, m, m)
    u8 = torch.as_tensor(img_a.get_regions(xs, ys, c, c), device="cuda")
    r = alternating(lambda: img_a.set_regions(xs, ys, u8), lambda: img_b.set_regions(xs, ys, u8, dtype=np.uint8), False)
    out["crops256_224_u8_identity"] = r
    return out


def masked_leg():
    """(10): fill_region and set_region(mask=) of DeviceChannel against the compositions they replace"""
    import ctypes as C
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec_m = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec_m)
    spec_m.loader.exec_module(ci)
    L = hip.load()
    L.cimg_shared_engine.restype = C.c_void_p
    se = hip.Engine.__new__(hip.Engine)                    # the module's engine, for its kernel times
    se.handle = C.c_void_p(L.cimg_shared_engine())
    every = range(len(hip.KERNELS))
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def alternating(old, new, old_has_torch):
        old(); new()
        torch.cuda.synchronize()
        se.enable_timing(1)
        rows = {"old": ([], []), "new": ([], [])}
        for _ in range(REPS):
            for name, f in (("old", old), ("new", new)):
                se.reset_timing()
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                rows[name][0].append((time.perf_counter() - t) * 1e6)
                k = sum(se.kernel_time(kid)[0] for kid in every) * 1e3
                rows[name][1].append(k + (ev_a.elapsed_time(ev_b) * 1e3 if name == "old" and old_has_torch else 0.0))
        se.enable_timing(0)
        return {name: dict(wall_us=round(float(np.median(wl)), 1), wall_min_us=round(float(np.min(wl)), 1), wall_max_us=round(float(np.max(wl)), 1),
                           kernel_us=round(float(np.median(kl)), 1)) for name, (wl, kl) in rows.items()}

    out = {}
    rng = np.random.default_rng(10)
    for name, dtype, m, (x, y, w, h) in (("f32_16384_region1024", np.float32, 16384, (5000, 7000, 1024, 1024)), ("u8_4096_whole", np.uint8, 4096, (0, 0, 4096, 4096))):
        host_plane = synth.tiled_channel(dtype, m, m)
        # Channel (host-resident chunks, numpy arrays): the old routes cross PCIe with h x w pixels, the fill with none
        hc_old = ci.Channel(host_plane, m, m)
        hc_new = ci.Channel(host_plane, m, m)
        r = alternating(lambda: hc_old.set_region(x, y, np.full((h, w), 7, dtype)), lambda: hc_new.fill_region(x, y, w, h, 7), False)
        r["pixels_equal"] = bool(np.array_equal(hc_old.get_region(x, y, w, h), hc_new.get_region(x, y, w, h)))
        out["channel_fill_" + name] = r
        hmask = rng.random((h, w)) < 0.5
        hnew = np.ascontiguousarray(hc_old.get_region(x, y, w, h)[::-1])
        r = alternating(lambda: hc_old.set_region(x, y, np.where(hmask, hnew, hc_old.get_region(x, y, w, h))),
                        lambda: hc_new.set_region(x, y, hnew, mask=hmask), False)
        r["pixels_equal"] = bool(np.array_equal(hc_old.get_region(x, y, w, h), hc_new.get_region(x, y, w, h)))
        out["channel_masked_" + name] = r
        del hc_old, hc_new
        plane = torch.from_numpy(host_plane).cuda()
        del host_plane
        ch_old = ci.DeviceChannel(plane, m, m)
        ch_new = ci.DeviceChannel(plane, m, m)
        del plane
        tdt = torch.float32 if dtype is np.float32 else torch.uint8
        # fill: the parent's only way materialises h x w copies of the scalar
        def old_fill():
            ev_a.record()
            c = torch.full((h, w), 7, dtype=tdt, device="cuda")
            ev_b.record()
            ch_old.set_region(x, y, c)
        r = alternating(old_fill, lambda: ch_new.fill_region(x, y, w, h, 7), True)
        r["pixels_equal"] = bool(torch.equal(torch.as_tensor(ch_old.get_region(x, y, w, h), device="cuda"), torch.as_tensor(ch_new.get_region(x, y, w, h), device="cuda")))
        out["fill_" + name] = r
        # masked write: get_region + where + set_region against set_region(mask=)
        mask = torch.from_numpy(rng.random((h, w)) < 0.5).cuda()
        new_px = torch.as_tensor(ch_old.get_region(x, y, w, h), device="cuda").flip(0).contiguous()
        def old_masked():
            cur = torch.as_tensor(ch_old.get_region(x, y, w, h), device="cuda")
            ev_a.record()
            mixed = torch.where(mask, new_px, cur)
            ev_b.record()
            ch_old.set_region(x, y, mixed)
        r = alternating(old_masked, lambda: ch_new.set_region(x, y, new_px, mask=mask), True)
        r["pixels_equal"] = bool(torch.equal(torch.as_tensor(ch_old.get_region(x, y, w, h), device="cuda"), torch.as_tensor(ch_new.get_region(x, y, w, h), device="cuda")))
        out["masked_" + name] = r
        del ch_old, ch_new
    return out


if MASKED_LEG:
    line = json.dumps(masked_leg())
    print("MASKED " + line)
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "masked", "diag_windows_masked.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(line + "\n")
    sys.exit(0)

if TYPED_WRITE_LEG:
    line = json.dumps(typed_write_leg())
    print("TYPED_WRITE " + line)
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "typed", "diag_windows_typed_write.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(line + "\n")
    sys.exit(0)

if TYPED_LEG:
    line = json.dumps(typed_leg())
    print("TYPED " + line)
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "typed", "diag_windows_typed.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(line + "\n")
    sys.exit(0)

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


def write_strided_leg():
    """(7), in the child process: strided and batched writes against the routes they replace"""
    out = {}
    rng = np.random.default_rng(7)

    def alternating(fa, fb, ka, kb):
        """fa and fb in turn, REPS times after a warm-up of each -> per call: wall median, wall max - min, kernel median (us)"""
        fa(); fb()
        eng.enable_timing(1)
        wa, wb, qa, qb = [], [], [], []
        for _ in range(REPS):
            for f, ws, ks, kid in ((fa, wa, qa, ka), (fb, wb, qb, kb)):
                eng.reset_timing()
                t = time.perf_counter()
                f()
                ws.append((time.perf_counter() - t) * 1e6)
                ks.append(eng.kernel_time(kid)[0] * 1e3)
        eng.enable_timing(0)
        return [dict(wall_us=round(float(np.median(x)), 1), wall_spread_us=round(float(max(x) - min(x)), 1), patch_kernel_us=round(float(np.median(k)), 1))
                for x, k in ((wa, qa), (wb, qb))]

    # the 1024^2 window of (3), col_pitch 1 against the plain call
    win = rng.integers(0, 1 << 20, (w, w)).astype(np.float32)
    d_src, d_new = eng.alloc(win.nbytes), eng.alloc(nch * dest)
    d_src.upload(win.view(np.uint8).ravel())
    args = (hip.cparams(4), d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, [chunk + 32] * nch)
    plain, strd = alternating(lambda: eng.update_windows_device(*args, [spec], d_src.ptr, d_new.ptr, comp_off, comp_size=cb),
                              lambda: eng.update_windows_strided_device(*args, [dict(spec, col_pitch=1)], d_src.ptr, d_new.ptr, comp_off, comp_size=cb),
                              hip.K_UPDATE_PATCH, hip.K_UPDATE_PATCH_STRIDED)
    out["window_1024_plain"], out["window_1024_col_pitch_1"] = plain, strd
    d_src.free(); d_new.free()
    # 4096 distinct pixels into a 4096^2 float16 plane
    m = 4096
    plane = np.ascontiguousarray(synth.tiled_channel(np.float16, m, m)).view(np.uint8).ravel()
    k16 = plane.size // chunk
    off16 = np.arange(k16, dtype=np.int64) * dest
    d_p, d_c, d_n = eng.alloc(plane.size), eng.alloc(k16 * dest), eng.alloc(k16 * dest)
    d_p.upload(plane)
    cb16 = eng.compress_device(hip.cparams(2), d_p.ptr, np.arange(k16, dtype=np.int64) * chunk, [chunk] * k16, d_c.ptr, off16, [dest] * k16)
    at = rng.choice(m * m, 4096, replace=False)
    px = [dict(chunk_first=0, chunk_count=k16, origin=int(a), row_pitch=1, width=1, height=1, out_off=2 * i, out_pitch=2) for i, a in enumerate(at)]
    d_v = eng.alloc(2 * 4096)
    d_v.upload(rng.integers(0, 255, 2 * 4096, dtype=np.uint8))
    # (the C entry points called directly over window tables built once: 4096 dicts to ctypes cost more than the call itself)
    import ctypes as C
    lib, p2 = hip.load(), hip.cparams(2)
    i32, i64, ptr = hip._i32, hip._i64, hip._ptr
    nb16, bs16, ds16, cs16, o16 = i32([chunk] * k16), i32([32768] * k16), i32([chunk + 32] * k16), i32(cb16), i64(off16)
    ncb, st = np.zeros(k16, np.int32), np.zeros(k16, np.int32)
    wp, wstr = hip.windows(px), hip.strided_windows([dict(q, col_pitch=1) for q in px])

    def direct(fn, wt):
        def f():
            rc = fn(eng.handle, C.byref(p2), k16, d_c.ptr, ptr(o16), ptr(cs16), ptr(nb16), ptr(bs16), ptr(ds16), len(px), wt, d_v.ptr, d_n.ptr,
                    ptr(o16), ptr(ncb), ptr(st))
            assert rc == 0, rc
        return f

    plain, strd = alternating(direct(lib.cimg_update_windows_device, wp), direct(lib.cimg_update_windows_strided_device, wstr),
                              hip.K_UPDATE_PATCH, hip.K_UPDATE_PATCH_STRIDED)
    out["pixels4096_plain"], out["pixels4096_strided"] = plain, strd
    out["pixels4096_blocks_encoded"] = eng.update_stats()["blocks_encoded"]
    for b in (d_p, d_c, d_n, d_v):
        b.free()
    # every 4th pixel of a 2048^2 region through the module, against get_region + scatter + set_region
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec_m = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec_m)
    spec_m.loader.exec_module(ci)
    dch = ci.DeviceChannel(torch.from_numpy(plane.view(np.float16).reshape(m, m)).cuda(), m, m, block_size=32768, chunk_size=chunk)
    sub = torch.from_numpy(rng.integers(0, 1000, (512, 512)).astype(np.float16)).cuda()

    def new_route():
        dch.set_region(1024, 1024, sub, step_x=4, step_y=4)

    def old_route():
        r = torch.as_tensor(dch.get_region(1024, 1024, 2048, 2048), device="cuda")
        r[::4, ::4] = sub
        dch.set_region(1024, 1024, r)

    for name, fn in (("subsample_set_region_steps", new_route), ("subsample_get_scatter_set", old_route)):
        fn()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e6)
        out[name] = dict(wall_us=round(float(np.median(ts)), 1), wall_spread_us=round(float(max(ts) - min(ts)), 1))
    want = plane.view(np.float16).reshape(m, m).copy()
    want[1024:3072:4, 1024:3072:4] = sub.cpu().numpy()
    assert np.array_equal(torch.as_tensor(dch.get_decompressed(), device="cuda").cpu().numpy(), want)
    return out


def strided_leg():
    """(5), in the child process: the plane decoded into a torch tensor and subsampled there, against the strided window call"""
    step = 16
    sw = n // step
    full = torch.empty(n * n, dtype=torch.float32, device="cuda")
    d_sub = eng.alloc(sw * sw * 4)
    sspec = dict(chunk_first=0, chunk_count=nch, origin=0, row_pitch=step * n, col_pitch=step, width=sw, height=sw, out_off=0, out_pitch=sw * 4)
    str_k, str_w = timed(lambda: eng.decompress_windows_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, 4, [sspec], d_sub.ptr,
                                                               comp_size=cb, strided=True), (hip.K_DECODE_WINDOW_STRIDED,))
    stats = eng.window_stats()
    assert np.array_equal(d_sub.download().view(np.float32).reshape(sw, sw), img[::step, ::step])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_us, kept = [], []

    def parent_route():
        eng.decompress_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, full.data_ptr(), raw_off, comp_size=cb)
        a.record()
        sub = full.view(n, n)[::step, ::step].contiguous()
        b.record()
        torch.cuda.synchronize()
        copy_us.append(a.elapsed_time(b) * 1e3)
        kept[:] = [sub]

    dec_k, par_w = timed(parent_route, (hip.K_DECODE, hip.K_DECODE_ZSTD))
    assert np.array_equal(kept[0].cpu().numpy(), img[::step, ::step])
    par_k = dec_k + float(np.median(copy_us[1:]))
    d_sub.free()
    return dict(strided_kernel_us=round(str_k, 1), strided_wall_us=round(str_w, 1), strided_blocks=stats["blocks_decoded"],
                strided_chunks_whole=stats["chunks_whole"], parent_decode_kernel_us=round(dec_k, 1),
                parent_copy_kernel_us=round(float(np.median(copy_us[1:])), 1), parent_kernel_us=round(par_k, 1), parent_wall_us=round(par_w, 1),
                strided_kernel_ratio=round(par_k / str_k, 2), strided_wall_ratio=round(par_w / str_w, 2))


def grouped_leg():
    """(6), in the child process: many regions a call, grouped against strided, whole decode + torch indexing, and N single calls"""
    rng = np.random.default_rng(6)
    cases = {
        "tiles16_1024": [(1024 * k, 7000, 1024, 1024) for k in range(16)],
        "crops64_256": [(int(x), int(y), 256, 256) for x, y in zip(rng.integers(0, n - 256, 64), rng.integers(0, n - 256, 64))],
        "pixels4096": [(int(x), int(y), 1, 1) for x, y in zip(rng.integers(0, n, 4096), rng.integers(0, n, 4096))],
        # a 32 KiB block is half a row: windows in different rows, or in the two halves of the same rows, share none
        "disjoint64": [(1000 + (k % 2) * 8192, 200 * (k // 2), 256, 64) for k in range(64)],
    }
    full = torch.empty(n * n, dtype=torch.float32, device="cuda")
    plane_t = torch.from_numpy(img).cuda()
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec_m = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec_m)
    spec_m.loader.exec_module(ci)
    dch = ci.DeviceChannel(plane_t, n, n, block_size=32768, chunk_size=chunk)
    del plane_t
    out = {}

    def timed_all(fn, kernels, extra=None):
        """extra: a function that returns the microseconds of the kernels fn ran outside the engine (torch's, from events)"""
        fn()
        eng.enable_timing(1)
        walls, kus = [], []
        for _ in range(REPS):
            eng.reset_timing()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t) * 1e6)
            kus.append(sum(eng.kernel_time(k)[0] for k in kernels) * 1e3 + (extra() if extra else 0.0))
        eng.enable_timing(0)
        return dict(kernel_us=round(float(np.median(kus)), 1), wall_us=round(float(np.median(walls)), 1),
                    wall_min_us=round(float(np.min(walls)), 1), wall_max_us=round(float(np.max(walls)), 1),
                    kernel_min_us=round(float(np.min(kus)), 1), kernel_max_us=round(float(np.max(kus)), 1))

    for name, regs in cases.items():
        specs, at = [], 0
        for (x, y, w_, h_) in regs:
            specs.append(dict(chunk_first=0, chunk_count=nch, origin=y * n + x, row_pitch=n, col_pitch=1, width=w_, height=h_, out_off=at,
                              out_pitch=w_ * 4))
            at += w_ * h_ * 4
        d_out = eng.alloc(at)
        want = np.concatenate([img[y:y + h_, x:x + w_].ravel() for (x, y, w_, h_) in regs])
        r = {"regions": len(regs), "out_bytes": at}
        for kind, kid in (("grouped", hip.K_DECODE_WINDOW_GROUPED), ("strided", hip.K_DECODE_WINDOW_STRIDED)):
            d_out.upload(np.zeros(at, np.uint8))
            call = lambda: eng.decompress_windows_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, 4, specs, d_out.ptr, comp_size=cb,  # noqa: E731
                                                         strided=kind == "strided", grouped=kind == "grouped")
            r[kind] = timed_all(call, (kid,))
            r[kind]["blocks"] = eng.window_stats()["blocks_decoded"]
            assert np.array_equal(d_out.download().view(np.float32), want), (name, kind)
        d_out.free()
        xs, ys = [g[0] for g in regs], [g[1] for g in regs]
        w_, h_ = regs[0][2], regs[0][3]
        kept = []
        ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def whole_route():
            eng.decompress_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, full.data_ptr(), raw_off, comp_size=cb)
            f2 = full.view(n, n)
            ev_a.record()                                  # torch's part (index upload, gather or stack) between two events
            if w_ == 1:
                kept[:] = [f2[torch.as_tensor(ys, device="cuda"), torch.as_tensor(xs, device="cuda")]]
            else:
                kept[:] = [torch.stack([f2[y:y + h_, x:x + w_] for x, y in zip(xs, ys)])]
            ev_b.record()

        index_us = []

        def torch_part():                                  # (timed_all has synchronized)
            index_us.append(ev_a.elapsed_time(ev_b) * 1e3)
            return index_us[-1]

        r["whole_decode_torch_index"] = timed_all(whole_route, (hip.K_DECODE, hip.K_DECODE_ZSTD), torch_part)
        r["whole_decode_torch_index"]["index_us"] = round(float(np.median(index_us)), 1)
        assert np.array_equal(kept[0].cpu().numpy().ravel(), want), name
        res_t = torch.empty(at // 4, dtype=torch.float32, device="cuda")

        def singles():
            o = 0
            for (x, y, ww, hh) in regs:
                dch.get_region(x, y, ww, hh, out=res_t[o:o + ww * hh].view(hh, ww))
                o += ww * hh

        r["single_get_region_calls"] = timed_all(singles, ())
        assert np.array_equal(res_t.cpu().numpy(), want), name
        if w_ == 1:
            r["device_channel_batched"] = timed_all(lambda: dch.get_pixels(xs, ys, out=res_t), ())
        else:
            r["device_channel_batched"] = timed_all(lambda: dch.get_regions(xs, ys, w_, h_, out=res_t.view(len(regs), h_, w_)), ())
        assert np.array_equal(res_t.cpu().numpy(), want), name
        out[name] = r
    return out


if GROUPED_LEG:
    line = json.dumps(grouped_leg())
    print("GROUPED " + line)
    if "--out" in sys.argv:
        dst = sys.argv[sys.argv.index("--out") + 1]
    else:
        dst = os.path.join(ROOT, "profiles", "grouped", "diag_windows_grouped.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(line + "\n")
    d_raw.free(); d_comp.free(); d_win.free()
    eng.close()
    sys.exit(0)

if WRITE_STRIDED_LEG:
    line = json.dumps(write_strided_leg())
    print("WSTRIDED " + line)
    if "--out" in sys.argv:
        open(sys.argv[sys.argv.index("--out") + 1], "w").write(line + "\n")
    d_raw.free(); d_comp.free(); d_win.free()
    eng.close()
    sys.exit(0)

if STRIDED_LEG:
    print("STRIDED " + json.dumps(strided_leg()))
    d_raw.free(); d_comp.free(); d_win.free()
    eng.close()
    sys.exit(0)

full_k, full_w = timed(lambda: eng.decompress_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, d_raw.ptr, raw_off, comp_size=cb),
                       (hip.K_DECODE, hip.K_DECODE_ZSTD))
win_k, win_w = timed(lambda: eng.decompress_windows_device(d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, 4, [spec], d_win.ptr, comp_size=cb),
                     (hip.K_DECODE_WINDOW,))
got = d_win.download().view(np.float32).reshape(w, w)
assert np.array_equal(got, img[y0:y0 + w, x0:x0 + w])
res.update(full_decode_kernel_us=round(full_k, 1), full_decode_wall_us=round(full_w, 1), window_kernel_us=round(win_k, 1),
           window_wall_us=round(win_w, 1), window_blocks=eng.window_stats()["blocks_decoded"], plane_blocks=nch * (chunk // 32768),
           kernel_ratio=round(full_k / win_k, 2), wall_ratio=round(full_w / win_w, 2))
# (3) write: a 1024^2 window into the plane, against decode + compress of the chunks it touches
rows = chunk // (n * 4)
first, last = y0 // rows, (y0 + w - 1) // rows
tc = list(range(first, last + 1))
win = np.random.default_rng(1).integers(0, 1 << 20, (w, w)).astype(np.float32)
d_src = eng.alloc(w * w * 4)
d_src.upload(win.view(np.uint8).ravel())
d_new = eng.alloc(nch * dest)
wspec = dict(spec, out_off=0, out_pitch=w * 4)
upd_k, upd_w = timed(lambda: eng.update_windows_device(hip.cparams(4), d_comp.ptr, comp_off, [chunk] * nch, [32768] * nch, [chunk + 32] * nch,
                                                       [wspec], d_src.ptr, d_new.ptr, comp_off, comp_size=cb),
                     (hip.K_UPDATE_PATCH, hip.K_UPDATE_LAYOUT, hip.K_UPDATE_EMIT, hip.K_ENCODE, hip.K_DECODE, hip.K_DECODE_ZSTD, hip.K_LAYOUT,
                      hip.K_EMIT))
ust = eng.update_stats()
tco, tro = comp_off[tc], np.arange(len(tc), dtype=np.int64) * chunk


def round_trip():
    eng.decompress_device(d_comp.ptr, tco, [chunk] * len(tc), [32768] * len(tc), d_raw.ptr, tro, comp_size=cb[tc])
    eng.compress_device(hip.cparams(4), d_raw.ptr, tro, [chunk] * len(tc), d_new.ptr, tco, [chunk + 32] * len(tc))


rt_k, rt_w = timed(round_trip, (hip.K_DECODE, hip.K_DECODE_ZSTD, hip.K_ENCODE, hip.K_LAYOUT, hip.K_EMIT))
res.update(write_chunks=len(tc), write_blocks_decoded=ust["blocks_decoded"], write_blocks_encoded=ust["blocks_encoded"],
           write_chunks_whole=ust["chunks_whole"], write_kernel_us=round(upd_k, 1), write_wall_us=round(upd_w, 1),
           roundtrip_kernel_us=round(rt_k, 1), roundtrip_wall_us=round(rt_w, 1), write_kernel_ratio=round(rt_k / upd_k, 2),
           write_wall_ratio=round(rt_w / upd_w, 2))
d_src.free(); d_new.free()
d_raw.free(); d_comp.free(); d_win.free()

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
# (5), host class: every 8th pixel of every 8th row
sub_us, a = wall(lambda: ch.get_region(0, 0, 4096, 4096, step_x=8, step_y=8))
dsub_us, b = wall(lambda: ch.get_decompressed()[::8, ::8].copy())
assert np.array_equal(a, b) and np.array_equal(a, arr[::8, ::8])
res.update(region_step8_wall_us=round(sub_us, 1), decompressed_step8_wall_us=round(dsub_us, 1), region_step8_speedup=round(dsub_us / sub_us, 2))

# (4) write through the module: set_region against get_chunk + edit + set_chunk of the chunk it lies in (chunk 2: rows 1024 .. 1535)
for side in (64, 512):
    p = np.random.default_rng(side).integers(0, 1000, (side, side)).astype(np.float16)
    set_us, _ = wall(lambda: ch.set_region(1024, 1024, p))

    def chunk_trip():
        c = ch.get_chunk(2).reshape(512, 4096)
        c[:side, 1024:1024 + side] = p
        ch.set_chunk(2, c.ravel())

    trip_us, _ = wall(chunk_trip)
    res["set_region_%d_wall_us" % side] = round(set_us, 1)
    res["chunk_trip_%d_wall_us" % side] = round(trip_us, 1)
    res["set_region_%d_speedup" % side] = round(trip_us / set_us, 2)
ref = arr.copy()
ref[1024:1536, 1024:1536] = np.random.default_rng(512).integers(0, 1000, (512, 512)).astype(np.float16)
assert np.array_equal(ch.get_decompressed(), ref)
# the host call's traffic for the 64^2 window: the touched chunk up, the window up, the new chunk down
plane16 = np.ascontiguousarray(arr).view(np.uint8).ravel()
chunks16 = eng.compress_host(hip.cparams(2), plane16, [chunk] * 8, [chunk + 32] * 8)
src16 = np.random.default_rng(2).integers(0, 1000, (64, 64)).astype(np.float16).view(np.uint8).ravel()
new16, _ = eng.update_windows_host(hip.cparams(2), chunks16, [chunk + 32] * 8, [dict(chunk_first=0, chunk_count=8, origin=1024 * 4096 + 1024,
                                   row_pitch=4096, width=64, height=64, out_off=0, out_pitch=128)], src16)
hst = eng.update_stats()
res.update(host_64_bytes_up=hst["bytes_uploaded"], host_64_bytes_down=sum(len(c) for c in new16 if c is not None),
           host_64_blocks_decoded=hst["blocks_decoded"], chunk_trip_bytes_each_way=chunk + len(chunks16[2]))
eng.close()
# (5), device: in a process of its own
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--strided-leg"], capture_output=True, text=True, timeout=900)
got = [ln for ln in child.stdout.splitlines() if ln.startswith("STRIDED ")]
assert child.returncode == 0 and got, child.stdout[-2000:] + child.stderr[-4000:]
res.update(json.loads(got[0][len("STRIDED "):]))
# (6): in a process of its own; it writes profiles/grouped/diag_windows_grouped.json itself
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--grouped-leg"], capture_output=True, text=True, timeout=1800)
got = [ln for ln in child.stdout.splitlines() if ln.startswith("GROUPED ")]
assert child.returncode == 0 and got, child.stdout[-2000:] + child.stderr[-4000:]
res["grouped"] = json.loads(got[0][len("GROUPED "):])
# (7): in a process of its own
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--write-strided-leg"], capture_output=True, text=True, timeout=1800)
got = [ln for ln in child.stdout.splitlines() if ln.startswith("WSTRIDED ")]
assert child.returncode == 0 and got, child.stdout[-2000:] + child.stderr[-4000:]
res["write_strided"] = json.loads(got[0][len("WSTRIDED "):])
line = json.dumps(res)
print(line)
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    open(sys.argv[2], "w").write(line + "\n")
