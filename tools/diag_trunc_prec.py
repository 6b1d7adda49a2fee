"""blosc2's trunc-prec filter (csrc/trunc_kernel.h, csrc/trunc_plan.h) on one MI355X.  Medians of REPS calls after
warm-up, kernel times from the engine's HIP-event slots, everything in ONE process, torch imported first:
  (1) cimg_trunc_prec over 128 MiB of float32 in 4 MiB chunks: copied (a caller's device pixels, one launch) and in place (the staging
      area of a host call, one launch per upload group), in us and GB/s (read + written), against a torch device-to-device copy of the
      same bytes;
  (2) 4 x 4096^2 float32, the tiled and the natural family, lz4 and zstd, 12 and 16 mantissa bits kept against no filter: the encode
      launches' us, the decode launches' us, the pass's us and the compression ratio -- the rows where truncation does not pay included.
Prints one JSON line.  usage: python tools/diag_trunc_prec.py [--out file]"""
import json
import os
import sys

import torch  # (first: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd")]
import numpy as np  # noqa: E402
from cimg import hip, synth  # noqa: E402

REPS = 10
CHUNK = 4 << 20
res = {}
eng = hip.Engine(0)


def kernel_us(fn, kernels):
    """median over REPS calls of the event time of each of `kernels` (summed over its launches in the call)"""
    fn(); fn()
    eng.enable_timing(1)
    out = []
    for _ in range(REPS):
        eng.reset_timing()
        fn()
        out.append([eng.kernel_time(k)[0] * 1e3 for k in kernels])
    eng.enable_timing(0)
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


def geometry(nbytes):
    n = nbytes // CHUNK
    return (np.arange(n, dtype=np.int64) * CHUNK, np.arange(n, dtype=np.int64) * (CHUNK + 64), [CHUNK] * n, [CHUNK + 32] * n, [32768] * n)


def trunc_np(a, kept):
    v = a.view(np.uint32) & np.uint32(~((1 << (23 - kept)) - 1) & 0xFFFFFFFF)
    return v.view(np.float32)


# ---- (1) the pass alone ---------------------------------------------------------------------------------------------------------
n = 4096
plane = np.stack([synth.tiled_channel(np.float32, n, n) for _ in range(2)])                # 128 MiB
pix = plane.nbytes
t = torch.from_numpy(plane.view(np.int32)).cuda()
roff, coff, nb, ds, bs = geometry(pix)
d_comp = torch.empty(len(nb) * (CHUNK + 64), dtype=torch.uint8, device="cuda")
p12 = hip.cparams(4, trunc_prec=12)
us_copy_pass = kernel_us(lambda: eng.compress_device(p12, t.data_ptr(), roff, nb, d_comp.data_ptr(), coff, ds), [hip.K_TRUNC_PREC])[0]
flat = plane.view(np.uint8).ravel()
us_inplace_pass = kernel_us(lambda: eng.compress_host(p12, flat, nb, ds), [hip.K_TRUNC_PREC])[0]
eng.enable_timing(1)
eng.reset_timing()
eng.compress_host(p12, flat, nb, ds)
inplace_launches = int(eng.kernel_time(hip.K_TRUNC_PREC)[1])          # one per upload group of the host call
eng.enable_timing(0)
us_torch = torch_copy_us(pix)
res["pass_128MiB"] = {"bytes": pix, "torch_copy_us": round(us_torch, 1),
                      "copied": {"us": round(us_copy_pass, 1), "gbps": round(2 * pix / us_copy_pass / 1e3, 1), "fraction_of_copy": round(us_torch / us_copy_pass, 3)},
                      "in_place": {"us": round(us_inplace_pass, 1), "gbps": round(2 * pix / us_inplace_pass / 1e3, 1),
                                   "fraction_of_copy": round(us_torch / us_inplace_pass, 3), "launches_per_call": inplace_launches}}
del t, plane, flat

# ---- (2) end to end -----------------------------------------------------------------------------------------------------------------
rows = []
for family in ("tiled", "natural"):
    fn = synth.tiled_channel if family == "tiled" else synth.natural_channel
    img = np.stack([fn(np.float32, n, n, c) for c in range(4)])                            # 256 MiB
    pix = img.nbytes
    t = torch.from_numpy(img.view(np.int32)).cuda()
    out = torch.empty_like(t)
    roff, coff, nb, ds, bs = geometry(pix)
    d_comp = torch.empty(len(nb) * (CHUNK + 64), dtype=torch.uint8, device="cuda")
    for code, name, k_enc, k_dec in ((hip.LZ4, "lz4", hip.K_ENCODE, hip.K_DECODE), (hip.ZSTD, "zstd", hip.K_ENCODE_ZSTD, hip.K_DECODE_ZSTD)):
        for kept in (None, 12, 16):
            p = hip.cparams(4, compcode=code, trunc_prec=kept)
            cb = {}

            def enc():
                cb["v"] = eng.compress_device(p, t.data_ptr(), roff, nb, d_comp.data_ptr(), coff, ds)

            def dec():
                eng.decompress_device(d_comp.data_ptr(), coff, nb, bs, out.data_ptr(), roff, comp_size=cb["v"])

            us_enc, us_pass = kernel_us(enc, [k_enc, hip.K_TRUNC_PREC])
            us_dec = sum(kernel_us(dec, [k_dec] if code == hip.LZ4 else [hip.K_DECODE, k_dec]))
            want = img if kept is None else trunc_np(img, kept)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (family, name, kept)
            rows.append({"family": family, "codec": name, "mantissa_bits": kept, "encode_us": round(us_enc, 1), "pass_us": round(us_pass, 1),
                         "decode_us": round(us_dec, 1), "ratio": round(pix / float(np.sum(cb["v"])), 3)})
    del t, out, d_comp, img
res["end_to_end_4x4096x4096_float32"] = rows
eng.close()

line = json.dumps(res)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
