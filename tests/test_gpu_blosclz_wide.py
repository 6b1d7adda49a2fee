"""BloscLZ with blocks up to 256 KiB on the MI355X: cimg_encode_wide_blosclz (csrc/wide_kernel.h: blosclz_wide_encode) behind the
engine's planner routing, through every public layer -- batch C ABI (host, device, packed), the blosc2 shim, trunc-prec in front,
window writes, the Python module.

The bytes are pinned to BloscLZ 2.3.0 through tests/golden/blosclz_wide_kat.npz (make_blosclz_wide_golden.py) and to the oracle's
chunks (oracle/blosclz.c has no length limit; the golden's generator holds it equal to BloscLZ on every vector).  The CPU twin of
this file is tests/test_emu_blosclz_wide.py.  Every compress call here with BloscLZ and a stream above 65 535 bytes was refused
with -7 before the wide BloscLZ instance existed.  The C++ classes have no case of their own: the Python cases below drive
channel<T> / image<T> / device_channel<T> through the same calls.
Run on the GPU box:  python -m pytest tests/test_gpu_blosclz_wide.py -m gpu -q
"""
import hashlib
import importlib.util
import os
import struct
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import _oracle as O
import _trunc as T
from _blosclz_wide import CHUNKS, chunk_case, load_kat, load_stream_inputs
from _window_writes import expected, source
from cimg import hip, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1048576


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    return load_kat()


@pytest.fixture(scope="module")
def stream_inputs(kat):
    return load_stream_inputs(kat)


def params(ts, blk, clevel=9, split=O.AUTO_SPLIT, filt=O.SHUFFLE, **kw):
    return hip.cparams(ts, clevel=clevel, blocksize=blk, compcode=hip.BLOSCLZ, splitmode=split, filters=(0, 0, 0, 0, 0, filt), **kw)


STREAMS = [("steps|65535", (1, 5, 9)), ("steps|65536", (1, 5, 9)), ("steps|65537", (1, 5, 9)),
           ("far|100000|8191", (9,)), ("far|100000|8192", (9,)), ("far|100000|73724", (5, 9)), ("far|100000|73725", (5, 9)),
           ("far|262144|73724", (9,)), ("far|262144|73725", (9,)),
           ("tiled_u16_hi|262144", (5, 9)), ("natural_u16_hi|200001", (9,)), ("period|131072", (1, 9)), ("steps|98304", (9,)),
           ("walk|262144", (9,)), ("random|131072", (9,))]


def test_stream_vectors_through_the_gpu_encoder(eng, kat, stream_inputs):
    """Each vector as the one stream of a 1-byte, unshuffled chunk: the chunk's stream bytes are BloscLZ's, the chunk the oracle's."""
    coded = 0
    for name, clevels in STREAMS:
        src = np.ascontiguousarray(stream_inputs[name])
        n = src.size
        for clevel in clevels:
            want_len = int(kat[f"len|{name}|{clevel}"])
            (c,) = eng.compress_host(params(1, n, clevel=clevel, filt=O.NOFILTER), src, [n], [n + 64])
            r, ref = O.compress(O.cparams(1, clevel=clevel, blocksize=n, compcode=O.BLOSCLZ, filters=(0,) * 6), src, destsize=n + 64)
            assert r > 0 and c == ref, (name, clevel)
            bstart = struct.unpack_from("<i", c, 32)[0]
            cs = struct.unpack_from("<i", c, bstart)[0]
            if want_len:                                   # BloscLZ codes it: the chunk holds that payload
                assert cs == want_len, (name, clevel)
                assert hashlib.sha256(c[bstart + 4:bstart + 4 + cs]).hexdigest() == str(kat[f"sha256|{name}|{clevel}"]), (name, clevel)
                coded += 1
            else:
                assert cs == n, (name, clevel)             # BloscLZ gives up: the stream is stored raw
            outs, st = eng.decompress_host([c])
            assert st[0] == 0 and outs[0].tobytes() == src.tobytes(), (name, clevel)
    assert coded >= 20


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_host_chunks_equal_the_oracle(eng, name):
    for clevel in ((9, 5) if name in ("u8_natural_b262144", "f16_tiled_b262144") else (9,)):
        raw, ts, blk, split, filt, want = chunk_case(name, clevel)
        (c,) = eng.compress_host(params(ts, blk, clevel, split, filt), raw, [raw.size], [raw.size + 32])
        assert c == want, (name, clevel)
        outs, st = eng.decompress_host([c])
        assert st[0] == 0 and outs[0].tobytes() == raw.tobytes(), name
        r, back = O.decompress(c)
        assert r == raw.size and back.tobytes() == raw.tobytes(), name


def test_destsizes_around_cbytes(eng):
    raw, ts, blk, split, filt, want = chunk_case("f16_natural_b262144")
    op = O.cparams(2, blocksize=262144, compcode=O.BLOSCLZ)
    full = len(want)
    seen = set()
    for dest in (full + 1, full, full - 1, full - 4096):
        r, ref = O.compress(op, raw, destsize=dest)
        (c,) = eng.compress_host(params(2, 262144), raw, [raw.size], [dest])
        assert c == ref, dest
        seen.add(r > 0)
    assert seen == {True, False}


def _batch():
    """three chunks of one geometry (float16, 256 KiB blocks): natural, tiled, natural mirrored"""
    a = chunk_case("f16_natural_b262144")[0]
    b = chunk_case("f16_tiled_b262144")[0]
    c = np.ascontiguousarray(a.view(np.float16)[::-1]).view(np.uint8)
    raws = [a, b, c]
    op = O.cparams(2, blocksize=262144, compcode=O.BLOSCLZ)
    want = [O.compress(op, r)[1] for r in raws]
    return raws, want


def test_device_and_packed_calls(eng):
    raws, want = _batch()
    host = np.concatenate(raws)
    n, chunk = len(raws), raws[0].size
    nbytes, dest = [chunk] * n, chunk + 32
    raw_off = np.arange(n, dtype=np.int64) * chunk
    comp_off = np.arange(n, dtype=np.int64) * (dest + 32)
    p = params(2, 262144)
    d_raw, d_comp, d_out = eng.alloc(host.size), eng.alloc(n * (dest + 32)), eng.alloc(host.size)
    try:
        d_raw.upload(host)
        cb = eng.compress_device(p, d_raw.ptr, raw_off, nbytes, d_comp.ptr, comp_off, [dest] * n)
        comp = d_comp.download()
        got = [comp[o:o + c].tobytes() for o, c in zip(comp_off, cb)]
        assert got == want
        (ch,) = eng.compress_host(p, raws[0], [chunk], [dest])                 # the first chunk against the host path
        assert got[0] == ch
        st = eng.decompress_device(d_comp.ptr, comp_off, nbytes, [262144] * n, d_out.ptr, raw_off, comp_size=cb)
        assert (st == 0).all() and np.array_equal(d_out.download(), host)
        # the two-step form
        eng.compress_device_begin(p, d_raw.ptr, raw_off, nbytes, d_comp.ptr, comp_off, [dest] * n)
        assert np.array_equal(eng.compress_device_fetch(n), cb)
        # packed: sizes first, then an exact-size store
        cbp = eng.compress_device_packed_begin(p, d_raw.ptr, raw_off, nbytes, [dest] * n)
        assert np.array_equal(cbp, cb)
        doff = np.concatenate([[3], 3 + np.cumsum(cbp[:-1].astype(np.int64) + 5)]).astype(np.int64)
        d_store = eng.alloc(int(doff[-1]) + int(cbp[-1]) + 16)
        eng.compress_device_packed_fetch(n, d_store.ptr, doff)
        store = d_store.download()
        assert [store[o:o + c].tobytes() for o, c in zip(doff, cbp)] == want
        d_store.free()
    finally:
        for d in (d_raw, d_comp, d_out):
            d.free()


def test_blosc2_ctx_calls_with_256k_blocks(eng):
    L = hip.load()
    cp = hip.Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = 0, 9, 2, 4, 262144, 3
    cp.filters[5] = 1
    cctx = L.blosc2_create_cctx(cp)
    dp = hip.Blosc2DParams()
    dp.nthreads = 1
    dctx = L.blosc2_create_dctx(dp)
    raw, _, _, _, _, want = chunk_case("f16_natural_b262144")
    src = np.ascontiguousarray(raw)
    dst = np.zeros(src.size + 32, np.uint8)
    r = L.blosc2_compress_ctx(cctx, src.ctypes.data, src.size, dst.ctypes.data, dst.size)
    assert r == len(want) and dst[:r].tobytes() == want
    # BLOSC_BLOSCLZ and a 128 KiB block of bytes
    cp.typesize, cp.blocksize = 1, 131072
    cctx1 = L.blosc2_create_cctx(cp)
    raw1, _, _, _, _, want1 = chunk_case("u8_natural_b131072")
    src1 = np.ascontiguousarray(raw1)
    r1 = L.blosc2_compress_ctx(cctx1, src1.ctypes.data, src1.size, dst.ctypes.data, dst.size)
    assert r1 == len(want1) and dst[:r1].tobytes() == want1
    out = np.zeros(src1.size, np.uint8)
    assert L.blosc2_decompress_ctx(dctx, dst.ctypes.data, 2**31 - 1, out.ctypes.data, out.size) == src1.size
    assert out.tobytes() == src1.tobytes()
    for c in (cctx, cctx1, dctx):
        L.blosc2_free_ctx(c)


def test_trunc_prec_in_front(eng):
    raw = synth.natural_channel(np.float32, 512, 512).view(np.uint8).ravel()
    for m in (10, -13):
        want, t = T.expected_chunk(raw, 4, m, compcode=O.BLOSCLZ, blocksize=262144)
        (c,) = eng.compress_host(params(4, 262144, trunc_prec=m), raw, [raw.size], [raw.size + 32])
        assert c == want, m
        outs, st = eng.decompress_host([c])
        assert st[0] == 0 and outs[0].tobytes() == t.tobytes(), m


def test_window_write_into_an_oracle_chunk(eng):
    ts, W = 2, 1024
    raw = chunk_case("f16_natural_b262144")[0]
    po = O.cparams(ts, blocksize=262144, compcode=O.BLOSCLZ)
    chunks = [chunk_case("f16_natural_b262144")[5]]
    ds = [raw.size + 32]
    specs, src = source([dict(chunk_first=0, chunk_count=1, origin=100 * W + 37, row_pitch=W, width=300, height=150),
                         dict(chunk_first=0, chunk_count=1, origin=raw.size // ts - 10, row_pitch=1, width=10, height=1)], ts)
    want, edited = expected(po, chunks, specs, ts, src, ds)
    new, st = eng.update_windows_host(params(ts, 262144), chunks, ds, specs, src)
    assert not st.any() and new == want
    outs, st = eng.decompress_host(new)
    assert st[0] == 0 and outs[0].tobytes() == edited[0].tobytes()


def _launches(eng, fn):
    eng.enable_timing(True)
    eng.reset_timing()
    try:
        out = fn()
        counts = {k: eng.kernel_time(k)[1] for k in (hip.K_ENCODE, hip.K_ENCODE_WIDE, hip.K_ENCODE_WIDE_BLOSCLZ)}
    finally:
        eng.enable_timing(False)
    return out, counts


def test_launch_counts_by_kernel(eng):
    assert hip.KERNELS[hip.K_ENCODE_WIDE_BLOSCLZ] == "cimg_encode_wide_blosclz"
    assert hip.load().cimg_kernel_name(hip.K_ENCODE_WIDE_BLOSCLZ).decode() == "cimg_encode_wide_blosclz"
    raw, ts, blk, split, filt, want = chunk_case("f16_natural_b262144")
    # 32 KiB blocks: the normal path, the bytes it gives today
    (c,), k = _launches(eng, lambda: eng.compress_host(params(2, 32768), raw, [raw.size], [raw.size + 32]))
    assert k[hip.K_ENCODE_WIDE_BLOSCLZ] == 0 and k[hip.K_ENCODE_WIDE] == 0 and k[hip.K_ENCODE] >= 1
    assert c == O.compress(O.cparams(2, blocksize=32768, compcode=O.BLOSCLZ), raw)[1]
    # lz4, wide
    _, k = _launches(eng, lambda: eng.compress_host(hip.cparams(2, blocksize=262144), raw, [raw.size], [raw.size + 32]))
    assert k[hip.K_ENCODE_WIDE] == 1 and k[hip.K_ENCODE_WIDE_BLOSCLZ] == 0
    # BloscLZ, wide
    (c,), k = _launches(eng, lambda: eng.compress_host(params(2, 262144), raw, [raw.size], [raw.size + 32]))
    assert k[hip.K_ENCODE_WIDE_BLOSCLZ] == 1 and k[hip.K_ENCODE] == 0 and k[hip.K_ENCODE_WIDE] == 0
    assert c == want


def test_still_refused(eng):
    raw = np.zeros(2 * MiB, np.uint8)
    for p in (params(2, 262144, filt=O.BITSHUFFLE), params(1, 262145), params(2, 524288)):
        with pytest.raises(hip.CodecError) as ei:
            eng.compress_host(p, raw, [raw.size], [raw.size + 32])
        assert ei.value.code == -7


# ---- the Python module ----------------------------------------------------------------------------------------------------------

def _module():
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    assert os.path.exists(path), "product module missing: run __graft_entry__.build()"
    spec = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    return ci


def test_python_channel_and_image_with_256k_blocks():
    ci = _module()
    W, H = 1024, 600
    for dtype in (np.uint8, np.float16, np.float32):
        arr = synth.natural_channel(dtype, W, H)
        patch = synth.tiled_channel(dtype, 200, 100)
        ch = ci.Channel(arr, W, H, compression_codec=ci.Codec.blosclz, block_size=262144)
        assert ch.block_size() == 262144
        assert np.array_equal(ch.get_decompressed(), arr)
        assert np.array_equal(ch.get_region(300, 200, 400, 77), arr[200:277, 300:700])
        ch.set_region(50, 60, patch)
        edited = arr.copy()
        edited[60:160, 50:250] = patch
        assert np.array_equal(ch.get_region(0, 0, W, H), edited)
        img = ci.Image(dtype, [arr, arr[::-1].copy()], W, H, ["a", "b"], compression_codec=ci.Codec.blosclz, block_size=262144)
        assert np.array_equal(img.get_decompressed(), np.stack([arr, arr[::-1]]))
        assert np.array_equal(img.get_region(300, 200, 400, 77), np.stack([arr, arr[::-1]])[:, 200:277, 300:700])
        img.set_region(50, 60, [patch, patch])
        assert np.array_equal(img.get_decompressed(), np.stack([edited, _with(arr[::-1], patch)]))


def _with(arr, patch):
    out = arr.copy()
    out[60:160, 50:250] = patch
    return out


def test_python_device_channel_with_256k_blocks():
    """DeviceChannel on torch tensors, in a child process that imports torch first (tests/_device_cases.py says why)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_blosclz_wide_device_case.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
