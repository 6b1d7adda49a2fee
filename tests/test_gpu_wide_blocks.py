"""Blocks up to 256 KiB on the MI355X: cimg_encode_wide / cimg_decode_wide (csrc/wide_kernel.h) behind the engine's planner
routing (csrc/wide_plan.h), through every public layer -- batch C ABI, device-resident calls, the blosc2 shim, the Python module.

The bytes are pinned to liblz4 1.9.3 through tests/golden/lz4_u32_kat.npz (make_lz4_u32_golden.py); the CPU twin of this file
is tests/test_emu_wide_blocks.py.  Run on the GPU box:  python -m pytest tests/test_gpu_wide_blocks.py -m gpu -q
"""
import ctypes as C
import hashlib
import importlib.util
import os
import struct
import sysconfig

import numpy as np
import pytest

import _oracle as O
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
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "lz4_u32_kat.npz"))


@pytest.fixture(scope="module")
def stream_inputs(golden_dir, kat):
    """The vectors' inputs, rebuilt by the generator's own stream_inputs() and checked against the digests in the file."""
    spec = importlib.util.spec_from_file_location("make_lz4_u32_golden", os.path.join(golden_dir, "make_lz4_u32_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs = dict(gen.stream_inputs())
    for name, src in inputs.items():
        assert hashlib.sha256(src.tobytes()).hexdigest() == str(kat["in_sha256|" + name]), name
    return inputs


def _chunk_cases():
    cases = []
    for dt in (np.float16, np.uint8, np.float32):
        for kind, fn in (("tiled", synth.tiled_channel), ("natural", synth.natural_channel)):
            for blk in (131072, 262144):
                cases.append((f"{kind}_{np.dtype(dt).name}_b{blk}", fn(dt, 1024, 1024), blk))
    cases.append(("ragged_float16_b262144",
                  synth.natural_channel(np.float16, 1024, 1044).view(np.uint8).ravel()[:2 * MiB + 40000].view(np.float16), 262144))
    return cases


@pytest.mark.parametrize("codec", ["lz4", "lz4hc"])
def test_wide_chunks_match_liblz4_digests(eng, kat, codec):
    cc = hip.LZ4 if codec == "lz4" else hip.LZ4HC
    for name, arr, blk in _chunk_cases():
        raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
        (c,) = eng.compress_host(hip.cparams(arr.dtype.itemsize, blocksize=blk, compcode=cc), raw, [raw.size], [raw.size + 96])
        key = f"{name}|{codec}"
        assert len(c) == int(kat["chunk_size|" + key]), key
        assert hashlib.sha256(c).hexdigest() == str(kat["chunk_sha256|" + key]), key
        outs, st = eng.decompress_host([c])
        assert st[0] == 0 and outs[0].tobytes() == raw.tobytes(), key


def test_u32_stream_vectors_through_the_gpu_encoder(eng, kat, stream_inputs):
    """Each byU32 vector as the one stream of a 1-byte, unshuffled chunk: the chunk's stream bytes are liblz4's."""
    seen = 0
    for name in sorted({str(k).split("|")[0] for k in kat["cases"]}):
        src = np.ascontiguousarray(stream_inputs[name])
        n = src.size
        if n < 65547 or n > 262144 or (src == src[0]).all():      # (a constant stream is a run, not an LZ4 block)
            continue
        want_len = int(kat[f"len|{name}|a1"])
        (c,) = eng.compress_host(hip.cparams(1, clevel=9, blocksize=n, filters=(0,) * 6), src, [n], [n + 64])
        bstart = struct.unpack_from("<i", c, 32)[0]
        cs = struct.unpack_from("<i", c, bstart)[0]
        if 0 < want_len < n:                         # liblz4 compresses it below the stream size: the chunk holds that LZ4 block
            assert cs == want_len, name
            assert hashlib.sha256(c[bstart + 4:bstart + 4 + cs]).hexdigest() == str(kat[f"sha256|{name}|a1"]), name
            seen += 1
        outs, st = eng.decompress_host([c])
        assert st[0] == 0 and outs[0].tobytes() == src.tobytes(), name
    assert seen >= 10


@pytest.mark.parametrize("dt", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("blk", [65536, 131072, 196608, 262144])
@pytest.mark.parametrize("codec", [hip.LZ4, hip.LZ4HC])
def test_block_size_table_round_trips(eng, dt, blk, codec):
    it = np.dtype(dt).itemsize
    arr = synth.natural_channel(dt, 1024, 2 * MiB // 1024 // it)
    raw = arr.view(np.uint8).ravel()
    (c,) = eng.compress_host(hip.cparams(it, blocksize=blk, compcode=codec), raw, [raw.size], [raw.size + 32])
    assert len(c) > 0
    outs, st = eng.decompress_host([c])
    assert st[0] == 0 and outs[0].tobytes() == raw.tobytes()
    r, ref = O.compress(O.cparams(it, blocksize=blk, compcode=codec), arr, destsize=raw.size + 32)
    if r > 0:                                        # where the oracle writes the chunk (byU16 streams) the bytes agree
        assert c == ref
    r, back = O.decompress(c)
    assert r == raw.size and back.tobytes() == raw.tobytes()


@pytest.mark.parametrize("dt", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("blk", [65536, 131072, 196608, 262144])
def test_block_size_table_blosclz_decode(eng, dt, blk):
    it = np.dtype(dt).itemsize
    arr = synth.natural_channel(dt, 1024, 2 * MiB // 1024 // it)
    raw = arr.view(np.uint8).ravel()
    r, c = O.compress(O.cparams(it, blocksize=blk, compcode=O.BLOSCLZ), arr, destsize=raw.size + 32)
    assert r > 0
    outs, st = eng.decompress_host([c])
    assert st[0] == 0 and outs[0].tobytes() == raw.tobytes()


def test_mixed_batch_of_normal_and_wide_blocks(eng):
    a = synth.tiled_channel(np.float16, 2048, 1024)                # 4 MiB
    b = synth.natural_channel(np.float16, 2048, 1024)
    ra, rb = a.view(np.uint8).ravel(), b.view(np.uint8).ravel()
    (ca,) = eng.compress_host(hip.cparams(2, blocksize=32768), ra, [ra.size], [ra.size + 32])
    (cb,) = eng.compress_host(hip.cparams(2, blocksize=262144), rb, [rb.size], [rb.size + 32])
    r, c32 = O.compress(O.cparams(2, blocksize=32768), a, destsize=ra.size + 32)
    assert ca == c32                                               # 32 KiB blocks: the normal path, bytes unchanged
    r, cblz = O.compress(O.cparams(2, blocksize=262144, compcode=O.BLOSCLZ, splitmode=O.NEVER_SPLIT), b, destsize=rb.size + 32)
    assert r > 0
    outs, st = eng.decompress_host([ca, cb, cblz, ca, cb])
    assert list(st) == [0] * 5
    for o, want in zip(outs, (ra, rb, rb, ra, rb)):
        assert o.tobytes() == want.tobytes()


def test_device_resident_1gib_with_256k_blocks(eng):
    chunk = 4 * MiB
    tile = np.concatenate([synth.natural_channel(np.float16, 2048, 1024, c=c).view(np.uint8).ravel() for c in range(4)])
    host = np.tile(tile, 1024 * MiB // tile.size)
    n = host.size // chunk
    nbytes = [chunk] * n
    raw_off = np.arange(n, dtype=np.int64) * chunk
    dest = chunk + 32
    comp_off = np.arange(n, dtype=np.int64) * dest
    d_raw, d_comp, d_out = eng.alloc(host.size), eng.alloc(n * dest), eng.alloc(host.size)
    try:
        d_raw.upload(host)
        cb = eng.compress_device(hip.cparams(2, blocksize=262144), d_raw.ptr, raw_off, nbytes, d_comp.ptr, comp_off, [dest] * n)
        assert (cb > 0).all()
        st = eng.decompress_device(d_comp.ptr, comp_off, nbytes, [262144] * n, d_out.ptr, raw_off, comp_size=cb)
        assert (st == 0).all()
        assert np.array_equal(d_out.download(), host)
        # the first chunk against the host path and the oracle's reader
        first = d_comp.download(int(cb[0]))
        (ch,) = eng.compress_host(hip.cparams(2, blocksize=262144), host[:chunk], [chunk], [dest])
        assert first.tobytes() == ch
        r, back = O.decompress(first)
        assert r == chunk and back.tobytes() == host[:chunk].tobytes()
    finally:
        for d in (d_raw, d_comp, d_out):
            d.free()


def test_blosc2_ctx_calls_with_256k_blocks(eng):
    L = hip.load()
    cp = hip.Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = 1, 9, 2, 4, 262144, 3
    cp.filters[5] = 1
    cctx = L.blosc2_create_cctx(cp)
    dp = hip.Blosc2DParams()
    dp.nthreads = 1
    dctx = L.blosc2_create_dctx(dp)
    a = synth.natural_channel(np.float16, 2048, 600)
    src = a.view(np.uint8).ravel()
    dst = np.zeros(src.size + 32, np.uint8)
    r = L.blosc2_compress_ctx(cctx, src.ctypes.data, src.size, dst.ctypes.data, dst.size)
    assert r > 0
    assert O.cbuffer_sizes(dst[:32])[2] == 262144
    out = np.zeros(src.size, np.uint8)
    assert L.blosc2_decompress_ctx(dctx, dst.ctypes.data, 2**31 - 1, out.ctypes.data, out.size) == src.size
    assert out.tobytes() == src.tobytes()
    L.blosc2_free_ctx(cctx)
    L.blosc2_free_ctx(dctx)


def test_python_image_with_256k_blocks():
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    assert os.path.exists(path), "product module missing: run __graft_entry__.build()"
    spec = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    for dtype in (np.float32, np.float16, np.uint8):
        arr = synth.natural_channel(dtype, 1920, 1080)
        img = ci.Image(dtype, [arr, arr[::-1].copy()], 1920, 1080, ["a", "b"], block_size=262144)
        assert np.array_equal(img.get_decompressed(), np.stack([arr, arr[::-1]]))


def test_truncated_wide_chunk_is_reported_not_crashed(eng):
    a = synth.natural_channel(np.uint8, 1024, 1024)
    raw = a.ravel()
    (good,) = eng.compress_host(hip.cparams(1, blocksize=262144), raw, [raw.size], [raw.size + 32])
    assert not good[2] & 0x02                                       # a regular chunk, not memcpyed
    bad = bytearray(good)
    struct.pack_into("<i", bad, 32, len(good) + 1000)               # bstart outside the chunk
    outs, status = eng.decompress_host([bytes(bad), good], check=False)
    assert status[0] < 0 and status[1] == 0
    assert outs[1].tobytes() == raw.tobytes()
    bad = bytearray(good)
    first = struct.unpack_from("<i", good, 32)[0]
    for k in range(first + 4 + 1000, first + 4 + 1064):
        bad[k] = 0xFF                                               # long literal / match runs inside the first LZ4 stream
    outs, status = eng.decompress_host([bytes(bad)], check=False)
    assert status[0] < 0 or outs[0].tobytes() != raw.tobytes()
    # the caller's buffer holds half of what the header claims: the kernel reads nothing behind the header and says so
    d_comp, d_out = eng.alloc(len(good) + 64), eng.alloc(raw.size)
    try:
        d_comp.upload(np.frombuffer(good, np.uint8))
        st = eng.decompress_device(d_comp.ptr, [0], [raw.size], [262144], d_out.ptr, [0], check=False, comp_size=[len(good) // 2])
        assert st[0] == -5
    finally:
        d_comp.free()
        d_out.free()


def test_blocks_above_256k_are_refused_before_launch(eng):
    raw = np.zeros(2 * MiB, np.uint8)
    for blk in (262145, 524288):
        with pytest.raises(hip.CodecError) as ei:
            eng.compress_host(hip.cparams(1, blocksize=blk), raw, [raw.size], [raw.size + 32])
        assert ei.value.code == -7
