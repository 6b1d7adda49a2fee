"""zstd blocks up to 256 KiB on the MI355X: cimg_encode_wide_zstd (streams of 64 .. 256 KiB as frames of more than one zstd block)
and the wide zstd read path (cimg_decode_wide leaves zstd blocks pending; cimg_zstd_walk + cimg_zstd_replay_wide), through every
public layer -- batch C ABI, device-resident calls, the blosc2 shim, the Python module.

The CPU twin of this file is tests/test_emu_zstd_wide_blocks.py; chunks libzstd wrote come from tests/golden/zstd_wide_kat.npz
(make_zstd_wide_golden.py).  Run on the GPU box:  python -m pytest tests/test_gpu_zstd_wide_blocks.py -m gpu -q
"""
import hashlib
import importlib.util
import os
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
def wkat(golden_dir):
    return np.load(os.path.join(golden_dir, "zstd_wide_kat.npz"))


@pytest.fixture(scope="module")
def golden_inputs(golden_dir, wkat):
    spec = importlib.util.spec_from_file_location("make_zstd_wide_golden", os.path.join(golden_dir, "make_zstd_wide_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs = gen.inputs()
    for name in wkat["chunks"]:
        assert hashlib.sha256(inputs[str(name)][0].tobytes()).hexdigest() == str(wkat["in_sha256|" + str(name)]), name
    return inputs


def zp(ts, blocksize, clevel=9, filters=(0, 0, 0, 0, 0, hip.SHUFFLE)):
    return hip.cparams(ts, clevel=clevel, blocksize=blocksize, compcode=hip.ZSTD, filters=filters)


def test_libzstd_chunks_decode(eng, wkat, golden_inputs):
    names = [str(n) for n in wkat["chunks"]]
    chunks = [wkat["chunk|" + n].tobytes() for n in names]
    outs, st = eng.decompress_host(chunks)
    assert list(st) == [0] * len(names)
    for o, n in zip(outs, names):
        assert o.tobytes() == golden_inputs[n][0].tobytes(), n


@pytest.mark.parametrize("dt", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("blk", [131072, 196608, 262144])
@pytest.mark.parametrize("clevel", [5, 9])
def test_block_size_table_round_trips(eng, dt, blk, clevel):
    it = np.dtype(dt).itemsize
    arr = synth.natural_channel(dt, 1024, 2 * MiB // 1024 // it)
    raw = arr.view(np.uint8).ravel()
    chunks = eng.compress_host(zp(it, blk, clevel), raw, [MiB, MiB], [MiB + 32, MiB + 32])
    assert all(len(c) < MiB for c in chunks)
    outs, st = eng.decompress_host(chunks)
    assert list(st) == [0, 0]
    assert np.concatenate(outs).tobytes() == raw.tobytes()


@pytest.mark.parametrize("clevel", [5, 9])
def test_streams_that_are_one_match_per_zstd_block_round_trip(eng, clevel):
    # rows that repeat: the second 128 KiB zstd block of every 256 KiB stream is a single match of 131 072 bytes
    x = np.arange(1024)
    cases = [(np.tile((x * 255 // 1023).astype(np.uint8), (1024, 1)), hip.SHUFFLE),
             (np.tile((x * 37 % 65536).astype(np.uint16), (512, 1)), hip.NOFILTER),
             (np.tile((x % 256).astype(np.uint16), (512, 1)), hip.SHUFFLE)]
    for img, filt in cases:
        raw = np.ascontiguousarray(img).view(np.uint8).ravel()
        (c,) = eng.compress_host(zp(img.dtype.itemsize, 262144, clevel, filters=(0, 0, 0, 0, 0, filt)), raw, [raw.size], [raw.size + 32])
        assert len(c) < raw.size // 8
        outs, st = eng.decompress_host([c])
        assert list(st) == [0]
        assert outs[0].tobytes() == raw.tobytes()


def test_mixed_batch_of_32k_zstd_256k_zstd_and_256k_lz4(eng):
    a = synth.tiled_channel(np.float16, 2048, 512)
    b = synth.natural_channel(np.float16, 2048, 512)
    ra, rb = a.view(np.uint8).ravel(), b.view(np.uint8).ravel()
    (c32,) = eng.compress_host(zp(2, 32768), ra, [ra.size], [ra.size + 32])
    (cz,) = eng.compress_host(zp(2, 262144), rb, [rb.size], [rb.size + 32])
    (cl,) = eng.compress_host(hip.cparams(2, blocksize=262144), rb, [rb.size], [rb.size + 32])
    outs, st = eng.decompress_host([c32, cz, cl, cz, c32])
    assert list(st) == [0] * 5
    for o, want in zip(outs, (ra, rb, rb, rb, ra)):
        assert o.tobytes() == want.tobytes()


def test_device_resident_1gib_with_256k_zstd_blocks(eng):
    chunk = 4 * MiB
    tile = np.concatenate([synth.natural_channel(np.float32, 1024, 1024, c=c).view(np.uint8).ravel() for c in range(4)])
    host = np.tile(tile, 1024 * MiB // tile.size)
    n = host.size // chunk
    nbytes = [chunk] * n
    raw_off = np.arange(n, dtype=np.int64) * chunk
    dest = chunk + 32
    comp_off = np.arange(n, dtype=np.int64) * dest
    d_raw, d_comp, d_out = eng.alloc(host.size), eng.alloc(n * dest), eng.alloc(host.size)
    try:
        d_raw.upload(host)
        cb = eng.compress_device(zp(4, 262144), d_raw.ptr, raw_off, nbytes, d_comp.ptr, comp_off, [dest] * n)
        assert (cb > 0).all() and int(cb.sum()) < host.size
        st = eng.decompress_device(d_comp.ptr, comp_off, nbytes, [262144] * n, d_out.ptr, raw_off, comp_size=cb)
        assert (st == 0).all()
        assert np.array_equal(d_out.download(), host)
        # the first chunk as the host path writes it
        first = d_comp.download(int(cb[0]))
        (ch,) = eng.compress_host(zp(4, 262144), host[:chunk], [chunk], [dest])
        assert first.tobytes() == ch
    finally:
        for d in (d_raw, d_comp, d_out):
            d.free()


def test_blosc2_ctx_calls_with_256k_zstd_blocks(eng):
    L = hip.load()
    cp = hip.Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = hip.ZSTD, 9, 2, 4, 262144, 3
    cp.filters[5] = 1
    cctx = L.blosc2_create_cctx(cp)
    dp = hip.Blosc2DParams()
    dp.nthreads = 1
    dctx = L.blosc2_create_dctx(dp)
    a = synth.natural_channel(np.float16, 2048, 600)
    src = a.view(np.uint8).ravel()
    dst = np.zeros(src.size + 32, np.uint8)
    r = L.blosc2_compress_ctx(cctx, src.ctypes.data, src.size, dst.ctypes.data, dst.size)
    assert 0 < r < src.size
    assert O.cbuffer_sizes(dst[:32])[2] == 262144 and dst[2] >> 5 == 4       # 256 KiB blocks, codec format 4
    out = np.zeros(src.size, np.uint8)
    assert L.blosc2_decompress_ctx(dctx, dst.ctypes.data, 2**31 - 1, out.ctypes.data, out.size) == src.size
    assert out.tobytes() == src.tobytes()
    L.blosc2_free_ctx(cctx)
    L.blosc2_free_ctx(dctx)


def test_python_image_with_256k_zstd_blocks():
    path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + sysconfig.get_config_var("EXT_SUFFIX"))
    assert os.path.exists(path), "product module missing: run __graft_entry__.build()"
    spec = importlib.util.spec_from_file_location("compressed_image", path)
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    for dtype in (np.float32, np.float16, np.uint8):
        arr = synth.natural_channel(dtype, 1920, 1080)
        img = ci.Image(dtype, [arr, arr[::-1].copy()], 1920, 1080, ["a", "b"], compression_codec=ci.Codec.zstd, block_size=262144)
        assert np.array_equal(img.get_decompressed(), np.stack([arr, arr[::-1]]))


def test_corrupt_frame_and_truncated_chunk_are_reported(eng):
    raw = synth.natural_channel(np.uint8, 1024, 1024).ravel()
    (good,) = eng.compress_host(zp(1, 262144), raw, [raw.size], [raw.size + 32])
    bstart = int(np.frombuffer(good[32:36], np.int32)[0])
    cs = int(np.frombuffer(good[bstart:bstart + 4], np.int32)[0])
    assert 0 < cs < 262144 and good[bstart + 4:bstart + 8] == b"\x28\xb5\x2f\xfd"
    bad = bytearray(good)
    for k in range(bstart + 4 + cs - 40, bstart + 4 + cs):
        bad[k] = 0xFF
    outs, st = eng.decompress_host([bytes(bad), good], check=False)
    assert st[0] < 0 and st[1] == 0
    assert outs[1].tobytes() == raw.tobytes()
    d_comp, d_out = eng.alloc(len(good) + 64), eng.alloc(raw.size)
    try:
        d_comp.upload(np.frombuffer(good, np.uint8))
        st = eng.decompress_device(d_comp.ptr, [0], [raw.size], [262144], d_out.ptr, [0], check=False, comp_size=[len(good) // 2])
        assert st[0] < 0
    finally:
        d_comp.free()
        d_out.free()


def test_blocks_above_256k_stay_refused(eng):
    raw = np.zeros(2 * MiB, np.uint8)
    for blk in (262145, 524288):
        with pytest.raises(hip.CodecError) as ei:
            eng.compress_host(zp(1, blk), raw, [raw.size], [raw.size + 32])
        assert ei.value.code == -7
