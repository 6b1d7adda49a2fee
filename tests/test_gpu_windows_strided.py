"""Strided windows on the MI355X: cimg_decompress_windows_strided_device / _host (csrc/window_kernel.h: cimg_decode_window_strided,
csrc/window_plan.h).

The matrix of tests/test_emu_windows_strided.py through the real engine, device call and host call: canary-filled outputs with
gaps between the rows, expected pixels by numpy indexing into the decoded plane (the oracle's decode for oracle-written chunks,
the source pixels for engine-written ones), and stats that equal a brute-force count of the blocks that hold a byte of a sampled
element.  Every hostile input here is one the host refuses before anything is launched.
"""
import numpy as np
import pytest

import _oracle as O
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, pack, sizes, standard_windows
from _windows_strided import expected, sampled_blocks, strided_windows
from cimg import hip, synth

pytestmark = pytest.mark.gpu
BLOSCLZ, LZ4, LZ4HC, ZSTD = 0, 1, 2, 5
I64, I32 = 2 ** 63 - 1, 2 ** 31 - 1


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def pixels(ts, elems, seed=0):
    rng = np.random.default_rng(seed)
    raw = synth.tiled_channel(np.float16, 64, max(elems * ts // 128 + 1, 1)).view(np.uint8).ravel()[:elems * ts].copy()
    raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)
    return raw


def engine_chunks(eng, ts, raw, chunk_bytes, **kw):
    p = hip.cparams(ts, **kw)
    nb = [min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)]
    chunks = eng.compress_host(p, raw, nb, [n + 64 for n in nb])
    assert all(len(c) > 0 for c in chunks)
    return chunks


def geometry(ts):
    chunk_elems = 13000
    elems = 2 * chunk_elems + 5001
    raw = pixels(ts, elems)
    if ts > 1:
        raw = np.concatenate([raw, np.arange(ts - 1, dtype=np.uint8)])
    return raw, chunk_elems * ts, elems, chunk_elems


def run_device(eng, chunks, specs, ts, size, nb=None, bs=None, strided=True):
    buf, off, cs = concat(chunks)
    if nb is None:
        nb, bs = sizes(chunks)
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    rc, st = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False, strided=strided)
    stats = eng.window_stats()
    out = d_out.download()
    d_comp.free(); d_out.free()
    return rc, st, out, stats


def run_host(eng, chunks, specs, size, strided=True):
    out = np.full(size, CANARY, np.uint8)
    rc, st = eng.decompress_windows_host(chunks, specs, out, check=False, strided=strided)
    return rc, st, out, eng.window_stats()


def plane(chunks):
    return np.concatenate([O.decompress(c)[1] for c in chunks])


def both(eng, chunks, specs, ts, size, nb=None, bs=None):
    yield "device", run_device(eng, chunks, specs, ts, size, nb, bs)
    yield "host", run_host(eng, chunks, specs, size)


def check(eng, chunks, ts, elems, chunk_elems, want_plane=None, whole=False):
    nb, bs = sizes(chunks)
    specs, size = pack(strided_windows(elems, chunk_elems, len(chunks), int(bs[0]) // ts), ts)
    want = expected([plane(chunks) if want_plane is None else want_plane] * len(specs), specs, ts, size)
    count, touched = sampled_blocks(specs, nb, bs, ts)
    for runner, (rc, st, out, stats) in both(eng, chunks, specs, ts, size):
        assert rc == 0 and not st.any(), (runner, rc, st, eng.last_error())
        assert np.array_equal(out, want), runner
        if whole:
            assert stats["blocks_decoded"] == 0 and stats["chunks_whole"] == len(touched), (runner, stats)
        else:
            assert stats["blocks_decoded"] == count and stats["chunks_whole"] == 0, (runner, stats, count)
        if runner == "host":
            assert stats["comp_bytes_uploaded"] == sum(len(chunks[i]) for i in touched)


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_oracle_chunks(eng, codec, ts, filt):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=8192, compcode=codec, filters=(0, 0, 0, 0, 0, filt)), raw, cbytes)
    check(eng, chunks, ts, elems, chunk_elems)


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ, ZSTD])
@pytest.mark.parametrize("ts,filt,split", [(4, 1, 3), (4, 1, 1), (4, 1, 2), (2, 2, 3), (3, 1, 3), (8, 0, 3), (1, 1, 3)])
def test_engine_chunks(eng, codec, ts, filt, split):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = engine_chunks(eng, ts, raw, cbytes, clevel=5, blocksize=8192, compcode=codec, splitmode=split,
                           filters=(0, 0, 0, 0, 0, filt))
    check(eng, chunks, ts, elems, chunk_elems, want_plane=raw, whole=codec == ZSTD)


def test_memcpyed_and_zero_chunks(eng):
    raw, cbytes, elems, chunk_elems = geometry(4)
    check(eng, oracle_chunks(O.cparams(4, clevel=0, blocksize=8192), raw, cbytes), 4, elems, chunk_elems)
    zeros = np.zeros(raw.size // 4 * 4, np.uint8)
    check(eng, engine_chunks(eng, 4, zeros, cbytes, blocksize=8192), 4, zeros.size // 4, chunk_elems, want_plane=zeros)


@pytest.mark.parametrize("codec", [LZ4, ZSTD])
def test_256k_blocks(eng, codec):
    ts = 4
    raw = pixels(ts, 3 * 65536 + 1000)
    chunks = engine_chunks(eng, ts, raw, 262144, clevel=5, blocksize=262144, compcode=codec)
    specs, size = pack([dict(chunk_first=0, chunk_count=len(chunks), origin=70000, row_pitch=1000, col_pitch=3, width=300, height=40),
                        dict(chunk_first=0, chunk_count=len(chunks), origin=5, row_pitch=1, col_pitch=65536, width=3, height=1)], ts)
    want = expected([raw, raw], specs, ts, size)
    for runner, (rc, st, out, stats) in both(eng, chunks, specs, ts, size):
        assert rc == 0 and not st.any() and np.array_equal(out, want), runner
        assert stats["chunks_whole"] == 3 and stats["blocks_decoded"] == 0


@pytest.mark.parametrize("ts", [1, 3, 4])
def test_col_pitch_1_equals_the_unstrided_call(eng, ts):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=8192), raw, cbytes)
    old, size = pack(standard_windows(elems, 180, chunk_elems, len(chunks)), ts)
    new = [dict(s, col_pitch=1) for s in old]
    a = run_device(eng, chunks, old, ts, size, strided=False), run_host(eng, chunks, old, size, strided=False)
    b = run_device(eng, chunks, new, ts, size), run_host(eng, chunks, new, size)
    for (rc0, st0, out0, stats0), (rc1, st1, out1, stats1) in zip(a, b):
        assert rc0 == 0 and rc1 == 0 and np.array_equal(st0, st1) and np.array_equal(out0, out1)
        assert stats0 == stats1


def test_selectivity_worked_case(eng):
    """8 float16 chunks of 4 MiB (1024 blocks of 32 KiB, 16 777 216 elements); one row, col_pitch 49152, width 342: exactly 342
    blocks are decoded."""
    ts, chunk = 2, 4 << 20
    raw = np.tile(pixels(ts, chunk // ts // 8), 64)
    chunks = engine_chunks(eng, ts, raw, chunk)
    nb, bs = sizes(chunks)
    assert (bs == 32768).all() and nb.sum() // ts == 16777216
    specs, size = pack([dict(chunk_first=0, chunk_count=8, origin=0, row_pitch=1, col_pitch=49152, width=342, height=1)], ts)
    count, touched = sampled_blocks(specs, nb, bs, ts)
    assert count == 342
    want = expected([raw], specs, ts, size)
    for runner, (rc, st, out, stats) in both(eng, chunks, specs, ts, size):
        assert rc == 0 and not st.any() and np.array_equal(out, want), runner
        assert stats["blocks_decoded"] == 342 and stats["chunks_whole"] == 0
        if runner == "host":
            assert stats["comp_bytes_uploaded"] == sum(len(chunks[i]) for i in touched)


def test_far_apart_samples_skip_whole_chunks(eng):
    raw, cbytes, elems, chunk_elems = geometry(4)
    chunks = oracle_chunks(O.cparams(4, blocksize=8192), raw, cbytes)
    nb, bs = sizes(chunks)
    # chunk 1 is garbage behind its header: the samples lie in chunks 0 and 2, so nothing of it is read, reported or uploaded
    bad = [c[:32] + bytes([0xFF]) * (len(c) - 32) if i == 1 else c for i, c in enumerate(chunks)]
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=100, row_pitch=1, col_pitch=2 * chunk_elems + 50, width=2, height=1)], 4)
    want = expected([plane(chunks)], specs, 4, size)
    for runner, (rc, st, out, stats) in both(eng, bad, specs, 4, size, nb, bs):
        assert rc == 0 and not st.any() and np.array_equal(out, want), runner
        assert stats["blocks_decoded"] == 2 and stats["chunks_whole"] == 0
        if runner == "host":
            assert stats["comp_bytes_uploaded"] == len(chunks[0]) + len(chunks[2])


def test_refusals_and_damaged_chunk(eng):
    ts = 2
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, blocksize=8192), raw, cbytes)
    pl = plane(chunks)
    ok = dict(chunk_first=0, chunk_count=3, origin=10, row_pitch=100, col_pitch=4, width=20, height=5, out_off=0, out_pitch=20 * ts)
    good, gsize = pack([ok], ts)
    for b in (dict(ok, col_pitch=0), dict(ok, col_pitch=-1), dict(ok, row_pitch=19 * 4), dict(ok, origin=elems - 19 * 4, height=1),
              dict(ok, origin=elems - 400 - 19 * 4), dict(ok, col_pitch=I64), dict(ok, col_pitch=I64 // 19 + 1),
              dict(ok, col_pitch=I64, width=I32, height=I32, out_pitch=I64), dict(ok, col_pitch=I32, width=I32, height=1, out_pitch=I64),
              dict(ok, row_pitch=I64 // 4 + 1), dict(ok, chunk_first=1), dict(ok, chunk_count=0), dict(ok, chunk_count=I32)):
        for runner, (rc, st, out, stats) in both(eng, chunks, [b], ts, 1 << 15):
            assert rc == ERR_INVALID_PARAM and (out == CANARY).all(), (runner, b)
            assert stats["blocks_decoded"] == 0 and stats["chunks_whole"] == 0
        for runner, (rc, st, out, stats) in both(eng, chunks, good, ts, gsize):                # the engine stays usable
            assert rc == 0 and np.array_equal(out, expected([pl], good, ts, gsize)), (runner, b)
    # a damaged block that holds a sample fails its chunk, and the other chunks' samples are still written; the same damage in a
    # block no sample lies in goes unnoticed
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")      # block 2 of chunk 1: elements chunk_elems + [8192, 12288)
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")
    bad = [chunks[0], bytes(c), chunks[2]]
    inside, size = pack([dict(chunk_first=0, chunk_count=3, origin=0, row_pitch=1, col_pitch=1000, width=31, height=1)], ts)
    want = expected([pl], inside, ts, size)
    o = inside[0]["out_off"]
    for runner, (rc, st, out, stats) in both(eng, bad, inside, ts, size):
        assert rc < 0 and st[1] == rc and st[0] == 0 and st[2] == 0, runner
        for k in range(31):
            if not chunk_elems <= k * 1000 < 2 * chunk_elems:
                assert np.array_equal(out[o + ts * k:o + ts * k + ts], want[o + ts * k:o + ts * k + ts]), (runner, k)
        assert (out[:o] == CANARY).all() and (out[o + 31 * ts:] == CANARY).all()
    outside, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 100, row_pitch=50, col_pitch=3, width=7, height=40)], ts)
    want = expected([pl], outside, ts, size)
    for runner, (rc, st, out, stats) in both(eng, bad, outside, ts, size):
        assert rc == 0 and not st.any() and np.array_equal(out, want), runner


def test_1gib_device_plane_subsampled(eng):
    """The plane of test_gpu_windows.py::test_1gib_device_plane (16384 x 16384 float32, 4 MiB chunks) read 16 x 16 subsampled:
    1024 sampled rows, two 32 KiB blocks each."""
    n, chunk, step = 16384, 4 << 20, 16
    img = synth.tiled_channel(np.float32, n, n)
    raw = np.ascontiguousarray(img).view(np.uint8).ravel()
    assert raw.size == 1 << 30
    nch = raw.size // chunk
    d_raw = eng.alloc(raw.size)
    d_raw.upload(raw)
    dest = chunk + 64
    d_comp = eng.alloc(nch * dest)
    cb = eng.compress_device(hip.cparams(4), d_raw.ptr, np.arange(nch) * chunk, [chunk] * nch, d_comp.ptr, np.arange(nch) * dest, [dest] * nch)
    assert (cb > 0).all()
    d_raw.free()
    w = n // step
    out_pitch = w * 4 + 64
    size = out_pitch * w
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    spec = dict(chunk_first=0, chunk_count=nch, origin=0, row_pitch=step * n, col_pitch=step, width=w, height=w, out_off=0, out_pitch=out_pitch)
    eng.decompress_windows_device(d_comp.ptr, np.arange(nch) * dest, [chunk] * nch, [32768] * nch, 4, [spec], d_out.ptr, comp_size=cb,
                                  strided=True)
    out = d_out.download().reshape(w, out_pitch)
    d_comp.free(); d_out.free()
    assert np.array_equal(out[:, :w * 4].view(np.float32), img[::step, ::step])
    assert (out[:, w * 4:] == CANARY).all()
    s = eng.window_stats()
    assert s["blocks_decoded"] == 2048 and s["chunks_whole"] == 0
