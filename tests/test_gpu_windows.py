"""Windows on the MI355X: cimg_decompress_windows_device / _host (csrc/window_kernel.h, csrc/window_plan.h) and blosc2_getitem_ctx.

Every call writes into a canary-filled output with gaps between the rows; the result must equal numpy slices of the decoded plane
(the oracle's decode for oracle-written chunks, the source pixels for engine-written ones) and the canary must survive elsewhere.
"""

import numpy as np
import pytest

import _oracle as O
from _windows import (CANARY, ERR_INVALID_PARAM, ERR_NULL_POINTER, ERR_READ_BUFFER, ERR_WRITE_BUFFER, concat, expected,
                      oracle_chunks, pack, sizes, standard_windows)
from cimg import hip, synth

pytestmark = pytest.mark.gpu
BLOSCLZ, LZ4, LZ4HC, ZSTD = 0, 1, 2, 5


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


def run_device(eng, chunks, specs, ts, size, nb=None, bs=None):
    buf, off, cs = concat(chunks)
    if nb is None:
        nb, bs = sizes(chunks)
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    rc, st = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False)
    out = d_out.download()
    d_comp.free(); d_out.free()
    return rc, st, out


def run_host(eng, chunks, specs, size):
    out = np.full(size, CANARY, np.uint8)
    rc, st = eng.decompress_windows_host(chunks, specs, out, check=False)
    return rc, st, out


def plane(chunks):
    return np.concatenate([O.decompress(c)[1] for c in chunks])


def check(eng, chunks, ts, elems, chunk_elems, want_plane=None):
    specs, size = pack(standard_windows(elems, 180, chunk_elems, len(chunks)), ts)
    want = expected([plane(chunks) if want_plane is None else want_plane] * len(specs), specs, ts, size)
    for runner in ("device", "host"):
        rc, st, out = run_device(eng, chunks, specs, ts, size) if runner == "device" else run_host(eng, chunks, specs, size)
        assert rc == 0 and not st.any(), (runner, rc, st, eng.last_error())
        assert np.array_equal(out, want), runner
    return eng.window_stats()


@pytest.mark.parametrize("codec", [LZ4, LZ4HC, BLOSCLZ])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_oracle_chunks(eng, codec, ts, filt):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=8192, compcode=codec, filters=(0, 0, 0, 0, 0, filt)), raw, cbytes)
    check(eng, chunks, ts, elems, chunk_elems)


@pytest.mark.parametrize("codec", [LZ4, LZ4HC, BLOSCLZ, ZSTD])
@pytest.mark.parametrize("ts,filt,split", [(4, 1, 3), (4, 1, 1), (4, 1, 2), (2, 2, 3), (3, 1, 3), (8, 0, 3), (1, 1, 3)])
def test_engine_chunks(eng, codec, ts, filt, split):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = engine_chunks(eng, ts, raw, cbytes, clevel=5, blocksize=8192, compcode=codec, splitmode=split,
                           filters=(0, 0, 0, 0, 0, filt))
    stats = check(eng, chunks, ts, elems, chunk_elems, want_plane=raw)
    assert stats["chunks_whole"] == (len(chunks) if codec == ZSTD else 0)


def test_memcpyed_chunks(eng):
    raw, cbytes, elems, chunk_elems = geometry(4)
    check(eng, oracle_chunks(O.cparams(4, clevel=0, blocksize=8192), raw, cbytes), 4, elems, chunk_elems)


@pytest.mark.parametrize("codec", [LZ4, ZSTD])
def test_256k_blocks(eng, codec):
    ts = 4
    raw = pixels(ts, 3 * 65536 + 1000)
    chunks = engine_chunks(eng, ts, raw, 262144, clevel=5, blocksize=262144, compcode=codec)
    specs, size = pack([dict(chunk_first=0, chunk_count=len(chunks), origin=70000, row_pitch=1000, width=300, height=40),
                        dict(chunk_first=0, chunk_count=len(chunks), origin=5, row_pitch=1, width=1, height=1)], ts)
    want = expected([raw, raw], specs, ts, size)
    for rc, st, out in (run_device(eng, chunks, specs, ts, size), run_host(eng, chunks, specs, size)):
        assert rc == 0 and not st.any() and np.array_equal(out, want)
        assert eng.window_stats()["chunks_whole"] == 2


def test_four_channels_in_one_call(eng):
    ts, W, H = 2, 512, 300
    chunks, specs, planes = [], [], []
    for c in range(4):
        raw = pixels(ts, W * H, seed=c)
        ch = engine_chunks(eng, ts, raw, 65536)
        specs.append(dict(chunk_first=len(chunks), chunk_count=len(ch), origin=100 * W + 37, row_pitch=W, width=128, height=90))
        chunks += ch
        planes.append(raw)
    specs, size = pack(specs, ts)
    want = expected(planes, specs, ts, size)
    for rc, st, out in (run_device(eng, chunks, specs, ts, size), run_host(eng, chunks, specs, size)):
        assert rc == 0 and not st.any() and np.array_equal(out, want)


def test_selectivity_and_upload(eng):
    raw, cbytes, elems, chunk_elems = geometry(4)
    chunks = oracle_chunks(O.cparams(4, blocksize=8192), raw, cbytes)
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 4000, row_pitch=1, width=1, height=1)], 4)
    rc, st, out = run_host(eng, chunks, specs, size)
    assert rc == 0 and np.array_equal(out, expected([plane(chunks)], specs, 4, size))
    s = eng.window_stats()
    assert s["blocks_decoded"] == 1 and s["chunks_whole"] == 0 and s["comp_bytes_uploaded"] == len(chunks[1])
    # a window over rows of chunks 1 and 2
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 100, row_pitch=200, width=50, height=70)], 4)
    rc, st, out = run_host(eng, chunks, specs, size)
    assert rc == 0 and eng.window_stats()["comp_bytes_uploaded"] == len(chunks[1]) + len(chunks[2])
    # chunks no row meets are not read: garbage behind their headers changes nothing
    nb, bs = sizes(chunks)
    bad = [c if i == 1 else c[:32] + bytes([0xFF]) * (len(c) - 32) for i, c in enumerate(chunks)]
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 545, row_pitch=180, width=40, height=20)], 4)
    want = expected([plane(chunks)], specs, 4, size)
    for rc, st, out in (run_device(eng, bad, specs, 4, size, nb, bs), run_host(eng, bad, specs, size)):
        assert rc == 0 and not st.any() and np.array_equal(out, want)


def test_invalid_windows_and_corruption(eng):
    ts = 2
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, blocksize=8192), raw, cbytes)
    ok = dict(chunk_first=0, chunk_count=3, origin=10, row_pitch=100, width=20, height=5, out_off=0, out_pitch=20 * ts)
    for b in (dict(ok, origin=elems - 10), dict(ok, origin=-1), dict(ok, width=-1), dict(ok, height=-2), dict(ok, row_pitch=10),
              dict(ok, out_pitch=20 * ts - 1), dict(ok, chunk_first=1), dict(ok, chunk_count=0), dict(ok, height=elems)):
        for rc, st, out in (run_device(eng, chunks, [b], ts, 1 << 15), run_host(eng, chunks, [b], 1 << 15)):
            assert rc == ERR_INVALID_PARAM and (out == CANARY).all(), b
    specs, size = pack([ok], ts)
    rc, st, out = run_host(eng, chunks, specs, size)
    assert rc == 0 and np.array_equal(out, expected([plane(chunks)], specs, ts, size))
    # a damaged block inside the window fails its chunk; the same damage outside the window goes unnoticed
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")      # block 2 of chunk 1
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")
    bad = [chunks[0], bytes(c), chunks[2]]
    inside, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 9000, row_pitch=1, width=10, height=1)], ts)
    for rc, st, out in (run_device(eng, bad, inside, ts, size), run_host(eng, bad, inside, size)):
        assert rc < 0 and st[1] < 0 and st[0] == 0 and st[2] == 0
    outside, size = pack([dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 100, row_pitch=50, width=20, height=40)], ts)
    want = expected([plane(chunks)], outside, ts, size)
    for rc, st, out in (run_device(eng, bad, outside, ts, size), run_host(eng, bad, outside, size)):
        assert rc == 0 and not st.any() and np.array_equal(out, want)


def test_1gib_device_plane(eng):
    n, chunk = 16384, 4 << 20
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
    x0, y0, w = 5000, 7000, 1024
    out_pitch = w * 4 + 64
    size = out_pitch * w
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    spec = dict(chunk_first=0, chunk_count=nch, origin=y0 * n + x0, row_pitch=n, width=w, height=w, out_off=0, out_pitch=out_pitch)
    eng.decompress_windows_device(d_comp.ptr, np.arange(nch) * dest, [chunk] * nch, [32768] * nch, 4, [spec], d_out.ptr, comp_size=cb)
    out = d_out.download().reshape(w, out_pitch)
    assert np.array_equal(out[:, :w * 4].view(np.float32), img[y0:y0 + w, x0:x0 + w])
    assert (out[:, w * 4:] == CANARY).all()
    s = eng.window_stats()
    assert 1024 <= s["blocks_decoded"] <= 2048 and s["chunks_whole"] == 0


def test_getitem(eng):
    L = hip.load()
    dctx = L.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    try:
        for ts, codec in ((4, LZ4), (2, BLOSCLZ), (3, LZ4HC), (1, LZ4)):
            raw = pixels(ts, 40000 // ts)
            p = O.cparams(ts, blocksize=8192, compcode=codec)
            r, chunk = O.compress(p, raw, destsize=raw.size + 64)
            full = O.decompress(chunk)[1]
            src = np.frombuffer(chunk, np.uint8)
            nitems_all = raw.size // ts
            for start, nitems in ((0, 1), (nitems_all // 2, 1), (1234, 5000), (0, nitems_all), (nitems_all - 3, 3), (7, 0)):
                dest = np.full(nitems * ts + 16, CANARY, np.uint8)
                rc = L.blosc2_getitem_ctx(dctx, hip._ptr(src), len(chunk), start, nitems, hip._ptr(dest), nitems * ts + 16)
                assert rc == nitems * ts, (ts, codec, start, nitems, rc)
                assert np.array_equal(dest[:nitems * ts], full[start * ts:(start + nitems) * ts])
                assert (dest[nitems * ts:] == CANARY).all()
            dest = np.zeros(64, np.uint8)
            g = lambda s, k, ss=len(chunk), d=hip._ptr(dest), ds=64, c=dctx, sp=hip._ptr(src): L.blosc2_getitem_ctx(c, sp, ss, s, k, d, ds)
            assert g(-1, 1) == ERR_INVALID_PARAM
            assert g(nitems_all - 1, 2) == ERR_INVALID_PARAM
            assert g(0, 64 // ts + 1) == ERR_WRITE_BUFFER
            assert g(0, 1, ss=len(chunk) - 1) == ERR_READ_BUFFER
            assert g(0, 1, c=None) == ERR_NULL_POINTER
            assert g(0, 1, sp=None) == ERR_NULL_POINTER
            assert g(0, 1, d=None) == ERR_NULL_POINTER
    finally:
        L.blosc2_free_ctx(dctx)
    cp = hip.Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = LZ4, 5, 4, 1, 32768, 3
    cp.filters[5] = 1
    cctx = L.blosc2_create_cctx(cp)
    assert cctx
    try:
        dest = np.zeros(64, np.uint8)
        assert L.blosc2_getitem_ctx(cctx, hip._ptr(src), len(chunk), 0, 1, hip._ptr(dest), 64) == ERR_INVALID_PARAM
    finally:
        L.blosc2_free_ctx(cctx)
