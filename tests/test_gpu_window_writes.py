"""Window writes on the MI355X: cimg_update_windows_device / _host (csrc/update_plan.h, csrc/update_kernel.h).

New chunks must equal a from-scratch compress of the edited pixels: the oracle's for lz4 and blosclz, the engine's own for lz4hc, zstd
and wide blocks.  The stats show which blocks were staged and re-encoded."""
import numpy as np
import pytest

import _oracle as O
from _window_writes import BLOSCLZ, LZ4, LZ4HC, ZSTD, expected, source
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from cimg import hip, synth

pytestmark = pytest.mark.gpu
CANARY = 0x5A


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


def shapes(elems, W, chunk_elems, n):
    mid = chunk_elems // W
    s = [dict(origin=elems // 2 + 5, row_pitch=1, width=1, height=1),
         dict(origin=3 * W + 7, row_pitch=W, width=W - 20, height=1),
         dict(origin=W * 4 + 17, row_pitch=W, width=1, height=60),
         dict(origin=W * 50, row_pitch=W, width=W, height=9),
         dict(origin=max(mid - 2, 0) * W + W - 37, row_pitch=W, width=53, height=5),
         dict(origin=W * 70 + 3, row_pitch=W, width=40, height=12),
         dict(origin=W * 75 + 20, row_pitch=W, width=40, height=12)]
    for d in s:
        d["chunk_first"], d["chunk_count"] = 0, n
    return s


def run_device(eng, p, chunks, specs, src, ds):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    ds = np.asarray(ds, np.int32)
    new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    total = int(new_off[-1]) + int(ds[-1]) + 64
    d_comp, d_src, d_new = eng.alloc(buf.size), eng.alloc(max(src.size, 1)), eng.alloc(total)
    d_comp.upload(buf)
    d_src.upload(src)
    d_new.upload(np.full(total, CANARY, np.uint8))
    rc, ncb, st = eng.update_windows_device(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr, d_new.ptr, new_off, comp_size=cs, check=False)
    out = d_new.download()
    back = d_comp.download()
    d_comp.free(); d_src.free(); d_new.free()
    assert np.array_equal(back, buf), "the input chunks were modified"
    new = [out[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]
    return rc, st, new, out


def both(eng, p, chunks, specs, src, ds):
    rc, st, new, _ = run_device(eng, p, chunks, specs, src, ds)
    yield "device", rc, st, new, eng.update_stats()
    rc, new, st = eng.update_windows_host(p, chunks, ds, specs, src, check=False)
    yield "host", rc, st, new, eng.update_stats()


def engine_compress(eng, p):
    def f(raw, d):
        return eng.compress_host(p, np.ascontiguousarray(raw), [raw.size], [d])[0]
    return f


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts,filt,split", [(1, 1, 3), (2, 1, 3), (2, 2, 3), (4, 1, 3), (4, 1, 1), (4, 0, 3), (3, 1, 3)])
def test_matrix_matches_oracle(eng, codec, ts, filt, split):
    chunk_elems = 13000
    elems = 2 * chunk_elems + 5001
    raw = pixels(ts, elems)
    po = O.cparams(ts, clevel=5, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
    chunks = oracle_chunks(po, raw, chunk_elems * ts)
    ds = [chunk_elems * ts + 32] * len(chunks)
    specs, src = source(shapes(elems, 180, chunk_elems, len(chunks)), ts)
    want, _ = expected(po, chunks, specs, ts, src, ds)
    p = hip.cparams(ts, clevel=5, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
    for how, rc, st, new, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and not st.any(), (how, rc, st, eng.last_error())
        assert new == want, how


@pytest.mark.parametrize("codec,bs,clevel", [(LZ4HC, 8192, 5), (ZSTD, 8192, 5), (LZ4, 131072, 9), (LZ4, 262144, 9), (ZSTD, 262144, 5),
                                             (LZ4, 8192, 0)])
def test_other_routes_match_engine_compress(eng, codec, bs, clevel):
    ts = 4
    chunk = 1 << 20
    raw = pixels(ts, (3 * chunk + 40000) // ts)
    p = hip.cparams(ts, clevel=clevel, blocksize=bs, compcode=codec)
    nb = [min(chunk, raw.size - o) for o in range(0, raw.size, chunk)]
    ds = [chunk + 32] * len(nb)
    chunks = eng.compress_host(p, raw, nb, ds)
    elems = raw.size // ts
    specs, src = source([dict(chunk_first=0, chunk_count=len(nb), origin=100000 + 7, row_pitch=1000, width=300, height=400),
                         dict(chunk_first=0, chunk_count=len(nb), origin=elems - 10, row_pitch=1, width=10, height=1)], ts)
    want, _ = expected(None, chunks, specs, ts, src, ds, compress=engine_compress(eng, p))
    for how, rc, st, new, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and not st.any(), (how, rc, eng.last_error())
        assert new == want, how
        if codec == LZ4HC:
            assert stats["chunks_whole"] == 0 and stats["blocks_encoded"] > 0
        elif codec == ZSTD or clevel == 0:
            assert stats["chunks_whole"] == sum(x is not None for x in want)


def test_granularity_4096_float16(eng):
    ts, W = 2, 4096
    rng = np.random.default_rng(3)
    plane = synth.tiled_channel(np.float16, W, 1024).view(np.uint8).ravel().copy()
    plane[::301] ^= rng.integers(0, 255, plane[::301].size, dtype=np.uint8)
    chunk = 4 << 20
    po = O.cparams(ts)
    chunks = oracle_chunks(po, plane, chunk)
    ds = [chunk + 32] * len(chunks)
    p = hip.cparams(ts)
    for spec, dec in [(dict(origin=64 * W + 100, row_pitch=W, width=64, height=64), 16),
                      (dict(origin=128 * W, row_pitch=W, width=W, height=64), 0)]:
        spec.update(chunk_first=0, chunk_count=len(chunks))
        specs, src = source([spec], ts)
        want, _ = expected(po, chunks, specs, ts, src, ds)
        for how, rc, st, new, stats in both(eng, p, chunks, specs, src, ds):
            assert rc == 0 and new == want, how
            assert stats["blocks_decoded"] == dec and stats["blocks_encoded"] == 16 and stats["chunks_whole"] == 0, (how, stats)
            if how == "host":
                assert stats["bytes_uploaded"] == len(chunks[0]) + 64 * spec["width"] * ts


def test_large_plane_float32(eng):
    """a 1024^2 window into a device-resident 16384^2 float32 plane (1 GiB, 256 chunks of 4 MiB): only the 17 chunks the window's
    rows meet are rewritten, each equal to the oracle's compress of the edited pixels"""
    ts, W = 4, 16384
    plane = synth.tiled_channel(np.float32, W, W).view(np.uint8).ravel()
    chunk = 4 << 20
    p = hip.cparams(ts)
    nb = [chunk] * (plane.size // chunk)
    ds = [chunk + 32] * len(nb)
    stride = chunk + 64
    comp_off = np.arange(len(nb), dtype=np.int64) * stride
    raw_off = np.arange(len(nb), dtype=np.int64) * chunk
    d_raw = eng.alloc(plane.size)
    d_raw.upload(plane)
    d_comp = eng.alloc(stride * len(nb))
    cb = eng.compress_device(p, d_raw.ptr, raw_off, nb, d_comp.ptr, comp_off, ds)
    d_raw.free()
    assert (np.asarray(cb) > 0).all()
    x0, y0, n = 5000, 3000, 1024
    win = np.random.default_rng(5).integers(0, 1 << 20, (n, n)).astype(np.float32)
    src = win.view(np.uint8).ravel()
    spec = dict(chunk_first=0, chunk_count=len(nb), origin=y0 * W + x0, row_pitch=W, width=n, height=n, out_off=0, out_pitch=n * ts)
    d_src, d_new = eng.alloc(src.size), eng.alloc(stride * len(nb))
    d_src.upload(src)
    rc, ncb, st = eng.update_windows_device(p, d_comp.ptr, comp_off, nb, [32768] * len(nb), ds, [spec], d_src.ptr, d_new.ptr, comp_off,
                                            comp_size=cb, check=False)
    stats = eng.update_stats()
    out = d_new.download()
    d_comp.free(); d_src.free(); d_new.free()
    assert rc == 0 and not st.any(), eng.last_error()
    rows_per_chunk = chunk // (W * ts)
    touched = [i for i in range(len(nb)) if ncb[i] > 0]
    assert touched == list(range(y0 // rows_per_chunk, (y0 + n - 1) // rows_per_chunk + 1))
    edited = plane.view(np.float32).reshape(W, W).copy()
    edited[y0:y0 + n, x0:x0 + n] = win
    flat = edited.view(np.uint8).ravel()
    for i in touched:
        want = O.compress(O.cparams(ts), flat[i * chunk:(i + 1) * chunk], destsize=chunk + 32)[1]
        assert out[comp_off[i]:comp_off[i] + ncb[i]].tobytes() == want, i
    assert stats["chunks_whole"] == 0 and stats["blocks_encoded"] == stats["blocks_decoded"] > 0


def test_invalid_and_damaged(eng):
    ts = 2
    chunk_elems = 13000
    elems = 2 * chunk_elems + 5001
    po = O.cparams(ts, blocksize=8192)
    chunks = oracle_chunks(po, pixels(ts, elems), chunk_elems * ts)
    ds = [chunk_elems * ts + 32] * 3
    ok = dict(chunk_first=0, chunk_count=3, origin=10, row_pitch=100, width=20, height=5, out_off=0, out_pitch=20 * ts)
    src = np.zeros(1 << 16, np.uint8)
    good = hip.cparams(ts, blocksize=8192)
    bad_specs = [dict(ok, origin=elems - 10), dict(ok, width=-1), dict(ok, row_pitch=10), dict(ok, out_pitch=20 * ts - 1),
                 dict(ok, chunk_first=1), dict(ok, chunk_count=0)]
    for b in bad_specs:
        rc, st, new, out = run_device(eng, good, chunks, [b], src, ds)
        assert rc == ERR_INVALID_PARAM and (out == CANARY).all(), b
    for p in (hip.cparams(4, blocksize=8192), hip.cparams(ts, blocksize=8192, compcode=BLOSCLZ), hip.cparams(ts, blocksize=4096),
              hip.cparams(ts, blocksize=8192, filters=(0, 0, 0, 0, 0, 2))):
        rc, st, new, out = run_device(eng, p, chunks, [ok], src, ds)
        assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
        rc, new, st = eng.update_windows_host(p, chunks, ds, [ok], src, check=False)
        assert rc == ERR_INVALID_PARAM and all(x is None for x in new)
    rc, st, new, out = run_device(eng, good, chunks, [ok], src, [ds[0], 31, ds[2]])
    assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
    # a damaged chunk: its status, and the others are still written
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")
    bad = chunks[:1] + [bytes(c)] + chunks[2:]
    specs, src = source([dict(chunk_first=0, chunk_count=3, origin=100, row_pitch=1, width=chunk_elems + 4200, height=1)], ts)
    want, _ = expected(po, chunks, specs, ts, src, ds)
    for how, rc, st, new, stats in both(eng, good, bad, specs, src, ds):
        assert rc < 0 and st[1] < 0 and st[0] == 0 and new[1] is None and new[0] == want[0], how
    # the engine stays usable
    specs, src = source([ok], ts)
    want, _ = expected(po, chunks, specs, ts, src, ds)
    for how, rc, st, new, stats in both(eng, good, chunks, specs, src, ds):
        assert rc == 0 and new == want, how
