"""Grouped windows on the MI355X: cimg_decompress_windows_grouped_device / _host (csrc/window_kernel.h: cimg_decode_window_grouped,
csrc/window_plan.h: group_items).

The matrix of tests/test_emu_windows_grouped.py at the same small shapes through the real engine, device call and host call.  Every
grouped call is compared byte for byte -- output, status[], return code -- with the strided call on the same engine over the same
windows and with numpy indexing into the decoded plane; canaries between the rows must survive; blocks_decoded must equal the
brute-force count of distinct blocks, where the strided call reports one per (window, block).  Every hostile input here is one the
host refuses before anything is launched, or a damaged stream the staging code is known to refuse.
"""
import numpy as np
import pytest

import _oracle as O
import _windows_grouped as G
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, pack, sizes
from _windows_grouped import BLOSCLZ, LZ4, ZSTD, H, W, rect
from _windows_strided import expected, sampled_blocks
from cimg import hip

pytestmark = pytest.mark.gpu
I64, I32 = 2 ** 63 - 1, 2 ** 31 - 1


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def engine_chunks(eng, ts, raw, chunk_bytes, **kw):
    p = hip.cparams(ts, **kw)
    nb = [min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)]
    chunks = eng.compress_host(p, np.ascontiguousarray(raw), nb, [n + 64 for n in nb])
    assert all(len(c) > 0 for c in chunks)
    return chunks


def run_device(eng, chunks, specs, ts, size, grouped=True):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    rc, st = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False, strided=not grouped,
                                           grouped=grouped)
    stats = eng.window_stats()
    out = d_out.download()
    d_comp.free(); d_out.free()
    return rc, st, out, stats


def run_host(eng, chunks, specs, size, grouped=True):
    out = np.full(size, CANARY, np.uint8)
    rc, st = eng.decompress_windows_host(chunks, specs, out, check=False, strided=not grouped, grouped=grouped)
    return rc, st, out, eng.window_stats()


def pairs(eng, chunks, specs, ts, size):
    """(runner, the strided call's result, the grouped call's result)"""
    yield "device", run_device(eng, chunks, specs, ts, size, grouped=False), run_device(eng, chunks, specs, ts, size)
    yield "host", run_host(eng, chunks, specs, size, grouped=False), run_host(eng, chunks, specs, size)


def plane(chunks):
    return np.concatenate([O.decompress(c)[1] for c in chunks])


def check(eng, chunks, planes, specs, ts, whole=False):
    nb, bs = sizes(chunks)
    specs, size = pack(specs, ts)
    want = expected(planes, specs, ts, size)
    items, touched = sampled_blocks(specs, nb, bs, ts)
    distinct = len(G.touched_blocks(specs, nb, bs, ts))
    for runner, (rc0, st0, out0, stats0), (rc, st, out, stats) in pairs(eng, chunks, specs, ts, size):
        assert rc == 0 and rc0 == 0 and not st.any() and not st0.any(), (runner, rc, rc0, st, eng.last_error())
        assert np.array_equal(out0, want), runner
        assert np.array_equal(out, want), runner
        if whole:
            assert stats["blocks_decoded"] == 0 and stats["chunks_whole"] == stats0["chunks_whole"] == len(touched), (runner, stats)
        else:
            assert stats["blocks_decoded"] == distinct and stats0["blocks_decoded"] == items and stats["chunks_whole"] == 0, (runner, stats, stats0)
        assert stats["comp_bytes_uploaded"] == stats0["comp_bytes_uploaded"]
        if runner == "host":
            assert stats["comp_bytes_uploaded"] == sum(len(chunks[i]) for i in touched)
    return stats


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_oracle_chunks(eng, codec, ts, filt):
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, compcode=codec, filters=(0, 0, 0, 0, 0, filt)), G.plane(ts), cbytes)
    check(eng, chunks, [plane(chunks)] * 100, G.matrix_windows(len(chunks)), ts)


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ, ZSTD])
@pytest.mark.parametrize("ts,filt,split", [(4, 1, 3), (4, 1, 1), (2, 2, 3), (3, 1, 3), (8, 0, 3), (1, 1, 3)])
def test_engine_chunks(eng, codec, ts, filt, split):
    cbytes, bsize = G.GEOMETRY[ts]
    raw = G.plane(ts)
    chunks = engine_chunks(eng, ts, raw, cbytes, clevel=5, blocksize=bsize, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
    check(eng, chunks, [np.asarray(raw)] * 100, G.matrix_windows(len(chunks)), ts, whole=codec == ZSTD)


def test_memcpyed_and_zero_chunks(eng):
    cbytes, bsize = G.GEOMETRY[4]
    chunks = oracle_chunks(O.cparams(4, clevel=0, blocksize=bsize), G.plane(4), cbytes)
    check(eng, chunks, [plane(chunks)] * 100, G.matrix_windows(len(chunks)), 4)
    zeros = np.zeros(W * H * 4, np.uint8)
    chunks = engine_chunks(eng, 4, zeros, cbytes, blocksize=bsize)
    check(eng, chunks, [zeros] * 100, G.matrix_windows(len(chunks)), 4)


def test_mixed_chunk_kinds_in_one_call(eng):
    """chunk 0 lz4, chunk 1 memcpyed, chunk 2 zstd (whole route, copy-mode units), chunks 3, 4 blosclz: one plane, one call"""
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]
    raw = G.plane(ts)
    a = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), raw, cbytes)
    m = oracle_chunks(O.cparams(ts, clevel=0, blocksize=bsize), raw, cbytes)
    z = engine_chunks(eng, ts, raw, cbytes, compcode=ZSTD, blocksize=bsize)
    b = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, compcode=BLOSCLZ), raw, cbytes)
    chunks = [a[0], m[1], z[2], b[3], b[4]]
    nb, bs = sizes(chunks)
    specs, size = pack(G.matrix_windows(5), ts)
    want = expected([np.asarray(raw)] * len(specs), specs, ts, size)
    for runner, (rc0, st0, out0, stats0), (rc, st, out, stats) in pairs(eng, chunks, specs, ts, size):
        assert rc == rc0 == 0 and not st.any() and not st0.any(), runner
        assert np.array_equal(out, want) and np.array_equal(out0, want), runner
        assert stats["chunks_whole"] == stats0["chunks_whole"] == 1
        assert stats["blocks_decoded"] == len({cb for cb in G.touched_blocks(specs, nb, bs, ts) if cb[0] != 2})


def test_two_planes_that_share_a_chunk(eng):
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), G.plane(ts), cbytes)
    A, B = plane(chunks[0:3]), plane(chunks[2:5])
    rows = cbytes // ts // W
    specs = [rect(10, 2 * rows + 3, 300, 12, nchunks=3, chunk_first=0), rect(200, 5, 250, 20, 3, 2, nchunks=3, chunk_first=2),
             rect(0, 7, 1, 1, nchunks=3, chunk_first=2), rect(0, 2 * rows + 7, 1, 1, nchunks=3, chunk_first=0),
             rect(0, rows - 2, W, 4, nchunks=3, chunk_first=0), rect(0, 2 * rows - 1, W, 3, nchunks=3, chunk_first=2)]
    check(eng, chunks, [A, B, B, A, A, B], specs, ts)


@pytest.mark.parametrize("k", [1, 4, 5, 70])
def test_unit_of_k_items(eng, k):
    """k 1 x 1 windows in one block: the single-item path, one item a wave, the round-robin's remainder, many rounds"""
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, filters=(0, 0, 0, 0, 0, 2)), G.plane(ts), cbytes)
    specs = [rect((37 * i) % W, 8 + i % 4, 1, 1, nchunks=len(chunks)) for i in range(k)]
    stats = check(eng, chunks, [plane(chunks)] * k, specs, ts)
    assert stats["blocks_decoded"] == 1


def test_worked_stats_example(eng):
    """float32, 512 x 96, chunk 65 536, block 32 768 (16 rows a block, 6 blocks): windows (0, 0, 16, 16), (100, 4, 32, 8) and
    (480, 15, 32, 2) stage blocks 0 and 1 -- 2 against the strided call's 4; seventy 1 x 1 windows in rows 0 .. 15: 1 against 70;
    disjoint windows that share no block: equal counts."""
    ts = 4
    raw = np.asarray(G.plane(ts)[:W * 96 * ts])
    chunks = engine_chunks(eng, ts, raw, 65536, clevel=5, blocksize=32768)
    nb, bs = sizes(chunks)
    assert len(chunks) == 3 and (bs == 32768).all()

    def stats_of(specs):
        specs, size = pack(specs, ts)
        want = expected([raw] * len(specs), specs, ts, size)
        got = set()
        for runner, (rc0, st0, out0, stats0), (rc, st, out, stats) in pairs(eng, chunks, specs, ts, size):
            assert rc == 0 and rc0 == 0 and np.array_equal(out, want) and np.array_equal(out0, want), runner
            got.add((stats["blocks_decoded"], stats0["blocks_decoded"]))
        assert len(got) == 1
        return got.pop()

    assert stats_of([rect(0, 0, 16, 16, nchunks=3), rect(100, 4, 32, 8, nchunks=3), rect(480, 15, 32, 2, nchunks=3)]) == (2, 4)
    assert stats_of([rect((7 * i) % W, i % 16, 1, 1, nchunks=3) for i in range(70)]) == (1, 70)
    assert stats_of([rect(10 + 50 * j, 16 * j + 3, 40, 9, nchunks=3) for j in range(6)]) == (6, 6)


def test_refusals_and_damaged_chunk(eng):
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), G.plane(ts), cbytes)
    good_plane = plane(chunks)
    n = len(chunks)
    ok = dict(rect(10, 10, 80, 20, 4, 2, nchunks=n), out_off=0, out_pitch=20 * ts)
    good, gsize = pack([ok], ts)
    for b in (dict(ok, col_pitch=0), dict(ok, row_pitch=19 * 4), dict(ok, origin=W * H - 19 * 4, height=1), dict(ok, col_pitch=I64),
              dict(ok, col_pitch=I64, width=I32, height=I32, out_pitch=I64), dict(ok, row_pitch=I64 // 4 + 1), dict(ok, chunk_first=1),
              dict(ok, chunk_count=0), dict(ok, chunk_count=I32), dict(ok, width=-1)):
        for runner, (rc0, st0, out0, stats0), (rc, st, out, stats) in pairs(eng, chunks, [good[0], b], ts, 1 << 15):
            assert rc == rc0 == ERR_INVALID_PARAM and (out == CANARY).all(), (runner, b)
            assert stats["blocks_decoded"] == 0 and stats["chunks_whole"] == 0
    for runner, _, (rc, st, out, stats) in pairs(eng, chunks, good, ts, gsize):                       # the engine stays usable
        assert rc == 0 and np.array_equal(out, expected([good_plane], good, ts, gsize)), runner
    # zero-sized windows and no windows at all
    empty, esize = pack([rect(5, 5, 0, 4, nchunks=n), rect(5, 5, 4, 0, 2, 3, nchunks=n)], ts)
    for specs in (empty, []):
        for runner, _, (rc, st, out, stats) in pairs(eng, chunks, specs, ts, esize):
            assert rc == 0 and not st.any() and (out == CANARY).all() and stats["blocks_decoded"] == 0, runner
    # block 2 of chunk 1 (rows 38 .. 41) claims more bytes than the chunk holds: the chunk's status is set as the strided call sets
    # it, windows that keep clear of chunk 1 are exact, and nothing outside the windows is written
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")
    bad = [chunks[0], bytes(c)] + chunks[2:]
    specs = [rect(0, 0, W, 29, nchunks=n), rect(7, 36, 200, 6, nchunks=n), rect(7, 39, 1, 1, nchunks=n), rect(50, 20, 100, 30, 3, 2, nchunks=n),
             rect(3, 61, 400, 60, 5, 3, nchunks=n), rect(100, 100, 1, 1, nchunks=n), rect(0, 60, W, 1, nchunks=n)]
    meets = [False, True, True, True, False, False, False]
    specs, size = pack(specs, ts)
    want = expected([good_plane] * len(specs), specs, ts, size)
    mask = np.ones(size, bool)
    for s in specs:
        for r in range(s["height"]):
            o = s["out_off"] + r * s["out_pitch"]
            mask[o:o + s["width"] * ts] = False
    for runner, (rc0, st0, out0, stats0), (rc, st, out, stats) in pairs(eng, bad, specs, ts, size):
        assert rc < 0 and rc == rc0 and np.array_equal(st, st0) and st[1] == rc and not st[[0, 2, 3, 4]].any(), runner
        for s, m in zip(specs, meets):
            lo, hi = s["out_off"], s["out_off"] + s["out_pitch"] * s["height"]
            if not m:
                assert np.array_equal(out[lo:hi], want[lo:hi]), (runner, s)
        assert (out[mask] == CANARY).all(), runner
    clear = [s for s, m in zip(specs, meets) if not m]
    for runner, _, (rc, st, out, stats) in pairs(eng, bad, clear, ts, size):
        assert rc == 0 and not st.any() and np.array_equal(out, expected([good_plane] * len(clear), clear, ts, size)), runner


def test_grouped_launches_its_own_kernel_and_leaves_the_others_alone(eng):
    """launch counts by kernel id, one launch a round: the two grouped calls launch cimg_decode_window_grouped and neither of the other
    window kernels; the four calls that were there before -- plain and strided, device and host -- launch the kernel they launched
    and never the grouped one"""
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), G.plane(ts), cbytes)
    specs, size = pack(G.matrix_windows(len(chunks)), ts)
    plain = [{k: v for k, v in s.items() if k != "col_pitch"} for s in specs if s["col_pitch"] == 1 and s["row_pitch"] == W]
    assert len(plain) >= 10
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp, d_out = eng.alloc(buf.size), eng.alloc(size)
    d_comp.upload(buf)
    host_out = np.zeros(size, np.uint8)
    kinds = (hip.K_DECODE_WINDOW, hip.K_DECODE_WINDOW_STRIDED, hip.K_DECODE_WINDOW_GROUPED)
    assert [hip.KERNELS[k] for k in kinds] == ["cimg_decode_window", "cimg_decode_window_strided", "cimg_decode_window_grouped"]

    def device(w, **kw):
        return lambda: eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, w, d_out.ptr, comp_size=cs, **kw)

    def host(w, **kw):
        return lambda: eng.decompress_windows_host(chunks, w, host_out, **kw)

    calls = [(device(plain), 0), (host(plain), 0), (device(specs, strided=True), 1), (host(specs, strided=True), 1),
             (device(specs, grouped=True), 2), (host(specs, grouped=True), 2)]
    eng.enable_timing(1)
    try:
        for n, (call, mine) in enumerate(calls):
            eng.reset_timing()
            call()
            assert [eng.kernel_time(k)[1] for k in kinds] == [int(j == mine) for j in range(3)], n
    finally:
        eng.enable_timing(0)
        d_comp.free(); d_out.free()
