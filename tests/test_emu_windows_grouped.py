"""Grouped windows (csrc/window_plan.h: group_items, run_windows_grouped; csrc/window_kernel.h: GroupedWindowBlock) on the host lane
emulator.

tests/emu/window_grouped_emu.cpp (which includes the strided and the plain window emulators), emu.cpp and wide_emu.cpp are compiled
into a library in a pytest temp directory (_windows_grouped.build_emu).  Every grouped call is compared byte for byte -- output,
status[] and return code -- with the strided call of the same emulator over the same windows and with numpy indexing into the
oracle's decode; every byte outside the windows must keep its canary.  blocks_decoded must equal the brute-force count of distinct
blocks, where the strided call reports one per (window, block).  Planner, grouping and kernel body run once more in a stand-alone
AddressSanitizer / UBSan program (tests/emu/window_grouped_asan_main.cpp) with every buffer an allocation of its exact size.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import _windows_grouped as G
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, pack, plane_of, sizes
from _windows_grouped import BLOSCLZ, LZ4, ZSTD, H, W, rect
from _windows_strided import expected, sampled_blocks, swindows


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return G.build_emu(tmp_path_factory.mktemp("window_grouped_emu"))


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return G.build_emu(tmp_path_factory.mktemp("window_grouped_asan"), sanitize=True)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def engine_chunks(L, ts, raw, chunk_bytes, compcode=LZ4, clevel=5, blocksize=8192, splitmode=3, filt=1):
    """raw cut into chunks and compressed by the emulated engine kernels -> list of bytes"""
    p = G.EmuCParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    nb = np.array([min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)], np.int32)
    n = nb.size
    raw_off = np.concatenate([[0], np.cumsum(nb[:-1])]).astype(np.int64)
    dest = (nb + 96).astype(np.int32)
    comp_off = np.concatenate([[0], np.cumsum(dest[:-1].astype(np.int64))]).astype(np.int64)
    comp = np.zeros(int(dest.sum()) + 64, np.uint8)
    cb = np.zeros(n, np.int32)
    rc = L.wemu_compress_batch(C.byref(p), n, _p(np.ascontiguousarray(raw)), _p(raw_off), _p(nb), _p(comp), _p(comp_off), _p(dest), _p(cb))
    assert rc == 0, rc
    return [comp[comp_off[i]:comp_off[i] + cb[i]].tobytes() for i in range(n)]


def call(L, chunks, specs, ts, size, host=False, grouped=True, nbytes=None, blocksize=None):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    out = np.full(size, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    w = swindows(specs)
    kind = "grouped" if grouped else "strided"
    if host:
        rc = getattr(L, "wnemu_windows_%s_host" % kind)(len(chunks), _p(buf), _p(off), _p(cs), len(specs), w, _p(out), _p(st))
    else:
        rc = getattr(L, "wnemu_windows_%s_device" % kind)(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), ts, len(specs), w, _p(out),
                                                          _p(st))
    stats = np.zeros(3, np.int64)
    L.wnemu_window_stats(_p(stats))
    return rc, st, out, stats


def check(L, chunks, planes, specs, ts, whole=False, orders=(0,)):
    """grouped == strided == numpy, device and host form; returns the grouped stats of the last call"""
    nb, bs = sizes(chunks)
    specs, size = pack(specs, ts)
    want = expected(planes, specs, ts, size)
    items, touched = sampled_blocks(specs, nb, bs, ts)
    distinct = len(G.touched_blocks(specs, nb, bs, ts))
    for host in (False, True):
        rc0, st0, out0, stats0 = call(L, chunks, specs, ts, size, host=host, grouped=False)
        assert rc0 == 0 and np.array_equal(out0, want)
        for order in orders:
            L.emu_set_write_order(order)
            try:
                rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
            finally:
                L.emu_set_write_order(0)
            assert rc == rc0 and np.array_equal(st, st0) and not st.any(), (rc, st)
            assert np.array_equal(out, want)
            assert np.array_equal(out, out0)
            if whole:
                assert stats[0] == 0 and stats0[0] == 0 and stats[1] == stats0[1] == len(touched)
            else:
                assert stats[0] == distinct and stats0[0] == items and stats[1] == 0, (stats, stats0, distinct, items)
            assert stats[2] == stats0[2]                                          # the host call uploads the same chunks
            if host:
                assert stats[2] == sum(len(chunks[i]) for i in touched)
    return stats


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_oracle_chunks(L, codec, ts, filt):
    cbytes, bsize = G.GEOMETRY[ts]
    raw = G.plane(ts)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, compcode=codec, filters=(0, 0, 0, 0, 0, filt)), raw, cbytes)
    nb, bs = sizes(chunks)
    assert len(chunks) >= 3 and sum(-(-int(n) // int(b)) for n, b in zip(nb, bs)) >= 9
    check(L, chunks, [plane_of(chunks)] * 100, G.matrix_windows(len(chunks)), ts, orders=(0, 1, 2))


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ, ZSTD])
@pytest.mark.parametrize("ts,filt,split", [(4, 1, 3), (4, 1, 1), (2, 2, 3), (3, 1, 3), (8, 0, 3), (1, 1, 3)])
def test_engine_chunks(L, codec, ts, filt, split):
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = engine_chunks(L, ts, G.plane(ts), cbytes, compcode=codec, blocksize=bsize, splitmode=split, filt=filt)
    check(L, chunks, [plane_of(chunks)] * 100, G.matrix_windows(len(chunks)), ts, whole=codec == ZSTD)   # zstd: the whole route


def test_memcpyed_and_zero_chunks(L):
    cbytes, bsize = G.GEOMETRY[4]
    chunks = oracle_chunks(O.cparams(4, clevel=0, blocksize=bsize), G.plane(4), cbytes)             # memcpyed
    check(L, chunks, [plane_of(chunks)] * 100, G.matrix_windows(len(chunks)), 4, orders=(0, 2))
    zeros = np.zeros(W * H * 4, np.uint8)                                                           # all-zero chunks (special value)
    chunks = engine_chunks(L, 4, zeros, cbytes, blocksize=bsize)
    check(L, chunks, [zeros] * 100, G.matrix_windows(len(chunks)), 4)


def test_mixed_chunk_kinds_in_one_call(L):
    """chunk 0 lz4, chunk 1 memcpyed, chunk 2 zstd (whole route, copy-mode units), chunks 3, 4 blosclz: one plane, one call"""
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]
    raw = G.plane(ts)
    a = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), raw, cbytes)
    m = oracle_chunks(O.cparams(ts, clevel=0, blocksize=bsize), raw, cbytes)
    z = engine_chunks(L, ts, raw, cbytes, compcode=ZSTD, blocksize=bsize)
    b = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, compcode=BLOSCLZ), raw, cbytes)
    chunks = [a[0], m[1], z[2], b[3], b[4]]
    nb, bs = sizes(chunks)
    specs, size = pack(G.matrix_windows(5), ts)
    want = expected([np.asarray(raw)] * len(specs), specs, ts, size)
    for host in (False, True):
        rc0, st0, out0, stats0 = call(L, chunks, specs, ts, size, host=host, grouped=False)
        rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
        assert rc == rc0 == 0 and not st.any() and not st0.any()
        assert np.array_equal(out, want) and np.array_equal(out0, want)
        assert stats[1] == stats0[1] == 1
        assert stats[0] == len({cb for cb in G.touched_blocks(specs, nb, bs, ts) if cb[0] != 2})


def test_two_planes_that_share_a_chunk(L):
    """Plane A is chunks 0 .. 2, plane B chunks 2 .. 4: windows of both meet blocks of chunk 2, which are staged once and written
    with each window's own plane offset."""
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), G.plane(ts), cbytes)
    assert len(chunks) == 5
    nb, bs = sizes(chunks)
    ce = cbytes // ts                                             # 15 360 elements a chunk: 30 rows of W
    A, B = plane_of(chunks[0:3]), plane_of(chunks[2:5])
    rows = ce // W
    specs = [rect(10, 2 * rows + 3, 300, 12, nchunks=3, chunk_first=0),           # rows 3 .. 14 of chunk 2, seen from plane A
             rect(200, 5, 250, 20, 3, 2, nchunks=3, chunk_first=2),               # rows 5 .. 24 of chunk 2, seen from plane B
             rect(0, 7, 1, 1, nchunks=3, chunk_first=2),
             rect(0, 2 * rows + 7, 1, 1, nchunks=3, chunk_first=0),               # the same pixel through plane A
             rect(0, rows - 2, W, 4, nchunks=3, chunk_first=0),                    # plane A alone: chunks 0 and 1
             rect(0, 2 * rows - 1, W, 3, nchunks=3, chunk_first=2)]                # plane B alone: chunks 3 and 4
    stats = check(L, chunks, [A, B, B, A, A, B], specs, ts, orders=(0, 1, 2))
    shared = {cb for cb in G.touched_blocks(specs[:1] + specs[3:4], nb, bs, ts)} & {cb for cb in G.touched_blocks(specs[1:3], nb, bs, ts)}
    assert shared and all(c == 2 for c, _ in shared)


@pytest.mark.parametrize("k", [1, 4, 5, 70])
def test_unit_of_k_items(L, k):
    """k 1 x 1 windows in one block: one unit of exactly k items -- the single-item path (all 256 threads), one item a wave, the
    round-robin's remainder, and many rounds"""
    ts = 4
    cbytes, bsize = G.GEOMETRY[ts]                                # 8192-byte blocks: 4 rows of W float32
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, filters=(0, 0, 0, 0, 0, 2)), G.plane(ts), cbytes)
    specs = [rect((37 * i) % W, 8 + i % 4, 1, 1, nchunks=len(chunks)) for i in range(k)]          # rows 8 .. 11: block 2 of chunk 0
    stats = check(L, chunks, [plane_of(chunks)] * k, specs, ts, orders=(0, 1, 2))
    assert stats[0] == 1


def test_group_items_units(L):
    """the grouping on its own: stable by block, decode units in block order with their items in window order, copy-mode items
    behind them as units of one"""
    b = np.array([5, 2, -1, 5, 2, 9, -1, 5, 2, 2, 0], np.int32)
    order = np.zeros(b.size, np.int32)
    u0, un = np.zeros(b.size, np.int32), np.zeros(b.size, np.int32)
    n = L.wnemu_group_items(b.size, _p(b), _p(order), _p(u0), _p(un))
    assert list(order) == [10, 1, 4, 8, 9, 0, 3, 7, 5, 2, 6]
    assert n == 6
    assert list(zip(u0[:n], un[:n])) == [(0, 1), (1, 4), (5, 3), (8, 1), (9, 1), (10, 1)]
    assert L.wnemu_group_items(0, _p(b), _p(order), _p(u0), _p(un)) == 0
    # blocks far apart (a range much larger than the items): the same answer from the key sort
    far = np.where(b >= 0, b.astype(np.int64) * 1000003 % (2 ** 31 - 1), -1).astype(np.int32)
    assert len(set(far[b >= 0])) == 4 and far.max() > 8 * b.size + 4096
    rank = {v: i for i, v in enumerate(sorted(set(far[far >= 0])))}
    n = L.wnemu_group_items(far.size, _p(far), _p(order), _p(u0), _p(un))
    want = sorted(range(far.size), key=lambda k: (rank[far[k]] if far[k] >= 0 else 99, k))
    assert list(order) == want and n == 6
    assert [int(x) for x in un[:n]] == [int((far == u).sum()) for u in sorted(set(far[far >= 0]))] + [1, 1]


def test_worked_stats_example(L):
    """float32, 512 x 96, chunk 65 536, block 32 768: 16 rows a block, 6 blocks.  Windows (0, 0, 16, 16), (100, 4, 32, 8) and
    (480, 15, 32, 2) meet blocks 0 and 1: the grouped call stages 2 blocks, the strided call 4 items.  Seventy 1 x 1 windows in
    rows 0 .. 15: 1 against 70.  Disjoint windows that share no block: equal counts."""
    ts = 4
    raw = G.plane(ts)[:W * 96 * ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=32768), raw, 65536)
    nb, bs = sizes(chunks)
    assert len(chunks) == 3 and (bs == 32768).all() and (nb == 65536).all()
    plane = plane_of(chunks)

    def stats_of(specs):
        specs, size = pack(specs, ts)
        res = {}
        for host in (False, True):
            for grouped in (True, False):
                rc, st, out, stats = call(L, chunks, specs, ts, size, host=host, grouped=grouped)
                assert rc == 0 and not st.any()
                assert np.array_equal(out, expected([plane] * len(specs), specs, ts, size))
                res[host, grouped] = int(stats[0])
        assert res[False, True] == res[True, True] and res[False, False] == res[True, False]
        return res[False, True], res[False, False]

    assert stats_of([rect(0, 0, 16, 16, nchunks=3), rect(100, 4, 32, 8, nchunks=3), rect(480, 15, 32, 2, nchunks=3)]) == (2, 4)
    assert stats_of([rect((7 * i) % W, i % 16, 1, 1, nchunks=3) for i in range(70)]) == (1, 70)
    assert stats_of([rect(10 + 50 * j, 16 * j + 3, 40, 9, nchunks=3) for j in range(6)]) == (6, 6)


def test_zero_sized_windows_and_no_windows(L):
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, blocksize=bsize), G.plane(ts), cbytes)
    specs, size = pack([rect(5, 5, 0, 4, nchunks=5), rect(5, 5, 4, 0, 2, 3, nchunks=5)], ts)
    for host in (False, True):
        rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
        assert rc == 0 and not st.any() and (out == CANARY).all() and not stats[:2].any()
        rc, st, out, stats = call(L, chunks, [], ts, 64, host=host)
        assert rc == 0 and (out == CANARY).all() and not stats.any()


I64, I32 = 2 ** 63 - 1, 2 ** 31 - 1


@pytest.mark.parametrize("host", [False, True])
def test_invalid_windows_are_refused_as_the_strided_call_refuses_them(L, host):
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, blocksize=bsize), G.plane(ts), cbytes)
    ok = dict(rect(10, 10, 80, 20, 4, 2, nchunks=5), out_off=0, out_pitch=20 * ts)
    bad = [dict(ok, col_pitch=0), dict(ok, col_pitch=-1), dict(ok, row_pitch=19 * 4), dict(ok, origin=W * H - 19 * 4, height=1),
           dict(ok, col_pitch=I64), dict(ok, col_pitch=I64, width=I32, height=I32, out_pitch=I64), dict(ok, row_pitch=I64 // 4 + 1),
           dict(ok, origin=-1), dict(ok, width=-1), dict(ok, height=-2), dict(ok, out_pitch=20 * ts - 1), dict(ok, chunk_first=1),
           dict(ok, chunk_first=-1), dict(ok, chunk_count=0), dict(ok, chunk_count=I32)]
    good, size = pack([ok], ts)
    for b in bad:
        for specs in ([b], [good[0], b]):
            rc0, _, _, _ = call(L, chunks, specs, ts, size, host=host, grouped=False)
            rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
            assert rc == rc0 == ERR_INVALID_PARAM, (b, rc, rc0)
            assert (out == CANARY).all() and not stats.any()                  # nothing run
    rc, st, out, _ = call(L, chunks, good, ts, size, host=host)
    assert rc == 0 and np.array_equal(out, expected([plane_of(chunks)], good, ts, size))


def damaged(ts=4):
    cbytes, bsize = G.GEOMETRY[ts]
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), G.plane(ts), cbytes)
    good = plane_of(chunks)
    c = bytearray(chunks[1])
    j = 2                                                     # block 2 of chunk 1: rows 30 + [8, 12)
    start = int.from_bytes(c[32 + 4 * j:36 + 4 * j], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")  # block 2's first stream claims more bytes than the chunk holds
    chunks[1] = bytes(c)
    return chunks, good


@pytest.mark.parametrize("host", [False, True])
def test_damaged_chunk(L, host):
    """chunk 1 (rows 30 .. 59) has a damaged block: its status is set as the strided call sets it, the windows that meet chunk 1 are
    unspecified, and every other window is exact"""
    ts = 4
    chunks, good = damaged(ts)
    n = len(chunks)
    specs = [rect(0, 0, W, 29, nchunks=n), rect(7, 36, 200, 6, nchunks=n), rect(7, 39, 1, 1, nchunks=n), rect(50, 20, 100, 30, 3, 2, nchunks=n),
             rect(3, 61, 400, 60, 5, 3, nchunks=n), rect(100, 100, 1, 1, nchunks=n), rect(0, 60, W, 1, nchunks=n)]
    meets = [False, True, True, True, False, False, False]
    specs, size = pack(specs, ts)
    want = expected([good] * len(specs), specs, ts, size)
    rc0, st0, out0, _ = call(L, chunks, specs, ts, size, host=host, grouped=False)
    rc, st, out, _ = call(L, chunks, specs, ts, size, host=host)
    assert rc < 0 and rc == rc0 and np.array_equal(st, st0)
    assert st[1] == rc and not st[[0, 2, 3, 4]].any()
    for s, m in zip(specs, meets):
        lo, hi = s["out_off"], s["out_off"] + s["out_pitch"] * s["height"]
        if not m:
            assert np.array_equal(out[lo:hi], want[lo:hi]), s
    # nothing outside the windows is written, damaged or not
    mask = np.ones(size, bool)
    for s in specs:
        for r in range(s["height"]):
            o = s["out_off"] + r * s["out_pitch"]
            mask[o:o + s["width"] * ts] = False
    assert (out[mask] == CANARY).all()
    # windows that keep clear of chunk 1 alone: a clean call
    clear = [s for s, m in zip(specs, meets) if not m]
    rc, st, out, _ = call(L, chunks, clear, ts, size, host=host)
    assert rc == 0 and not st.any()
    assert np.array_equal(out, expected([good] * len(clear), clear, ts, size))


def case_blob(chunks, specs, ts, size, comp_size=None):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    w = swindows(specs)
    return b"".join([np.array([len(chunks), ts, size, len(specs)], np.int64).tobytes(), off.tobytes(),
                     (cs if comp_size is None else comp_size).tobytes(), nb.tobytes(), bs.tobytes(),
                     bytes(w)[:C.sizeof(w._type_) * len(specs)], np.array([buf.size], np.int64).tobytes(), buf.tobytes()])


def test_planner_grouping_and_kernel_under_asan(asan_exe, tmp_path):
    """The matrix in one call, with an output that ends at the last window's last byte; the units of 1, 4, 5 and 70 items; two planes
    that share a chunk; the damaged chunk and a truncated buffer; invalid windows.  The sanitizers are the check, with the return
    codes and the program's own comparison of the grouped outputs with the strided call's."""
    path = tmp_path / "case.bin"

    def run(chunks, specs, ts, comp_size=None, order=0):
        at, packed = 0, []
        for s in specs:                                       # dense: no byte of the output is outside a window
            packed.append(dict(s, out_off=at, out_pitch=s["width"] * ts))
            at += s["width"] * ts * s["height"]
        path.write_bytes(case_blob(chunks, packed, ts, at, comp_size))
        r = subprocess.run([asan_exe, str(path), str(order)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [int(x) for x in r.stdout.split()[:4]]

    for ts, filt, order in ((3, 1, 0), (4, 2, 1), (2, 0, 2), (8, 1, 0)):
        cbytes, bsize = G.GEOMETRY[ts]
        chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, filters=(0, 0, 0, 0, 0, filt)), G.plane(ts), cbytes)
        assert run(chunks, G.matrix_windows(len(chunks)), ts, order=order) == [0, 0, 0, 1]
    cbytes, bsize = G.GEOMETRY[4]
    chunks = oracle_chunks(O.cparams(4, clevel=5, blocksize=bsize), G.plane(4), cbytes)
    for k in (1, 4, 5, 70):
        assert run(chunks, [rect((37 * i) % W, 8 + i % 4, 1, 1, nchunks=len(chunks)) for i in range(k)], 4, order=k % 3) == [0, 0, 0, 1]
    assert run(chunks, [rect(10, 63, 300, 12, nchunks=3, chunk_first=0), rect(200, 5, 250, 20, 3, 2, nchunks=3, chunk_first=2),
                        rect(0, 7, 1, 1, nchunks=3, chunk_first=2)], 4) == [0, 0, 0, 1]
    bad, _ = damaged(4)
    _, _, cs = concat(bad)
    n = len(bad)
    inside = [rect(7, 36, 200, 6, nchunks=n), rect(7, 39, 1, 1, nchunks=n), rect(0, 0, W, 29, nchunks=n)]
    outside = [rect(0, 0, W, 29, nchunks=n), rect(3, 61, 400, 60, 5, 3, nchunks=n)]
    for specs, fails in ((inside, True), (outside, False)):
        for trunc in (0, 1):
            sz = cs.copy()
            if trunc:
                sz[0] = 100
            a, b, c, _ = run(bad, specs, 4, sz)
            if fails or trunc:
                assert a < 0 and b < 0 and c < 0, (trunc, a, b, c)
            else:
                assert [a, b, c] == [0, 0, 0]
    ok = rect(10, 10, 80, 20, 4, 2, nchunks=n)
    for b in (dict(ok, col_pitch=0), dict(ok, origin=W * H - 19 * 4, height=1), dict(ok, chunk_count=I32), dict(ok, width=-1)):
        path.write_bytes(case_blob(bad, [dict(ok, out_off=0, out_pitch=80), dict(b, out_off=0, out_pitch=1 << 20)], 4, 4096))
        r = subprocess.run([asan_exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert [int(x) for x in r.stdout.split()[:3]] == [ERR_INVALID_PARAM] * 3, b
