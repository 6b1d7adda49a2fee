"""Strided window writes (csrc/update_plan.h over StridedWindowSpec, csrc/update_kernel.h: StridedPatchBlock) on the host lane emulator.

tests/emu/window_write_strided_emu.cpp (which includes window_write_emu.cpp: the plain calls of the same library are the col_pitch 1
comparison), emu.cpp and wide_emu.cpp are compiled into a library in a pytest temp directory.  Every call's new chunks must equal
the oracle's compress of the edited pixels -- numpy assignment plane[origin + r * row_pitch + c * col_pitch] = src[r, c], window after
window in call order, into the oracle's decode of the old chunks; the stats prove which blocks were staged and re-encoded."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import _special_chunks as SC
import _trunc as T
import _window_writes_strided as S
from _window_writes import BLOSCLZ, LZ4, ZSTD
from _window_writes import expected as plain_expected
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes, windows
from cimg import synth

CANARY = 0x5A


class CParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32), ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


def cp(ts, clevel=5, blocksize=8192, compcode=LZ4, splitmode=3, filt=1, trunc=None):
    p = CParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    if trunc is not None:
        p.filters[4], p.filters_meta[4] = 4, trunc & 0xFF
    return p


def ocp(ts, clevel=5, blocksize=8192, compcode=LZ4, splitmode=3, filt=1):
    return O.cparams(ts, clevel=clevel, blocksize=blocksize, compcode=compcode, splitmode=splitmode, filters=(0, 0, 0, 0, 0, filt))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return S.build_emu(tmp_path_factory.mktemp("window_write_strided_emu"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update(L, p, chunks, specs, src, destsize, host=False, strided=True, comp_size=True):
    """-> (rc, status, new chunks (bytes, or None where untouched), new_cbytes, stats, canaries intact)"""
    buf, off, cs = concat(chunks)
    before = buf.copy()
    nb, bs = sizes(chunks)
    n = len(chunks)
    ds = np.asarray(destsize, np.int32)
    st = np.zeros(n, np.int32)
    ncb = np.zeros(n, np.int32)
    w = S.swindows(specs) if strided else windows(specs)
    csp = _p(cs) if comp_size else None
    intact = True
    if host:
        ptrs = (C.c_void_p * n)()
        fn = L.wwsemu_update_host if strided else L.wwemu_update_host
        rc = fn(C.byref(p), n, _p(buf), _p(off), csp, _p(ds), len(specs), w, _p(src), ptrs, _p(ncb), _p(st))
        new = []
        for i in range(n):
            new.append(C.string_at(ptrs[i], int(ncb[i])) if ptrs[i] else None)
            if ptrs[i]:
                L.wwemu_free(ptrs[i])
    else:
        new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
        nbuf = np.full(int(new_off[-1]) + int(ds[-1]) + 64, CANARY, np.uint8)
        fn = L.wwsemu_update_device if strided else L.wwemu_update_device
        rc = fn(C.byref(p), n, _p(buf), _p(off), csp, _p(nb), _p(bs), _p(ds), len(specs), w, _p(src), _p(nbuf), _p(new_off), _p(ncb), _p(st))
        new = [nbuf[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]
        if rc == ERR_INVALID_PARAM:
            intact = bool((nbuf == CANARY).all())
    assert np.array_equal(buf, before), "the input chunks were modified"
    stats = np.zeros(4, np.int64)
    L.wwemu_update_stats(_p(stats))
    return rc, st, new, ncb, stats, intact


def schedule(L):
    out = np.zeros(2, np.int64)
    L.wwsemu_schedule_stats(_p(out))
    return int(out[0]), int(out[1])


def pixels(ts, elems, seed=0):
    rng = np.random.default_rng(seed)
    base = synth.tiled_channel(np.float16, 64, max(elems * ts // 128 + 1, 1)).view(np.uint8).ravel()
    raw = base[:elems * ts].copy()
    raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)
    return raw


_cases = {}


def case(ts, codec=LZ4, filt=1, split=3, clevel=5):
    """the matrix plane of typesize ts as the oracle's chunks (shared, read-only)"""
    key = (ts, codec, filt, split, clevel)
    if key not in _cases:
        po = ocp(ts, clevel=clevel, compcode=codec, splitmode=split, filt=filt)
        chunks = oracle_chunks(po, pixels(ts, S.ELEMS), S.CHUNK_ELEMS * ts)
        _cases[key] = (po, chunks, [S.CHUNK_ELEMS * ts + 32] * len(chunks))
    return _cases[key]


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts,filt,split", S.MATRIX)
def test_matrix_matches_oracle(L, codec, ts, filt, split):
    po, chunks, ds = case(ts, codec, filt, split)
    specs, src = S.source(S.matrix_windows(ts), ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    nb, bs = sizes(chunks)
    blocks = len(S.touched_blocks(specs, nb, bs, ts))
    try:
        for order in (0, 1, 2):
            L.emu_set_write_order(order)
            for host in (False, True):
                rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 8192, codec, split, filt), chunks, specs, src, ds, host=host)
                assert rc == 0 and not st.any(), (order, host, rc, st)
                for i, (a, b) in enumerate(zip(new, want)):
                    assert a == b, (order, host, i, None if a is None else len(a), None if b is None else len(b))
                if stats[2] == 0:                       # (chunks that come out memcpyed are recompressed whole)
                    assert stats[1] == blocks, (stats, blocks)
    finally:
        L.emu_set_write_order(0)


def unit_windows(ts, n, dup, seed=7):
    """n distinct 1 x 1 windows in block 1 of chunk 0, then dup more that hit elements already written (other values)"""
    rng = np.random.default_rng(seed)
    epb = 8192 // ts
    at = epb + 3 + rng.choice(epb - 10, n, replace=False)
    at = np.concatenate([at, rng.choice(at, dup)])
    return [S.win(int(a), 1, 1) for a in at]              # (a 1 x 1 window is dense whatever its col_pitch: the planner makes cpitch = typesize)


@pytest.mark.parametrize("ts", [2, 3])
def test_unit_of_300_pixels_takes_the_disjoint_schedule_and_duplicates_the_ordered_one(L, ts):
    po, chunks, ds = case(ts)
    try:
        for order in (0, 1, 2):
            L.emu_set_write_order(order)
            for dup, sched in ((0, (1, 0)), (20, (0, 1))):
                specs, src = S.source(unit_windows(ts, 300, dup), ts)
                want, edited = S.expected(po, chunks, specs, ts, src, ds)
                rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, ds)
                assert rc == 0 and new == want, (order, dup)
                assert schedule(L) == sched, (order, dup, schedule(L))
                assert stats[0] == 1 and stats[1] == 1 and [c is not None for c in new] == [True, False, False]
                if dup:                                  # the last value wins
                    s = specs[-1]
                    o = s["out_off"]
                    assert bytes(edited[0][s["origin"] * ts:s["origin"] * ts + ts]) == bytes(src[o:o + ts])
    finally:
        L.emu_set_write_order(0)


@pytest.mark.parametrize("ts", [1, 2, 3, 4])
def test_disjoint_unit_of_strided_windows(L, ts):
    """windows with cpitch != typesize, more than 64 samples a row, no common byte: one unit, disjoint schedule, per-element stores"""
    po, chunks, ds = case(ts)
    specs, src = S.source(S.disjoint_strided_unit(ts), ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    try:
        for order in (0, 1, 2):
            L.emu_set_write_order(order)
            for host in (False, True):
                rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, ds, host=host)
                assert rc == 0 and new == want, (order, host)
                assert schedule(L) == (1, 0), (order, host, schedule(L))
                assert stats[0] == 1 and stats[1] == 1 and [c is not None for c in new] == [True, False, False]
    finally:
        L.emu_set_write_order(0)


def plain_shapes(elems, W_, chunk_elems, nchunks):
    """the windows of test_emu_window_writes.py's matrix"""
    mid = chunk_elems // W_
    s = [dict(origin=elems // 2 + 5, row_pitch=1, width=1, height=1), dict(origin=3 * W_ + 7, row_pitch=W_, width=W_ - 20, height=1),
         dict(origin=W_ * 4 + 17, row_pitch=W_, width=1, height=60), dict(origin=W_ * 50, row_pitch=W_, width=W_, height=9),
         dict(origin=max(mid - 2, 0) * W_ + W_ - 37, row_pitch=W_, width=53, height=5),
         dict(origin=W_ * 70 + 3, row_pitch=W_, width=40, height=12), dict(origin=W_ * 75 + 20, row_pitch=W_, width=40, height=12),
         dict(origin=0, row_pitch=1, width=8192, height=1)]                   # (covers block 0 of chunk 0 for every typesize: not staged)
    for d in s:
        d["chunk_first"], d["chunk_count"] = 0, nchunks
    return s


@pytest.mark.parametrize("ts,codec,clevel", [(1, LZ4, 5), (3, BLOSCLZ, 5), (4, LZ4, 5), (4, LZ4, 0)])
def test_col_pitch_1_equals_the_plain_call(L, ts, codec, clevel):
    po, chunks, ds = case(ts, codec, clevel=clevel)
    specs, src = S.source(plain_shapes(S.ELEMS, S.ROW, S.CHUNK_ELEMS, len(chunks)), ts)
    p = cp(ts, clevel, 8192, codec)
    # a tight destsize too: the hand-back to the whole route
    for dsz in (ds, [len(c) + 8 for c in chunks]):
        for host in (False, True):
            a = update(L, p, chunks, specs, src, dsz, host=host, strided=False)
            b = update(L, p, chunks, S.with_col_pitch(specs), src, dsz, host=host, strided=True)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), (host, a[0], b[0])
            assert np.array_equal(a[4], b[4]), (host, a[4], b[4])
            if dsz is ds:
                assert a[0] == 0 and a[2] == plain_expected(po, chunks, specs, ts, src, dsz)[0]


def test_stats_and_untouched_chunks(L):
    ts = 2
    po, chunks, ds = case(ts)
    nb, bs = sizes(chunks)
    far = 2 * S.CHUNK_ELEMS + 100
    for wins in ([S.win(5, 2, 1, col_pitch=far)],                                               # chunks 0 and 2; chunk 1 lies between the samples
                 [S.win(7, 3, 3, row_pitch=2 * 4096 + 50, col_pitch=4096 + 7)],                 # one sample a block: the blocks between are left
                 [S.win(S.ROW * 3 + 1, 40, 30, col_pitch=4), S.win(9000, 200, 2, row_pitch=9000, col_pitch=45)]):
        specs, src = S.source(wins, ts)
        want, _ = S.expected(po, chunks, specs, ts, src, ds)
        blocks = S.touched_blocks(specs, nb, bs, ts)
        tch = {c for c, _ in blocks}
        for host in (False, True):
            rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, ds, host=host)
            assert rc == 0 and new == want
            assert stats[1] == len(blocks) and stats[0] == len(blocks) and stats[2] == 0, (stats, len(blocks))
            assert [int(c) > 0 for c in ncb] == [i in tch for i in range(3)]
            if host:
                assert stats[3] == sum(len(chunks[i]) for i in tch) + sum(s["width"] * s["height"] * ts for s in specs), stats
    assert len(S.touched_blocks(S.source([S.win(5, 2, 1, col_pitch=far)], ts)[0], nb, bs, ts)) == 2


def emu_compress(L, p):
    def f(piece, d):
        piece = np.ascontiguousarray(piece)
        out = np.zeros(d + 64, np.uint8)
        c = np.zeros(1, np.int32)
        assert L.wemu_compress_batch(C.byref(p), 1, _p(piece), _p(np.zeros(1, np.int64)), _p(np.array([piece.size], np.int32)), _p(out),
                                     _p(np.zeros(1, np.int64)), _p(np.array([d], np.int32)), _p(c)) == 0
        return out[:c[0]].tobytes()
    return f


@pytest.mark.parametrize("codec,bs,clevel", [(ZSTD, 8192, 5), (LZ4, 131072, 9), (LZ4, 8192, 0)])
def test_whole_routes_match_the_emulators_compress(L, codec, bs, clevel):
    """zstd chunks, wide blocks and memcpyed (clevel 0) chunks: equal to the emulated engine's own compress of the edited pixels"""
    ts = 4
    chunk_elems = 40000 if bs > 8192 else S.CHUNK_ELEMS              # (a chunk holds a 128 KiB block and a leftover)
    elems = 2 * chunk_elems + 5001
    raw = pixels(ts, elems)
    p = cp(ts, clevel, bs, codec)
    comp = emu_compress(L, p)
    cb = chunk_elems * ts
    chunks = [comp(raw[o:o + cb], min(cb, raw.size - o) + 32) for o in range(0, raw.size, cb)]
    ds = [min(cb, raw.size - o) + 32 for o in range(0, raw.size, cb)]
    planes = {0: raw}
    specs, src = S.source(S.matrix_windows(ts, elems=elems, chunk_elems=chunk_elems), ts)
    want, _ = S.expected(None, chunks, specs, ts, src, ds, compress=comp, planes=planes)
    try:
        for order in (0, 1, 2):                          # (`want` was made in ascending order: the chunks are the same in every order)
            L.emu_set_write_order(order)
            for host in (False, True):
                rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds, host=host)
                assert rc == 0 and new == want, (codec, bs, clevel, host, order)
                if codec == ZSTD or clevel == 0:         # (128 KiB lz4 blocks still fit the staging: spliced, like the plain call)
                    assert stats[2] == 3 and stats[1] == 0, stats
    finally:
        L.emu_set_write_order(0)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_special_zero_and_repeated_value_chunks(L, host):
    chunks, plane = SC.six_chunks()                      # regular, value, nan, zero, memcpyed, uninit: 256 x 96 float32, 16 rows a chunk
    p = SC.plane_params()
    ts, PW = SC.TS, SC.PW
    # rows 20 .. 62, every 3rd, every 5th column: the value chunk (rows 16 .. 31), the nan chunk and the zero chunk (rows 48 .. 63)
    specs, src = S.source([S.win(20 * PW + 31, 40, 15, row_pitch=3 * PW, col_pitch=5, nchunks=6), S.win(50 * PW + 1, 1, 1, nchunks=6)], ts, seed=4)
    ds = [SC.CHUNK + 32] * 6
    want, edited = S.expected(p, chunks, specs, ts, src, ds, planes={0: np.ascontiguousarray(plane).view(np.uint8).ravel()})
    rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 4096), chunks, specs, src, ds, host=host)
    assert rc == 0 and not st.any(), (rc, st)
    assert [c is not None for c in new] == [False, True, True, True, False, False]
    assert new == want
    after = [c if c is not None else old for c, old in zip(new, chunks)]
    assert np.array_equal(np.concatenate([SC.want(c) for c in after]), edited[0])


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_trunc_prec_on_the_splice_route(L, host):
    """float32, 12 mantissa bits kept: written pixels are truncated like the chunk's own"""
    ts, m = 4, 12
    t = T.trunc(T.pixels("tiled", np.float32, 512, 48), ts, m)
    po = T.oracle_cparams(ts, m, clevel=5, blocksize=8192)
    chunks = oracle_chunks(po, t, 32768)
    ds = [32768 + 32] * len(chunks)
    n = len(chunks)
    specs, src = S.source([S.win(512 * 5 + 3, 100, 10, row_pitch=3 * 512, col_pitch=5, nchunks=n), S.win(512 * 20 + 9, 64, 4, row_pitch=512, nchunks=n)], ts)
    want, edited = S.expected(None, chunks, specs, ts, src, ds, compress=lambda raw, d: O.compress(po, T.trunc(raw, ts, m), destsize=d)[1])
    rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 8192, trunc=m), chunks, specs, src, ds, host=host)
    assert rc == 0 and new == want and stats[2] == 0 and stats[1] > 0, (rc, stats)
    assert any(c is not None for c in want)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_refusals_leave_everything_alone(L, host):
    ts = 2
    po, chunks, ds = case(ts)
    src = np.zeros(1 << 16, np.uint8)
    ok = dict(S.win(11, 20, 5, row_pitch=100, col_pitch=3), out_off=0, out_pitch=20 * ts)
    bad = [dict(ok, col_pitch=0), dict(ok, col_pitch=-2), dict(ok, row_pitch=57), dict(ok, origin=S.ELEMS - 57), dict(ok, origin=-1),
           dict(ok, col_pitch=S.ELEMS), dict(ok, height=S.ELEMS), dict(ok, out_pitch=20 * ts - 1), dict(ok, chunk_first=1), dict(ok, chunk_count=0)]
    for b in bad:
        rc, st, new, ncb, _, intact = update(L, cp(ts), chunks, [b], src, ds, host=host)
        assert rc == ERR_INVALID_PARAM and intact and all(x is None for x in new) and not ncb.any(), b
    for p in (cp(4), cp(ts, compcode=BLOSCLZ), cp(ts, filt=2), cp(ts, splitmode=2), cp(ts, blocksize=4096)):
        rc, st, new, ncb, _, intact = update(L, p, chunks, [ok], src, ds, host=host)
        assert rc == ERR_INVALID_PARAM and intact and all(x is None for x in new), (p.typesize, p.compcode, p.filters[5], p.splitmode, p.blocksize)
    rc, st, new, ncb, _, intact = update(L, cp(ts), chunks, [ok], src, [ds[0], 31, ds[2]], host=host)
    assert rc == ERR_INVALID_PARAM and intact
    # a good call afterwards
    specs, src2 = S.source([ok], ts)
    rc, st, new, ncb, _, _ = update(L, cp(ts), chunks, specs, src2, ds, host=host)
    assert rc == 0 and new == S.expected(po, chunks, specs, ts, src2, ds)[0]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_damaged_chunk_gets_its_status_and_the_others_are_written(L, host):
    ts = 4
    po, chunks, ds = case(ts)
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")                # block 2 of chunk 1 claims more than the chunk holds
    bad = chunks[:1] + [bytes(c)] + chunks[2:]
    specs, src = S.source([S.win(100, (S.CHUNK_ELEMS + 4200) // 3, 1, col_pitch=3)], ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    rc, st, new, ncb, _, _ = update(L, cp(ts), bad, specs, src, ds, host=host)
    assert rc < 0 and st[1] < 0 and st[0] == 0 and new[1] is None and ncb[1] == 0
    assert new[0] == want[0]


def test_under_sanitizers(tmp_path):
    """planner, proof and kernel body once more as a stand-alone ASan / UBSan program (tests/emu/window_write_strided_asan_main.cpp):
    every buffer an allocation of its exact size, LDS with zero slack"""
    exe = S.build_emu(tmp_path, sanitize=True)
    for order in ("0", "1", "2"):
        r = subprocess.run([exe, order], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ok" in r.stdout
