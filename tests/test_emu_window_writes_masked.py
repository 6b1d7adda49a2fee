"""Masked and constant window writes (csrc/update_plan.h over MaskedWindowSpec, csrc/update_kernel.h: MaskedPatchBlock) on the host
lane emulator.

tests/emu/window_write_masked_emu.cpp (which includes the typed, strided and plain write emulators: the strided calls of the same
library are the flags == 0 comparison), emu.cpp and wide_emu.cpp are compiled into a library in a pytest temp directory.  Every
call's new chunks must equal the oracle's compress of the edited pixels -- np.copyto(view, src_or_value, where=mask), window after
window in call order, into the oracle's decode of the old chunks; the stats prove which blocks were staged and re-encoded and what a
host call uploads."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import _special_chunks as SC
import _trunc as T
import _window_writes_masked as M
import _window_writes_strided as S
from _window_writes import BLOSCLZ, LZ4, ZSTD
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from cimg import synth

CANARY = 0x5A
WM_CONST, WM_MASK = M.WM_CONST, M.WM_MASK


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
    return M.build_emu(tmp_path_factory.mktemp("window_write_masked_emu"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def update(L, p, chunks, specs, src, masks, destsize, host=False, masked=True, words=0):
    """-> (rc, status, new chunks (bytes, or None where untouched), new_cbytes, stats, canaries intact).  masked=False: the strided
    call over the specs' strided fields.  words: what status and new_cbytes hold before the call."""
    buf, off, cs = concat(chunks)
    before = buf.copy()
    nb, bs = sizes(chunks)
    n = len(chunks)
    ds = np.asarray(destsize, np.int32)
    st = np.full(n, words, np.int32)
    ncb = np.full(n, words, np.int32)
    w = M.mwindows(specs) if masked else S.swindows(M.strided_of(specs))
    intact = True
    if host:
        ptrs = (C.c_void_p * n)()
        if masked:
            rc = L.wwmemu_update_host(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(ds), len(specs), w, _p(src), _p(masks), ptrs, _p(ncb), _p(st))
        else:
            rc = L.wwsemu_update_host(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(ds), len(specs), w, _p(src), ptrs, _p(ncb), _p(st))
        new = []
        for i in range(n):
            new.append(C.string_at(ptrs[i], int(ncb[i])) if ptrs[i] else None)
            if ptrs[i]:
                L.wwemu_free(ptrs[i])
    else:
        new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
        nbuf = np.full(int(new_off[-1]) + int(ds[-1]) + 64, CANARY, np.uint8)
        if masked:
            rc = L.wwmemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), w, _p(src), _p(masks),
                                        _p(nbuf), _p(new_off), _p(ncb), _p(st))
        else:
            rc = L.wwsemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), w, _p(src), _p(nbuf),
                                        _p(new_off), _p(ncb), _p(st))
        new = [nbuf[o:o + c].tobytes() if 0 < c != words else None for o, c in zip(new_off, ncb)]
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
def test_matrix_in_every_form_matches_oracle(L, codec, ts, filt, split):
    """every window of the strided matrix as an array, a constant, a masked array and a masked constant -- each form in a call of its
    own and the four mixed in one call -- in the three write orders; the host call in ascending order"""
    po, chunks, ds = case(ts, codec, filt, split)
    nb, bs = sizes(chunks)
    try:
        for form in ("array", "const", "array_masked", "const_masked", "mixed"):
            specs, src, masks = M.dress(S.matrix_windows(ts), form, ts, mask="cycle", seed=3)
            want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
            blocks = len(S.touched_blocks(specs, nb, bs, ts))
            for order, host in ((0, False), (1, False), (2, False), (0, True)):
                L.emu_set_write_order(order)
                rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 8192, codec, split, filt), chunks, specs, src, masks, ds, host=host)
                assert rc == 0 and not st.any(), (form, order, host, rc, st)
                for i, (a, b) in enumerate(zip(new, want)):
                    assert a == b, (form, order, host, i, None if a is None else len(a), None if b is None else len(b))
                if stats[2] == 0:                       # (chunks that come out memcpyed are recompressed whole)
                    assert stats[1] == blocks, (form, stats, blocks)
    finally:
        L.emu_set_write_order(0)


@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("kind", M.MASKS)
def test_every_mask_kind(L, ts, kind):
    """all ones, all zeros, a checkerboard, exactly one element, random 50 %, the values 2 and 255, runs of 1, 2 and 3 set bytes at
    every alignment: dense rows from odd origins and strided rows, arrays and constants, mask rows at odd offsets"""
    if ts == 8:
        po = ocp(8)
        chunks = oracle_chunks(po, pixels(8, 4000), 4000 * 8)
        ds = [4000 * 8 + 32]
        wins = [S.win(37, 61, 9, row_pitch=97, nchunks=1), S.win(1001, 30, 5, row_pitch=200, col_pitch=3, nchunks=1)]
    else:
        po, chunks, ds = case(ts)
        R = S.ROW
        wins = [S.win(R * 3 + 1, 67, 9), S.win(R * 14 + 2, 66, 9), S.win(R * 25 + 3, 65, 9), S.win(R * 36 + 4, 64, 9),     # dense, every start alignment
                S.win(R * 47 + 1, 25, 7, col_pitch=3), S.win(S.CHUNK_ELEMS - 2 * R - 17, 29, 6),                       # strided; over the chunk boundary
                S.win(8192 // ts - 40, 90, 1)]                                                                          # over a block boundary
    for form in ("array_masked", "const_masked"):
        specs, src, masks = M.dress(wins, form, ts, mask=kind, seed=11)
        want, edited = M.expected(po, chunks, specs, ts, src, masks, ds)
        for host in (False, True):
            rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, masks, ds, host=host)
            assert rc == 0 and new == want, (form, host, rc)
        if kind == "zeros":                              # the old chunks, byte for byte
            assert [c for c in new if c is not None] == [c for c, w in zip(chunks, want) if w is not None]
        if kind == "one":
            old = np.concatenate([O.decompress(c)[1] for c in chunks])
            assert (old != edited[0]).reshape(-1, ts).any(axis=1).sum() <= len(specs)


def test_flags_0_equals_the_strided_call(L):
    for ts, codec in ((1, LZ4), (3, BLOSCLZ), (4, LZ4)):
        po, chunks, ds = case(ts, codec)
        specs, src, masks = M.dress(S.matrix_windows(ts), "array", ts)
        p = cp(ts, 5, 8192, codec)
        for dsz in (ds, [len(c) + 8 for c in chunks]):   # a tight destsize too: the hand-back to the whole route
            for host in (False, True):
                a = update(L, p, chunks, specs, src, None, dsz, host=host, masked=False)
                b = update(L, p, chunks, specs, src, None, dsz, host=host, masked=True)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), (ts, host, a[0], b[0])
                assert np.array_equal(a[4], b[4]), (ts, host, a[4], b[4])


def test_constant_fill_of_whole_blocks_is_not_staged_and_uploads_only_chunks(L):
    """a constant unmasked col_pitch 1 window over blocks 1 and 2 of chunk 0 and a few elements more: the two whole blocks are not
    staged, the host call uploads the touched chunk and nothing else; the same window with a mask stages them again and uploads
    the mask"""
    ts = 2
    po, chunks, ds = case(ts)
    epb = 8192 // ts
    w = S.win(epb - 10, 2 * epb + 30, 1)                 # blocks 0 (tail), 1, 2 (whole), 3 (head)
    for form, decoded in (("const", 2), ("const_masked", 4), ("array", 2), ("array_masked", 4)):
        specs, src, masks = M.dress([w], form, ts, mask="checker")
        want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
        for host in (False, True):
            rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, masks, ds, host=host)
            assert rc == 0 and new == want and new[1] is None and new[2] is None, (form, host)
            assert stats[0] == decoded and stats[1] == 4 and stats[2] == 0, (form, host, stats)
            if host:
                n = w["width"]
                up = len(chunks[0]) + (0 if "const" in form else n * ts) + (n if "masked" in form else 0)
                assert stats[3] == up, (form, stats, up)


def test_a_masked_window_over_an_earlier_one_wins_only_where_its_mask_is_set(L):
    ts = 1
    po, chunks, ds = case(ts)
    R = S.ROW
    for first, second in (("array", "const_masked"), ("const", "array_masked"), ("array_masked", "array_masked")):
        a, sa, ma = M.dress([S.win(R * 5 + 3, 100, 20)], first, ts, mask="random", seed=5)
        b, sb, mb = M.dress([S.win(R * 9 + 31, 100, 20)], second, ts, mask="checker", seed=6)
        # one source and one mask buffer for the call
        b[0]["out_off"] += sa.size
        b[0]["mask_off"] += ma.size + (ma.size & 1)
        src = np.concatenate([sa, sb])
        masks = np.concatenate([ma, np.zeros(ma.size & 1, np.uint8), mb])
        specs = a + b
        want, edited = M.expected(po, chunks, specs, ts, src, masks, ds)
        only_a, _ = M.expected(po, chunks, a, ts, src, masks, ds)
        assert want != only_a
        try:
            for order in (0, 1, 2):
                L.emu_set_write_order(order)
                for host in (False, True):
                    rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, masks, ds, host=host)
                    assert rc == 0 and new == want, (first, second, order, host)
                    assert schedule(L)[0] == 0               # (overlapping windows: the ordered schedule)
        finally:
            L.emu_set_write_order(0)


@pytest.mark.parametrize("kind", ["columns", "rows", "tiles"])
def test_windows_that_share_every_dword(L, kind):
    """the GPU suite's read-modify-write case on the emulator (which cannot show the race: here it pins the bytes and the schedule)"""
    ts = 1
    po = ocp(ts)
    chunks = oracle_chunks(po, pixels(ts, 8192), 8192)
    ds = [8192 + 32]
    try:
        for form in ("array_masked", "const_masked", "mixed"):
            specs, src, masks = M.dress(M.rmw_windows(kind), form, ts, mask="checker", seed=2)
            want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
            for order in (0, 1, 2):
                L.emu_set_write_order(order)
                rc, st, new, ncb, stats, _ = update(L, cp(ts), chunks, specs, src, masks, ds)
                assert rc == 0 and new == want, (kind, form, order)
                # interleaved columns: the proof counts the bytes between samples as written, so the unit is ordered; alternating
                # rows: disjoint (the unit runs once more, in the same schedule, if the splice hands the chunk to the whole route)
                d, o = schedule(L)
                assert (d == 0 and o >= 1) if kind == "columns" else (o == 0 and d >= 1), (kind, d, o)
    finally:
        L.emu_set_write_order(0)


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
    """zstd chunks, a chunk of 128 KiB blocks and memcpyed (clevel 0) chunks: equal to the emulated engine's own compress of the
    edited pixels, and the pixels equal to numpy's"""
    ts = 4
    chunk_elems = 40000 if bs > 8192 else S.CHUNK_ELEMS              # (a chunk holds a 128 KiB block and a leftover)
    elems = 2 * chunk_elems + 5001
    raw = pixels(ts, elems)
    p = cp(ts, clevel, bs, codec)
    comp = emu_compress(L, p)
    cb = chunk_elems * ts
    chunks = [comp(raw[o:o + cb], min(cb, raw.size - o) + 32) for o in range(0, raw.size, cb)]
    ds = [min(cb, raw.size - o) + 32 for o in range(0, raw.size, cb)]
    specs, src, masks = M.dress(S.matrix_windows(ts, elems=elems, chunk_elems=chunk_elems), "mixed", ts, mask="cycle")
    want, _ = M.expected(None, chunks, specs, ts, src, masks, ds, compress=comp, planes={0: raw})
    try:
        for order in (0, 1, 2):                          # (`want` was made in ascending order: the chunks are the same in every order)
            L.emu_set_write_order(order)
            for host in (False, True):
                rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, masks, ds, host=host)
                assert rc == 0 and new == want, (codec, bs, clevel, host, order)
                if codec == ZSTD or clevel == 0:
                    assert stats[2] == 3 and stats[1] == 0, stats
    finally:
        L.emu_set_write_order(0)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_special_zero_and_repeated_value_chunks(L, host):
    chunks, plane = SC.six_chunks()                      # regular, value, nan, zero, memcpyed, uninit: 256 x 96 float32, 16 rows a chunk
    p = SC.plane_params()
    ts, PW = SC.TS, SC.PW
    wins = [S.win(20 * PW + 31, 40, 15, row_pitch=3 * PW, col_pitch=5, nchunks=6), S.win(50 * PW + 1, 30, 4, row_pitch=PW, nchunks=6),
            S.win(24 * PW + 3, 50, 3, row_pitch=PW, nchunks=6), S.win(66 * PW + 5, 40, 6, row_pitch=PW, nchunks=6)]
    specs, src, masks = M.dress(wins, "mixed", ts, mask="random", seed=4)
    ds = [SC.CHUNK + 32] * 6
    want, edited = M.expected(p, chunks, specs, ts, src, masks, ds, planes={0: np.ascontiguousarray(plane).view(np.uint8).ravel()})
    rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 4096), chunks, specs, src, masks, ds, host=host)
    assert rc == 0 and not st.any(), (rc, st)
    assert [c is not None for c in new] == [False, True, True, True, True, False]
    assert new == want
    after = [c if c is not None else old for c, old in zip(new, chunks)]
    assert np.array_equal(np.concatenate([SC.want(c) for c in after]), edited[0])


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_trunc_prec_truncates_the_constant(L, host):
    """float32, 12 mantissa bits kept: a constant comes back truncated like any written pixel"""
    ts, m = 4, 12
    t = T.trunc(T.pixels("tiled", np.float32, 512, 48), ts, m)
    po = T.oracle_cparams(ts, m, clevel=5, blocksize=8192)
    chunks = oracle_chunks(po, t, 32768)
    ds = [32768 + 32] * len(chunks)
    n = len(chunks)
    wins = [S.win(512 * 5 + 3, 100, 10, row_pitch=3 * 512, col_pitch=5, nchunks=n), S.win(512 * 20 + 9, 64, 4, row_pitch=512, nchunks=n)]
    specs, src, masks = M.dress(wins, "const_masked", ts, mask="checker")
    value = np.array([1.2345678], np.float32)
    for s in specs:
        s["value"] = value.tobytes()
    specs[1]["flags"] = WM_CONST
    want, edited = M.expected(None, chunks, specs, ts, src, masks, ds, compress=lambda raw, d: O.compress(po, T.trunc(raw, ts, m), destsize=d)[1])
    rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 8192, trunc=m), chunks, specs, src, masks, ds, host=host)
    assert rc == 0 and new == want and stats[2] == 0 and stats[1] > 0, (rc, stats)
    got = O.decompress(next(c for c in new if c is not None))[1].view(np.float32)
    tv = T.trunc(value.view(np.uint8), ts, m).view(np.float32)[0]
    assert tv != value[0] and (got == tv).any() and not (got == value[0]).any()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_refusals_leave_status_and_new_cbytes_untouched(L, host):
    ts = 2
    po, chunks, ds = case(ts)
    src = np.zeros(1 << 16, np.uint8)
    masks = np.ones(1 << 16, np.uint8)
    ok = dict(S.win(11, 20, 5, row_pitch=100, col_pitch=3), out_off=0, out_pitch=20 * ts, mask_off=0, mask_pitch=20, flags=WM_MASK, value=b"")
    W = M.WORD
    bad = [(dict(ok, flags=4), src, masks), (dict(ok, flags=WM_MASK | 8), src, masks), (dict(ok, flags=-1), src, masks),
           (dict(ok, mask_pitch=19), src, masks), (dict(ok, mask_off=-1), src, masks), (dict(ok, mask_pitch=-1, height=1), src, masks),
           (ok, src, None), (ok, None, masks), (dict(ok, flags=0), None, None)]
    for b, s_, m_ in bad:
        rc, st, new, ncb, _, intact = update(L, cp(ts), chunks, [b], s_, m_, ds, host=host, words=W)
        assert rc == ERR_INVALID_PARAM and intact and (st == W).all() and (ncb == W).all(), (b, st, ncb)
    # a constant needs typesize <= 8
    p16 = cp(16)
    rc, st, new, ncb, _, intact = update(L, p16, chunks, [dict(ok, flags=WM_CONST)], src, masks, ds, host=host, words=W)
    assert rc == ERR_INVALID_PARAM and intact and (st == W).all() and (ncb == W).all()
    # the strided call's refusals stay (status and new_cbytes are zeroed there, as there)
    for b in (dict(ok, col_pitch=0), dict(ok, row_pitch=57), dict(ok, origin=S.ELEMS - 57), dict(ok, out_pitch=20 * ts - 1), dict(ok, chunk_count=0)):
        rc, st, new, ncb, _, intact = update(L, cp(ts), chunks, [b], src, masks, ds, host=host)
        assert rc == ERR_INVALID_PARAM and intact and all(x is None for x in new) and not ncb.any(), b
    # what is ignored: out_pitch of a constant window, the mask fields of an unmasked one, NULL pointers nobody needs
    good = [dict(ok, flags=WM_CONST, out_pitch=-5, out_off=-9, mask_off=-3, mask_pitch=-1, value=b"\x07\x09")]
    want, _ = M.expected(po, chunks, good, ts, None, None, ds)
    rc, st, new, ncb, _, _ = update(L, cp(ts), chunks, good, None, None, ds, host=host)
    assert rc == 0 and new == want
    # one row: any mask_pitch
    one = [dict(ok, height=1, mask_pitch=0)]
    want, _ = M.expected(po, chunks, one, ts, src, masks, ds)
    rc, st, new, ncb, _, _ = update(L, cp(ts), chunks, one, src, masks, ds, host=host)
    assert rc == 0 and new == want


def test_under_sanitizers(tmp_path):
    """planner, proofs and kernel body once more as a stand-alone ASan / UBSan program (tests/emu/window_write_masked_asan_main.cpp):
    every buffer an allocation of its exact size, LDS with zero slack, in the three write orders"""
    exe = M.build_emu(tmp_path, sanitize=True)
    for order in ("0", "1", "2"):
        r = subprocess.run([exe, order], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ok" in r.stdout
