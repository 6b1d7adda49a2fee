"""Masked and constant window writes on the MI355X: cimg_update_windows_masked_device / _host (csrc/update_plan.h over MaskedWindowSpec,
cimg_update_patch_masked in csrc/update_kernel.h).

New chunks must equal a from-scratch compress of the edited pixels -- np.copyto(view, src_or_value, where=mask) in call order into the
oracle's decode --: the oracle's bytes for lz4 and blosclz; for zstd the decoded pixels are compared, and the chunks with the
emulator's (tests/emu/window_write_masked_emu.cpp, built once for the module).  Canaries surround every new chunk.  The timing ids
show which patch kernel ran."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _window_writes_masked as M
import _window_writes_strided as S
from _window_writes import BLOSCLZ, LZ4, ZSTD
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from cimg import hip, synth

pytestmark = pytest.mark.gpu
CANARY = 0x5A
WM_CONST, WM_MASK = M.WM_CONST, M.WM_MASK


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return M.build_emu(tmp_path_factory.mktemp("window_write_masked_emu_gpu"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pixels(ts, elems, seed=0):
    rng = np.random.default_rng(seed)
    raw = synth.tiled_channel(np.float16, 64, max(elems * ts // 128 + 1, 1)).view(np.uint8).ravel()[:elems * ts].copy()
    raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)
    return raw


def run_device(eng, p, chunks, specs, src, masks, ds, words=0):
    """-> (rc, status, new chunks, new_cbytes, every byte of d_new outside the new chunks is still the canary)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    ds = np.asarray(ds, np.int32)
    n = len(chunks)
    new_off = 64 + np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64 + 64)[:-1]]).astype(np.int64)   # canaries around each
    total = int(new_off[-1]) + int(ds[-1]) + 64
    d_comp, d_new = eng.alloc(buf.size), eng.alloc(total)
    d_src = eng.alloc(src.size) if src is not None else None
    d_mask = eng.alloc(masks.size) if masks is not None else None
    d_comp.upload(buf)
    if d_src:
        d_src.upload(src)
    if d_mask:
        d_mask.upload(masks)
    d_new.upload(np.full(total, CANARY, np.uint8))
    st, ncb = np.full(n, words, np.int32), np.full(n, words, np.int32)
    rc, ncb, st = eng.update_windows_masked_device(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr if d_src else None,
                                                   d_mask.ptr if d_mask else None, d_new.ptr, new_off, comp_size=cs, check=False,
                                                   new_cbytes=ncb, status=st)
    out = d_new.download()
    back = d_comp.download()
    for b in (d_comp, d_new, d_src, d_mask):
        if b:
            b.free()
    assert np.array_equal(back, buf), "the input chunks were modified"
    new = [out[o:o + c].tobytes() if 0 < c != words else None for o, c in zip(new_off, ncb)]
    keep = np.ones(total, bool)
    if rc != ERR_INVALID_PARAM:                   # (a refused call writes nothing at all; any other only inside the chunks' capacities)
        for o, d in zip(new_off, ds):
            keep[o:o + d] = False
    return rc, st, new, ncb, bool((out[keep] == CANARY).all())


def both(eng, p, chunks, specs, src, masks, ds, words=0):
    rc, st, new, ncb, intact = run_device(eng, p, chunks, specs, src, masks, ds, words)
    assert intact, "bytes outside the new chunks were written"
    yield "device", rc, st, new, ncb, eng.update_stats()
    before = [bytes(c) for c in chunks]
    n = len(chunks)
    st, ncb = np.full(n, words, np.int32), np.full(n, words, np.int32)
    rc, new, st = eng.update_windows_masked_host(p, chunks, ds, specs, src, masks, check=False, new_cbytes=ncb, status=st)
    assert before == [bytes(c) for c in chunks], "the input chunks were modified"
    yield "host", rc, st, new, ncb, eng.update_stats()


def run_emu(L, p, chunks, specs, src, masks, ds):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    n = len(chunks)
    ds = np.asarray(ds, np.int32)
    st, ncb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    nbuf = np.zeros(int(new_off[-1]) + int(ds[-1]) + 64, np.uint8)
    rc = L.wwmemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), M.mwindows(specs), _p(src), _p(masks),
                                _p(nbuf), _p(new_off), _p(ncb), _p(st))
    return rc, [nbuf[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]


_cases = {}


def case(ts, codec=LZ4, filt=1, split=3, clevel=5):
    key = (ts, codec, filt, split, clevel)
    if key not in _cases:
        po = O.cparams(ts, clevel=clevel, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
        chunks = oracle_chunks(po, pixels(ts, S.ELEMS), S.CHUNK_ELEMS * ts)
        p = hip.cparams(ts, clevel=clevel, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
        _cases[key] = (po, p, chunks, [S.CHUNK_ELEMS * ts + 32] * len(chunks))
    return _cases[key]


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts,filt,split", S.MATRIX)
def test_matrix_in_every_form_matches_oracle_and_emulator(eng, L, codec, ts, filt, split):
    po, p, chunks, ds = case(ts, codec, filt, split)
    nb, bs = sizes(chunks)
    for form in ("array", "const", "array_masked", "const_masked", "mixed"):
        specs, src, masks = M.dress(S.matrix_windows(ts), form, ts, mask="cycle", seed=3)
        want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
        blocks = len(S.touched_blocks(specs, nb, bs, ts))
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, masks, ds):
            assert rc == 0 and not st.any(), (form, how, rc, st, eng.last_error())
            assert new == want, (form, how)
            if stats["chunks_whole"] == 0:
                assert stats["blocks_encoded"] == blocks, (form, how, stats, blocks)
        if form == "mixed":
            erc, enew = run_emu(L, p, chunks, specs, src, masks, ds)
            assert erc == 0 and enew == new


@pytest.mark.parametrize("ts", [1, 2, 8])
@pytest.mark.parametrize("kind", M.MASKS)
def test_every_mask_kind(eng, ts, kind):
    """dense rows from every start alignment under every mask kind (mask rows at odd offsets), arrays and constants"""
    if ts == 8:
        po = O.cparams(8, clevel=5, blocksize=8192)
        p = hip.cparams(8, clevel=5, blocksize=8192)
        chunks = oracle_chunks(po, pixels(8, 4000), 4000 * 8)
        ds = [4000 * 8 + 32]
        wins = [S.win(37, 61, 9, row_pitch=97, nchunks=1), S.win(1001, 30, 5, row_pitch=200, col_pitch=3, nchunks=1)]
    else:
        po, p, chunks, ds = case(ts)
        R = S.ROW
        wins = [S.win(R * 3 + 1, 67, 9), S.win(R * 14 + 2, 66, 9), S.win(R * 25 + 3, 65, 9), S.win(R * 36 + 4, 64, 9),
                S.win(R * 47 + 1, 25, 7, col_pitch=3), S.win(S.CHUNK_ELEMS - 2 * R - 17, 29, 6), S.win(8192 // ts - 40, 90, 1)]
    for form in ("array_masked", "const_masked"):
        specs, src, masks = M.dress(wins, form, ts, mask=kind, seed=11)
        want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, masks, ds):
            assert rc == 0 and new == want, (form, how, rc, eng.last_error())
            if kind == "zeros":
                assert [c for c in new if c is not None] == [c for c, w in zip(chunks, want) if w is not None]


@pytest.mark.parametrize("kind", ["columns", "rows", "tiles"])
def test_windows_that_share_every_dword(eng, kind):
    """THE READ-MODIFY-WRITE CASE.  A uint8 plane of one 8 KiB block; two masked windows on even and odd columns (col_pitch 2, origins 1
    apart: the planner's conservative proof runs this unit ORDERED, so the sharing there is between lanes, not between unsynchronised
    waves), two col_pitch 1 windows of odd width on alternating rows (the disjoint schedule: four waves, no barrier, shared dwords at
    the row ends), or 50 windows 3 bytes wide side by side (the disjoint schedule with EVERY dword shared by two waves), all under
    checkerboard and run masks: lanes and waves write neighbouring bytes of the same dwords, and an overlay that merged old and new bytes
    into a dword before storing it would lose some of them.  The result must equal numpy's."""
    ts = 1
    po = O.cparams(ts, clevel=5, blocksize=8192)
    p = hip.cparams(ts, clevel=5, blocksize=8192)
    chunks = oracle_chunks(po, pixels(ts, 8192), 8192)
    ds = [8192 + 32]
    for form in ("array_masked", "const_masked", "mixed"):
        for mask in ("checker", "runs"):
            specs, src, masks = M.dress(M.rmw_windows(kind), form, ts, mask=mask, seed=2)
            want, _ = M.expected(po, chunks, specs, ts, src, masks, ds)
            for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, masks, ds):
                assert rc == 0 and new == want, (kind, form, mask, how, rc, eng.last_error())


def test_constant_fill_of_whole_blocks_is_not_staged_and_uploads_only_chunks(eng):
    ts = 2
    po, p, chunks, ds = case(ts)
    epb = 8192 // ts
    w = S.win(epb - 10, 2 * epb + 30, 1)                 # blocks 0 (tail), 1, 2 (whole), 3 (head)
    for form, decoded in (("const", 2), ("const_masked", 4)):
        specs, src, masks = M.dress([w], form, ts, mask="checker")
        want, _ = M.expected(po, chunks, specs, ts, None, masks, ds)
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, None, masks if "masked" in form else None, ds):
            assert rc == 0 and new == want, (form, how, rc, eng.last_error())
            assert stats["blocks_decoded"] == decoded and stats["blocks_encoded"] == 4 and stats["chunks_whole"] == 0, (form, how, stats)
            if how == "host":
                assert stats["bytes_uploaded"] == len(chunks[0]) + (w["width"] if "masked" in form else 0), (form, stats)


def test_flags_0_equals_the_strided_call(eng):
    ts = 3
    po, p, chunks, ds = case(ts, BLOSCLZ)
    specs, src, _ = M.dress(S.matrix_windows(ts), "array", ts)
    for dsz in (ds, [len(c) + 8 for c in chunks]):
        a = list(both(eng, p, chunks, specs, src, None, dsz))
        buf, off, cs = concat(chunks)
        nb, bs = sizes(chunks)
        d_comp, d_src = eng.alloc(buf.size), eng.alloc(src.size)
        new_off = np.concatenate([[0], np.cumsum((np.asarray(dsz, np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
        d_new = eng.alloc(int(new_off[-1]) + int(dsz[-1]) + 64)
        d_comp.upload(buf)
        d_src.upload(src)
        rc, ncb, st = eng.update_windows_strided_device(p, d_comp.ptr, off, nb, bs, dsz, M.strided_of(specs), d_src.ptr, d_new.ptr, new_off, comp_size=cs,
                                                        check=False)
        out = d_new.download()
        sstats = eng.update_stats()
        d_comp.free(); d_src.free(); d_new.free()
        snew = [out[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]
        how, mrc, mst, mnew, mncb, mstats = a[0]
        assert (rc, snew, sstats) == (mrc, mnew, mstats) and np.array_equal(st, mst) and np.array_equal(ncb, mncb)
        hrc, hnew, hst = eng.update_windows_strided_host(p, chunks, dsz, M.strided_of(specs), src, check=False)
        assert (hrc, hnew, eng.update_stats()) == (a[1][1], a[1][3], a[1][5]) and np.array_equal(hst, a[1][2])


def test_zstd_chunks_pixels_and_the_emulators_chunks(eng, L):
    ts = 4
    raw = pixels(ts, S.ELEMS)
    p = hip.cparams(ts, clevel=5, blocksize=8192, compcode=ZSTD)
    cb = S.CHUNK_ELEMS * ts
    nbl = [min(cb, raw.size - o) for o in range(0, raw.size, cb)]
    ds = [n + 32 for n in nbl]
    chunks = eng.compress_host(p, raw, nbl, ds)
    specs, src, masks = M.dress(S.matrix_windows(ts), "mixed", ts, mask="cycle")
    edited = M.apply({0: raw}, specs, ts, src, masks)[0]
    erc, enew = run_emu(L, p, chunks, specs, src, masks, ds)
    assert erc == 0
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, masks, ds):
        assert rc == 0 and not st.any(), (how, rc, eng.last_error())
        assert stats["chunks_whole"] == 3
        # (the oracle decodes zstd where it finds a libzstd; else the engine's batch decode, which this feature does not touch)
        got = np.concatenate([O.decompress(c)[1] for c in new] if O.zstd_available() else eng.decompress_host(new)[0])
        assert np.array_equal(got, edited), how
        assert new == enew, how


def launches(eng, kid):
    return eng.kernel_time(kid)[1]


def test_each_call_launches_its_own_patch_kernel(eng):
    """the four existing write calls launch their own patch kernel and never the masked one; the masked calls launch it and none of
    the other three"""
    ts = 2
    po, p, chunks, ds = case(ts)
    specs, src, masks = M.dress(S.matrix_windows(ts), "mixed", ts)
    plain = [dict(S.win(S.ROW * 5 + 3, 40, 6)), dict(S.win(S.ROW * 30, 90, 2))]
    sspecs, ssrc = S.source(plain, ts)
    pspecs = S.without_col_pitch(sspecs)
    # (a typed source is aligned on its type: rows of its own inside the same buffer)
    tspecs = [dict(s, out_off=1024 * k, out_pitch=s["width"] * ts, elem_pitch=ts, src_type=hip.T_U16, out_type=hip.T_U16, scale=1.0, offset=0.0)
              for k, s in enumerate(sspecs)]
    ssrc = np.concatenate([ssrc, np.zeros(4096, np.uint8)])
    kinds = (hip.K_UPDATE_PATCH, hip.K_UPDATE_PATCH_STRIDED, hip.K_UPDATE_PATCH_TYPED, hip.K_UPDATE_PATCH_MASKED)
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    new_off = np.concatenate([[0], np.cumsum((np.asarray(ds, np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    d_comp, d_src, d_new = eng.alloc(buf.size), eng.alloc(ssrc.size), eng.alloc(int(new_off[-1]) + int(ds[-1]) + 64)
    d_comp.upload(buf)
    d_src.upload(ssrc)
    eng.enable_timing(1)
    try:
        eng.update_windows_host(p, chunks, ds, pspecs, ssrc)                  # (timing takes hold at the first batch step after it is enabled)
        calls = [(lambda: eng.update_windows_device(p, d_comp.ptr, off, nb, bs, ds, pspecs, d_src.ptr, d_new.ptr, new_off, comp_size=cs), 0),
                 (lambda: eng.update_windows_host(p, chunks, ds, pspecs, ssrc), 0),
                 (lambda: eng.update_windows_strided_device(p, d_comp.ptr, off, nb, bs, ds, sspecs, d_src.ptr, d_new.ptr, new_off, comp_size=cs), 1),
                 (lambda: eng.update_windows_strided_host(p, chunks, ds, sspecs, ssrc), 1),
                 (lambda: eng.update_windows_typed_device(p, d_comp.ptr, off, nb, bs, ds, tspecs, d_src.ptr, d_new.ptr, new_off, comp_size=cs), 2),
                 (lambda: list(both(eng, p, chunks, specs, src, masks, ds)), 3)]
        for call, which in calls:
            eng.reset_timing()
            call()
            got = [launches(eng, k) for k in kinds]
            assert [g > 0 for g in got] == [i == which for i in range(4)], (which, got)
            assert got[which] == (2 if which == 3 else 1), (which, got)
    finally:
        eng.enable_timing(0)
        eng.reset_timing()
        d_comp.free(); d_src.free(); d_new.free()
    assert hip.K_UPDATE_PATCH_MASKED == 29 and hip.KERNELS[29] == "cimg_update_patch_masked"
    assert hip.load().cimg_kernel_name(29).decode() == "cimg_update_patch_masked"


def test_refusals_leave_status_and_new_cbytes_untouched(eng):
    ts = 2
    po, p, chunks, ds = case(ts)
    src = np.zeros(1 << 16, np.uint8)
    masks = np.ones(1 << 16, np.uint8)
    ok = dict(S.win(11, 20, 5, row_pitch=100, col_pitch=3), out_off=0, out_pitch=20 * ts, mask_off=0, mask_pitch=20, flags=WM_MASK, value=b"")
    W = M.WORD
    bad = [(dict(ok, flags=4), src, masks), (dict(ok, flags=WM_MASK | 8), src, masks), (dict(ok, mask_pitch=19), src, masks),
           (dict(ok, mask_off=-1), src, masks), (dict(ok, mask_pitch=-1, height=1), src, masks), (ok, src, None), (ok, None, masks),
           (dict(ok, flags=0), None, None)]
    for b, s_, m_ in bad:
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, [b], s_, m_, ds, words=W):
            assert rc == ERR_INVALID_PARAM and (st == W).all() and (np.asarray(ncb) == W).all(), (how, b, st, ncb)
    for how, rc, st, new, ncb, stats in both(eng, hip.cparams(16, clevel=5, blocksize=8192), chunks, [dict(ok, flags=WM_CONST)], src, masks, ds, words=W):
        assert rc == ERR_INVALID_PARAM and (st == W).all() and (np.asarray(ncb) == W).all(), how
    # the strided call's refusals stay
    for b in (dict(ok, col_pitch=0), dict(ok, row_pitch=57), dict(ok, out_pitch=20 * ts - 1), dict(ok, chunk_count=0)):
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, [b], src, masks, ds):
            assert rc == ERR_INVALID_PARAM and all(x is None for x in new), (how, b)
    # the engine stays usable: a constant window with no source and no mask
    good = [dict(ok, flags=WM_CONST, out_pitch=-5, out_off=-9, mask_off=-3, mask_pitch=-1, value=b"\x07\x09")]
    want, _ = M.expected(po, chunks, good, ts, None, None, ds)
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, good, None, None, ds):
        assert rc == 0 and new == want, (how, rc, eng.last_error())
