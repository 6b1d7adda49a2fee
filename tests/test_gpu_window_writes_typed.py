"""Typed window writes on the MI355X: cimg_update_windows_typed_device (csrc/update_plan.h over TypedWindowSpec, cimg_update_patch_typed
in csrc/update_kernel.h, the conversion helpers of csrc/window_kernel.h).

The same checks as tests/test_emu_window_writes_typed.py through libcimg_hip.so, on a trimmed set: pixels are numpy's conversion of
the source tables (ties, saturation, NaN, subnormals), assigned into the oracle's decode in call order; every call's new chunks are
checked in the two steps _window_writes_typed.check_new describes; for integer planes -- where no NaN leaves its bits open -- the
new chunks also equal the emulator's, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _special_chunks as SC
import _trunc as TR
import _window_writes_strided as S
import _window_writes_typed as WT
import _windows_grouped as G
import _windows_typed as T
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from _windows_grouped import BLOSCLZ, LZ4, ZSTD, H, W, rect
from _windows_typed import F16, F32, I16, U8, U16
from cimg import hip

pytestmark = pytest.mark.gpu
CANARY = 0x5A


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return WT.build_emu(tmp_path_factory.mktemp("window_write_typed_emu_gpu"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_device(eng, p, chunks, specs, src, ds, typed=True, nbytes=None, blocksize=None, src_shift=0):
    """-> (rc, status, new chunks, new_cbytes, stats, d_new / new_cbytes / status all left alone); every byte of d_new outside the new
    chunks' capacities must still be the canary"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    ds = np.asarray(ds, np.int32)
    n = len(chunks)
    new_off = 64 + np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64 + 64)[:-1]]).astype(np.int64)   # canaries around each
    total = int(new_off[-1]) + int(ds[-1]) + 64
    d_comp, d_src, d_new = eng.alloc(buf.size), eng.alloc(src.size + 64), eng.alloc(total)
    d_comp.upload(buf)
    d_src.upload(src, offset=src_shift)
    d_new.upload(np.full(total, CANARY, np.uint8))
    st, ncb = np.full(n, WT.WORD, np.int32), np.full(n, WT.WORD, np.int32)
    if typed:
        rc, ncb, st = eng.update_windows_typed_device(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr + src_shift, d_new.ptr, new_off, comp_size=cs,
                                                      check=False, new_cbytes=ncb, status=st)
    else:
        rc, ncb, st = eng.update_windows_strided_device(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr, d_new.ptr, new_off, comp_size=cs, check=False)
    stats = eng.update_stats()
    out = d_new.download()
    back = d_comp.download()
    d_comp.free(); d_src.free(); d_new.free()
    assert np.array_equal(back, buf), "the input chunks were modified"
    alone = bool((out == CANARY).all() and (ncb == WT.WORD).all() and (st == WT.WORD).all())
    new = [out[o:o + c].tobytes() if 0 < c != WT.WORD else None for o, c in zip(new_off, ncb)]
    keep = np.ones(total, bool)
    if rc != ERR_INVALID_PARAM:
        for o, d in zip(new_off, ds):
            keep[o:o + d] = False
    assert (out[keep] == CANARY).all(), "bytes outside the new chunks were written"
    return rc, st, new, ncb, stats, alone


def run_emu(L, p, chunks, specs, src, ds):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    n = len(chunks)
    ds = np.asarray(ds, np.int32)
    q = G.EmuCParams()
    q.typesize, q.clevel, q.blocksize, q.compcode, q.splitmode = p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode
    for k in range(6):
        q.filters[k], q.filters_meta[k] = p.filters[k], p.filters_meta[k]
    st, ncb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    nbuf = np.zeros(int(new_off[-1]) + int(ds[-1]) + 64, np.uint8)
    held = np.concatenate([src, np.zeros(16, np.uint8)])
    rc = L.wwtemu_update_device(C.byref(q), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), T.twindows(specs), _p(held), _p(nbuf),
                                _p(new_off), _p(ncb), _p(st))
    return rc, [nbuf[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]


_cases = {}


def case(stored, codec=LZ4, filt=1, clevel=5):
    key = (stored, codec, filt, clevel)
    if key not in _cases:
        ts = T.SIZE[stored]
        cbytes, bsize = G.GEOMETRY[ts]
        po = O.cparams(ts, clevel=clevel, blocksize=bsize, compcode=codec, splitmode=3, filters=(0, 0, 0, 0, 0, filt))
        chunks = oracle_chunks(po, T.raw_of(T.plane(stored)), cbytes)
        p = hip.cparams(ts, clevel=clevel, blocksize=bsize, compcode=codec, splitmode=3, filters=(0, 0, 0, 0, 0, filt))
        _cases[key] = (po, p, chunks, [len(O.decompress(c)[1]) + 32 for c in chunks])
    return _cases[key]


def shapes(n):
    return G.matrix_windows(n) + [rect(7, 3, 300, 100, 3, 2, nchunks=n), rect(2, 70, 400, 40, 2, 1, nchunks=n), rect(9, 100, 301, 9, 7, 3, nchunks=n)]


def test_kernel_name_and_one_launch_per_call(eng):
    assert hip.K_UPDATE_PATCH_TYPED == 28 and hip.KERNELS[28] == "cimg_update_patch_typed"
    assert hip.load().cimg_kernel_name(28).decode() == "cimg_update_patch_typed"
    po, p, chunks, ds = case(U8)
    specs, src, vals = WT.source(WT.dress(shapes(len(chunks))[:6], U8, F32))
    kinds = (hip.K_UPDATE_PATCH, hip.K_UPDATE_PATCH_STRIDED, hip.K_UPDATE_PATCH_TYPED)
    eng.enable_timing(1)
    try:
        run_device(eng, p, chunks, specs, src, ds)                        # (timing takes hold at the first batch step after it is enabled)
        eng.reset_timing()
        rc = run_device(eng, p, chunks, specs, src, ds)[0]
        assert rc == 0
        assert [eng.kernel_time(k)[1] for k in kinds] == [0, 0, 1]
        assert len(eng.kernel_samples(hip.K_UPDATE_PATCH_TYPED)) == 1
    finally:
        eng.enable_timing(0)
        eng.reset_timing()


@pytest.mark.parametrize("stored,mem", [(U8, F32), (U16, F32), (I16, F32), (F16, F32), (U8, F16)])
def test_tables_through_the_matrix_windows(eng, L, stored, mem):
    """tie, saturation, NaN and subnormal tables under every scale / offset pair; dense and strided windows, elem_pitch of 1, 3 and 4
    memory sizes, overlapping windows; GPU == numpy (two steps) and, for integer planes, GPU == emulator"""
    po, p, chunks, ds = case(stored)
    specs, src, vals = WT.source(WT.dress(shapes(len(chunks)), stored, mem, k0=stored))
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and not st.any(), (rc, st, eng.last_error())
    WT.check_new(po, chunks, specs, new, want, edited)
    nb, bs = sizes(chunks)
    assert stats["chunks_whole"] == 0 and stats["blocks_encoded"] == len(G.touched_blocks(specs, nb, bs, T.SIZE[stored]))
    if stored != F16:
        assert new == want
        erc, enew = run_emu(L, p, chunks, specs, src, ds)
        assert erc == 0 and enew == new


def test_a_division_not_a_reciprocal_multiply(eng):
    y, teeth = WT.division_teeth()
    assert teeth > 0
    po, p, chunks, ds = case(U16)
    specs, src, vals = WT.source([WT.typed(rect(0, 5, 512, 1, nchunks=len(chunks)), U16, F32, 1 / 255, 0.0)], tables=[y])
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0
    got = O.decompress(new[0])[1].view(np.uint16)[5 * W:6 * W]
    assert np.array_equal(got, np.rint(y / np.float32(1 / 255)).astype(np.uint16))


def test_disjoint_unit(eng, L):
    po, p, chunks, ds = case(U8)
    wins = [dict(w, chunk_count=len(chunks)) for w in S.disjoint_strided_unit(1, G.GEOMETRY[1][1])]
    specs, src, vals = WT.source(WT.dress(wins, U8, F32))
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and new == want and stats["blocks_encoded"] == 1
    assert run_emu(L, p, chunks, specs, src, ds)[1] == new


def test_pixel_major_source_of_three_planes(eng, L):
    vals0, chunks, n = T.three_planes()
    bsize = G.GEOMETRY[1][1]
    po = O.cparams(1, clevel=5, blocksize=bsize, splitmode=3)
    p = hip.cparams(1, clevel=5, blocksize=bsize, splitmode=3)
    ds = [len(O.decompress(c)[1]) + 32 for c in chunks]
    regions = [(10, 5, 200, 60, 1, 1), (100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5), (W - 1, H - 1, 1, 1, 1, 1), (0, 0, W, H, 2, 3)]
    specs, size = WT.pixel_major(regions, n, U8, F32, (1 / 255, 1 / (255 * 0.229), -0.5), (0.0, -0.485 / 0.229, 3.0))
    src, vals = WT.fill_pixel_major(specs, size)
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and not st.any() and new == want, (rc, eng.last_error())
    assert run_emu(L, p, chunks, specs, src, ds)[1] == new


def test_every_staging_mode(eng, L):
    """lz4 + bitshuffle and blosclz on the splice route, memcpyed chunks and zstd chunks on the whole route, then zero / value / NaN /
    uninit special chunks of a float32 plane"""
    for codec, filt, clevel in ((LZ4, 2, 5), (BLOSCLZ, 1, 5), (LZ4, 1, 0)):
        po, p, chunks, ds = case(U16, codec, filt, clevel)
        specs, src, vals = WT.source(WT.dress(shapes(len(chunks)), U16, F32, k0=1))
        want, edited = WT.expected(po, chunks, specs, vals, ds)
        rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
        assert rc == 0 and new == want, (codec, filt, clevel, rc, eng.last_error())
        assert (stats["chunks_whole"] == len(chunks)) == (clevel == 0)
        assert run_emu(L, p, chunks, specs, src, ds)[1] == new
    # zstd: no byte-exact oracle -- the engine's own compress of numpy's pixels, and a round trip through the engine's decode
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    p = hip.cparams(ts, clevel=5, blocksize=bsize, compcode=ZSTD)
    raw = T.raw_of(T.plane(I16))
    nb = [min(cbytes, raw.size - o) for o in range(0, raw.size, cbytes)]
    ds = [b + 32 for b in nb]
    chunks = eng.compress_host(p, raw, nb, ds)
    comp = lambda piece, d: eng.compress_host(p, np.ascontiguousarray(piece), [piece.size], [d])[0]     # noqa: E731
    specs, src, vals = WT.source(WT.dress(shapes(len(chunks)), I16, F32))
    want, edited = WT.expected(None, chunks, specs, vals, ds, compress=comp, planes={0: raw})
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and new == want and stats["chunks_whole"] == len(chunks)
    assert np.array_equal(np.concatenate([np.frombuffer(b, np.uint8) for b in eng.decompress_host(new)[0]]), edited[0])
    # special chunks
    chunks, plane = SC.six_chunks()
    po = SC.plane_params()
    PW = SC.PW
    wins = [S.win(3 * PW + 31, 40, 30, row_pitch=3 * PW, col_pitch=5, nchunks=6), S.win(50 * PW + 1, 1, 1, nchunks=6), S.win(64 * PW, PW, 32, row_pitch=PW, nchunks=6)]
    specs, src, vals = WT.source(WT.dress(wins, F32, F16))
    ds = [SC.CHUNK + 32] * 6
    want, edited = WT.expected(po, chunks, specs, vals, ds, planes={0: np.ascontiguousarray(plane).view(np.uint8).ravel()})
    rc, st, new, ncb, stats, _ = run_device(eng, hip.cparams(SC.TS, clevel=5, blocksize=4096), chunks, specs, src, ds)
    assert rc == 0 and not st.any() and all(c is not None for c in new), (rc, st, eng.last_error())
    WT.check_new(po, chunks, specs, new, want, edited)


def test_trunc_prec_applies_after_the_conversion(eng):
    ts, m = 4, 12
    t = TR.trunc(TR.pixels("tiled", np.float32, 512, 48), ts, m)
    po = TR.oracle_cparams(ts, m, clevel=5, blocksize=8192)
    chunks = oracle_chunks(po, t, 32768)
    ds = [32768 + 32] * len(chunks)
    n = len(chunks)
    wins = [S.win(512 * 5 + 3, 100, 10, row_pitch=3 * 512, col_pitch=5, nchunks=n), S.win(512 * 20 + 9, 64, 4, row_pitch=512, nchunks=n)]
    specs, src, vals = WT.source(WT.dress(wins, F32, F32, k0=1))
    want, edited = WT.expected(None, chunks, specs, vals, ds, compress=lambda raw, d: O.compress(po, TR.trunc(raw, ts, m), destsize=d)[1])
    edited = {k: TR.trunc(v, ts, m) for k, v in edited.items()}
    p = hip.cparams(ts, clevel=5, blocksize=8192, trunc_prec=m)
    rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and stats["chunks_whole"] == 0 and stats["blocks_encoded"] > 0, (rc, stats, eng.last_error())
    WT.check_new(po, chunks, specs, new, want, edited)


@pytest.mark.parametrize("stored", [U8, F32])
def test_identity_call_equals_the_strided_call(eng, stored):
    ts = T.SIZE[stored]
    po, p, chunks, ds = case(stored)
    specs, src, vals = WT.source([T.typed(r, stored, stored) for r in shapes(len(chunks))])
    plain = [{k: s[k] for k, _ in T.StridedWindow._fields_} for s in specs]
    for dsz in (ds, [len(c) + 8 for c in chunks]):
        a = run_device(eng, p, chunks, specs, src, dsz)
        b = run_device(eng, p, chunks, plain, src, dsz, typed=False)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4], (a[0], b[0], a[4], b[4])
    want, _ = WT.expected(po, chunks, specs, vals, ds)
    assert run_device(eng, p, chunks, specs, src, ds)[2] == want


def test_read_then_write_gives_the_old_chunks_back(eng):
    """a typed read to float32 and a typed write of what it gave, same scale and offset: every touched chunk comes back byte for
    byte, for pairs under which every uint8 returns to itself"""
    po, p, chunks, ds = case(U8)
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    n = len(chunks)
    for sc, of in ((1 / 255, 0.0), (1 / (255 * 0.229), -0.485 / 0.229), (1 / 255, -0.4851), (1 / 128, -1.0)):
        specs, size = T.pack_typed([T.typed(r, U8, F32, sc, of, pitch_mult=1 + k % 2) for k, r in enumerate(shapes(n)[:9])])
        d_comp, d_mem = eng.alloc(buf.size), eng.alloc(size)
        d_comp.upload(buf)
        eng.decompress_windows_typed_device(d_comp.ptr, off, nb, bs, 1, specs, d_mem.ptr, comp_size=cs)
        mem = d_mem.download()
        d_comp.free(); d_mem.free()
        rc, st, new, ncb, stats, _ = run_device(eng, p, chunks, specs, mem, ds)
        assert rc == 0 and sum(c is not None for c in new) >= 4 and all(c is None or c == old for c, old in zip(new, chunks)), (sc, of)


def test_refusals_leave_everything_alone(eng):
    ts = 2
    po, p, chunks, ds = case(U16)
    n = len(chunks)
    src = np.zeros(1 << 16, np.uint8)
    ok = dict(WT.typed(rect(10, 10, 80, 20, 4, 2, nchunks=n), U16, F32, 0.5, 1.0, pitch_mult=3), out_off=8, out_pitch=20 * 12)
    nan, inf = float("nan"), float("inf")
    bad = [dict(ok, scale=0.0), dict(ok, scale=nan), dict(ok, scale=-inf), dict(ok, offset=nan), dict(ok, offset=inf),
           dict(ok, elem_pitch=3), dict(ok, elem_pitch=6), dict(ok, out_pitch=19 * 12 + 3), dict(ok, out_pitch=242),
           dict(ok, src_type=9), dict(ok, out_type=-1), dict(ok, src_type=U8), dict(ok, out_type=U16), dict(ok, out_type=T.F64, elem_pitch=8, out_pitch=160),
           dict(ok, out_off=6), dict(ok, col_pitch=0), dict(ok, origin=-1), dict(ok, chunk_count=0)]
    for b in bad:
        rc, st, new, ncb, _, alone = run_device(eng, p, chunks, [ok, b], src, ds)
        assert rc == ERR_INVALID_PARAM and alone, (b, rc)
    rc, _, _, _, _, alone = run_device(eng, p, chunks, [ok], src, ds, src_shift=2)
    assert rc == ERR_INVALID_PARAM and alone
    nb, bs = sizes(chunks)
    rc, _, _, _, _, alone = run_device(eng, p, chunks, [ok], src, ds, nbytes=nb, blocksize=np.full(n, 4097, np.int32))
    assert rc == ERR_INVALID_PARAM and alone
    specs, src2, vals = WT.source([{k: v for k, v in ok.items() if k not in ("out_off", "out_pitch")}])
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    rc, st, new, ncb, _, _ = run_device(eng, p, chunks, specs, src2, ds)
    assert rc == 0 and new == want
