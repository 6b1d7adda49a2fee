"""Typed window writes (csrc/update_plan.h: check_typed_update and run_update over TypedWindowSpec; csrc/update_kernel.h:
TypedPatchBlock; the conversion helpers of csrc/window_kernel.h) on the host lane emulator.

tests/emu/window_write_typed_emu.cpp (which includes the strided and the plain write emulators: the strided call of the same
library is the identity comparison), emu.cpp and wide_emu.cpp are compiled into a library in a pytest temp directory
(_window_writes_typed.build_emu, -ffp-contract=off).  Pixels come from numpy's conversion of the source tables, chunk bytes from
the oracle's compress; every call's new chunks are checked in the two steps _window_writes_typed.check_new describes.  Planner and
kernel body run once more in a stand-alone AddressSanitizer / UBSan program (tests/emu/window_write_typed_asan_main.cpp)."""
import ctypes as C
import subprocess

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
from _windows_strided import swindows
from _windows_typed import F16, F32, F64, I8, I16, I32, U8, U16, U32

CANARY = 0x5A


def cp(ts, clevel=5, blocksize=8192, compcode=LZ4, splitmode=3, filt=1, trunc=None):
    p = G.EmuCParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    if trunc is not None:
        p.filters[4], p.filters_meta[4] = 4, trunc & 0xFF
    return p


def ocp(ts, clevel=5, blocksize=8192, compcode=LZ4, splitmode=3, filt=1):
    return O.cparams(ts, clevel=clevel, blocksize=blocksize, compcode=compcode, splitmode=splitmode, filters=(0, 0, 0, 0, 0, filt))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return WT.build_emu(tmp_path_factory.mktemp("window_write_typed_emu"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update(L, p, chunks, specs, src, destsize, typed=True, order=0, nbytes=None, blocksize=None, src_shift=0):
    """-> (rc, status, new chunks (bytes, or None where untouched), new_cbytes, stats, d_new / new_cbytes / status all left alone)"""
    buf, off, cs = concat(chunks)
    before = buf.copy()
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    n = len(chunks)
    ds = np.asarray(destsize, np.int32)
    st = np.full(n, WT.WORD, np.int32)
    ncb = np.full(n, WT.WORD, np.int32)
    new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    nbuf = np.full(int(new_off[-1]) + int(ds[-1]) + 64, CANARY, np.uint8)
    held = np.zeros(src.size + 16, np.uint8)                    # (a source that starts `src_shift` bytes past an aligned address)
    held[src_shift:src_shift + src.size] = src
    L.emu_set_write_order(order)
    try:
        if typed:
            rc = L.wwtemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), T.twindows(specs),
                                        held.ctypes.data + src_shift, _p(nbuf), _p(new_off), _p(ncb), _p(st))
        else:
            rc = L.wwsemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), swindows(specs),
                                        held.ctypes.data + src_shift, _p(nbuf), _p(new_off), _p(ncb), _p(st))
    finally:
        L.emu_set_write_order(0)
    assert np.array_equal(buf, before), "the input chunks were modified"
    alone = bool((nbuf == CANARY).all() and (ncb == WT.WORD).all() and (st == WT.WORD).all())
    new = [nbuf[o:o + c].tobytes() if 0 < c != WT.WORD else None for o, c in zip(new_off, ncb)]
    stats = np.zeros(4, np.int64)
    L.wwemu_update_stats(_p(stats))
    return rc, st, new, ncb, stats, alone


def schedule(L):
    out = np.zeros(2, np.int64)
    L.wwsemu_schedule_stats(_p(out))
    return int(out[0]), int(out[1])


_cases = {}


def case(stored, codec=LZ4, filt=1, clevel=5):
    """the W x H plane of T.plane(stored) as the oracle's chunks in the grouped geometry (shared, read-only)"""
    key = (stored, codec, filt, clevel)
    if key not in _cases:
        ts = T.SIZE[stored]
        cbytes, bsize = G.GEOMETRY[ts]
        po = ocp(ts, clevel=clevel, blocksize=bsize, compcode=codec, filt=filt)
        chunks = oracle_chunks(po, T.raw_of(T.plane(stored)), cbytes)
        _cases[key] = (po, cp(ts, clevel, bsize, codec, 3, filt), chunks, [len(O.decompress(c)[1]) + 32 for c in chunks])
    return _cases[key]


def shapes(n):
    """dense and strided windows (col_pitch 1, 2, 3, 7), overlapping ones, the whole plane in between, 1 x 1 and empty windows"""
    return G.matrix_windows(n) + [rect(7, 3, 300, 100, 3, 2, nchunks=n), rect(2, 70, 400, 40, 2, 1, nchunks=n), rect(9, 100, 301, 9, 7, 3, nchunks=n)]


def run_and_check(L, po, p, chunks, ds, specs, orders=(0,), **kw):
    specs, src, vals = WT.source(specs)
    want, edited = WT.expected(po, chunks, specs, vals, ds, **{k: v for k, v in kw.items() if k in ("compress", "planes")})
    for order in orders:
        rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds, order=order)
        assert rc == 0 and not st.any(), (order, rc, st)
        WT.check_new(po, chunks, specs, new, want, edited, decode=kw.get("decode"), compress=kw.get("check_compress"))
    return specs, src, new, stats


@pytest.mark.parametrize("mem", [F32, F16])
@pytest.mark.parametrize("stored", [U8, I8, U16, I16, U32, I32, F16, F32])
def test_every_stored_type(L, stored, mem):
    """the matrix windows over oracle chunks (lz4 + shuffle, several chunks, leftover blocks), every scale / offset pair, elem_pitch of
    1, 3 and 4 memory sizes, col_pitch 1, 2, 3 and 7; overlapping windows make ordered units"""
    po, p, chunks, ds = case(stored)
    run_and_check(L, po, p, chunks, ds, WT.dress(shapes(len(chunks)), stored, mem, k0=stored), orders=(0, 1, 2) if stored in (U8, F16) else (0,))
    assert schedule(L)[1] > 0


def test_a_division_not_a_reciprocal_multiply(L):
    """one row of half steps k / 2 * s, s = float32(1 / 255): 95 of the 512 elements round differently under y * 255"""
    y, teeth = WT.division_teeth()
    assert teeth > 0
    po, p, chunks, ds = case(U16)
    spec = WT.typed(rect(0, 5, 512, 1, nchunks=len(chunks)), U16, F32, 1 / 255, 0.0)
    specs, src, vals = WT.source([spec], tables=[y])
    assert np.array_equal(vals[0].ravel(), y)
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds)
    assert rc == 0 and new == want
    got = O.decompress(new[0])[1].view(np.uint16)[5 * W:6 * W]
    assert np.array_equal(got, np.rint(y / np.float32(1 / 255)).astype(np.uint16))


def test_float64_planes_take_the_identity(L):
    po, p, chunks, ds = case(F64)
    n = len(chunks)
    specs = [T.typed(r, F64, F64, pitch_mult=(1, 3)[k % 2]) for k, r in enumerate(shapes(n))]
    run_and_check(L, po, p, chunks, ds, specs, orders=(0, 1))
    ok = dict(T.typed(rect(3, 3, 20, 4, nchunks=n), F64, F32, 0.5, 0.0), out_off=0, out_pitch=80)
    rc, _, _, _, _, alone = update(L, p, chunks, [ok], np.zeros(4096, np.uint8), ds)
    assert rc == ERR_INVALID_PARAM and alone


@pytest.mark.parametrize("stored,mem", [(U8, F32), (U16, F16), (F16, F32), (F32, F32)])
def test_disjoint_units_run_round_robin_in_any_order(L, stored, mem):
    """interleaved windows that share no byte inside one block: the disjoint schedule, under all three wave orders"""
    ts = T.SIZE[stored]
    po, p, chunks, ds = case(stored)
    bsize = G.GEOMETRY[ts][1]
    wins = [dict(w, chunk_count=len(chunks)) for w in S.disjoint_strided_unit(ts, bsize)]
    specs, src, vals = WT.source(WT.dress(wins, stored, mem))
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    for order in (0, 1, 2):
        rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds, order=order)
        assert rc == 0 and schedule(L) == (1, 0), (order, schedule(L))
        assert stats[0] == 1 and stats[1] == 1
        WT.check_new(po, chunks, specs, new, want, edited)


def test_later_window_wins(L):
    po, p, chunks, ds = case(U8)
    n = len(chunks)
    wins = [WT.typed(rect(40, 40, 100, 20, nchunks=n), U8, F32, 1 / 255, 0.0), WT.typed(rect(60, 45, 100, 20, 2, 1, nchunks=n), U8, F16, -0.5, 3.0, 3),
            WT.typed(rect(60, 45, 30, 5, nchunks=n), U8, U8), WT.typed(rect(61, 46, 1, 1, nchunks=n), U8, F32, 1.0, 0.0)]
    specs, src, new, _ = run_and_check(L, po, p, chunks, ds, wins, orders=(0, 1, 2))
    assert schedule(L)[0] == 0 and schedule(L)[1] > 0
    px = np.concatenate([O.decompress(c if c is not None else o)[1] for c, o in zip(new, chunks)]).reshape(H, W)
    s = specs[-1]
    y = src[s["out_off"]:s["out_off"] + 4].view(np.float32)
    assert px[46, 61] == WT.unconvert(y, U8)[0]


def emu_compress(L, p):
    def f(piece, d):
        piece = np.ascontiguousarray(piece)
        out = np.zeros(d + 64, np.uint8)
        c = np.zeros(1, np.int32)
        assert L.wemu_compress_batch(C.byref(p), 1, _p(piece), _p(np.zeros(1, np.int64)), _p(np.array([piece.size], np.int32)), _p(out),
                                     _p(np.zeros(1, np.int64)), _p(np.array([d], np.int32)), _p(c)) == 0
        return out[:c[0]].tobytes()
    return f


def emu_decode(L):
    def f(chunk, nbytes):
        c = np.frombuffer(chunk, np.uint8).copy()
        out = np.zeros(nbytes, np.uint8)
        st = np.zeros(1, np.int32)
        bs = sizes([chunk])[1]
        rc = L.wemu_decompress_batch(1, _p(c), _p(np.zeros(1, np.int64)), _p(np.array([c.size], np.int32)), _p(np.array([nbytes], np.int32)), _p(bs),
                                     _p(out), _p(np.zeros(1, np.int64)), _p(st))
        assert rc == 0 and st[0] == 0, (rc, st)
        return out
    return f


@pytest.mark.parametrize("codec,filt,clevel", [(LZ4, 2, 5), (BLOSCLZ, 1, 5), (LZ4, 1, 0)], ids=["bitshuffle", "blosclz", "memcpyed"])
def test_staging_modes_with_an_oracle(L, codec, filt, clevel):
    """lz4 + bitshuffle and blosclz on the splice route, memcpyed chunks (clevel 0) on the whole route"""
    po, p, chunks, ds = case(U16, codec, filt, clevel)
    specs, src, new, stats = run_and_check(L, po, p, chunks, ds, WT.dress(shapes(len(chunks)), U16, F32, k0=1), orders=(0, 2))
    assert (stats[2] == len(chunks)) == (clevel == 0), stats


def test_zstd_chunks_go_the_whole_route(L):
    """no byte-exact oracle: the new chunks decode (the emulated read path, and libzstd through the oracle where there is one) to
    numpy's pixels and equal the emulated compress of them"""
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    p = cp(ts, 5, bsize, ZSTD)
    comp = emu_compress(L, p)
    raw = T.raw_of(T.plane(I16))
    chunks = [comp(raw[o:o + cbytes], min(cbytes, raw.size - o) + 32) for o in range(0, raw.size, cbytes)]
    ds = [min(cbytes, raw.size - o) + 32 for o in range(0, raw.size, cbytes)]
    specs, src, new, stats = run_and_check(L, None, p, chunks, ds, WT.dress(shapes(len(chunks)), I16, F32), compress=comp, planes={0: raw},
                                           decode=emu_decode(L), check_compress=comp)
    assert stats[2] == len(chunks) and stats[1] == 0
    if O.zstd_available():
        for c in new:
            assert O.decompress(c)[0] == len(emu_decode(L)(c, O.cbuffer_sizes(c)[0]))


def test_special_chunks(L):
    """zero, repeated-value, NaN and uninit chunks (and a memcpyed one) of a float32 plane, written from float16 memory"""
    chunks, plane = SC.six_chunks()                      # regular, value, nan, zero, memcpyed, uninit: 256 x 96 float32, 16 rows a chunk
    po = SC.plane_params()
    ts, PW = SC.TS, SC.PW
    wins = [S.win(3 * PW + 31, 40, 30, row_pitch=3 * PW, col_pitch=5, nchunks=6), S.win(50 * PW + 1, 1, 1, nchunks=6), S.win(64 * PW, PW, 32, row_pitch=PW, nchunks=6)]
    specs, src, vals = WT.source(WT.dress(wins, F32, F16))
    ds = [SC.CHUNK + 32] * 6
    want, edited = WT.expected(po, chunks, specs, vals, ds, planes={0: np.ascontiguousarray(plane).view(np.uint8).ravel()})
    rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 4096), chunks, specs, src, ds)
    assert rc == 0 and not st.any(), (rc, st)
    assert all(c is not None for c in new)
    WT.check_new(po, chunks, specs, new, want, edited)


def test_trunc_prec_applies_after_the_conversion(L):
    """float32 plane, 12 mantissa bits kept: a written pixel is converted first and truncated like the chunk's own then"""
    ts, m = 4, 12
    t = TR.trunc(TR.pixels("tiled", np.float32, 512, 48), ts, m)
    po = TR.oracle_cparams(ts, m, clevel=5, blocksize=8192)
    chunks = oracle_chunks(po, t, 32768)
    ds = [32768 + 32] * len(chunks)
    n = len(chunks)
    wins = [S.win(512 * 5 + 3, 100, 10, row_pitch=3 * 512, col_pitch=5, nchunks=n), S.win(512 * 20 + 9, 64, 4, row_pitch=512, nchunks=n)]
    for mem in (F32, F16):
        specs, src, vals = WT.source(WT.dress(wins, F32, mem, k0=1))
        want, edited = WT.expected(None, chunks, specs, vals, ds, compress=lambda raw, d: O.compress(po, TR.trunc(raw, ts, m), destsize=d)[1])
        plain = {k: v.copy() for k, v in edited.items()}
        edited = {k: TR.trunc(v, ts, m) for k, v in edited.items()}
        assert any(not np.array_equal(plain[k], edited[k]) for k in edited)          # (the truncation has something to do)
        rc, st, new, ncb, stats, _ = update(L, cp(ts, 5, 8192, trunc=m), chunks, specs, src, ds)
        assert rc == 0 and stats[2] == 0 and stats[1] > 0, (rc, stats)
        WT.check_new(po, chunks, specs, new, want, edited)


@pytest.mark.parametrize("mem", [F32, F16])
def test_pixel_major_source_of_three_planes(L, mem):
    """three channels with their own scale and offset written from (N, oh, ow, C) rows in one call: the C windows of a region read
    the channel slots of the same rows"""
    vals0, chunks, n = T.three_planes()
    cbytes, bsize = G.GEOMETRY[1]
    po, p = ocp(1, blocksize=bsize), cp(1, 5, bsize)
    ds = [len(O.decompress(c)[1]) + 32 for c in chunks]
    regions = [(10, 5, 200, 60, 1, 1), (100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5), (W - 1, H - 1, 1, 1, 1, 1), (0, 0, W, H, 2, 3)]
    specs, size = WT.pixel_major(regions, n, U8, mem, (1 / 255, 1 / (255 * 0.229), -0.5), (0.0, -0.485 / 0.229, 3.0))
    src, vals = WT.fill_pixel_major(specs, size)
    want, edited = WT.expected(po, chunks, specs, vals, ds)
    for order in (0, 1):
        rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds, order=order)
        assert rc == 0 and not st.any()
        WT.check_new(po, chunks, specs, new, want, edited)
    nb, bs = sizes(chunks)
    assert stats[1] == len(G.touched_blocks(specs, nb, bs, 1))


@pytest.mark.parametrize("stored", [U8, I16, F32, F64])
def test_identity_call_equals_the_strided_call(L, stored):
    """out_type == src_type, scale 1, offset 0, elem_pitch == typesize: new chunks, new_cbytes, status, return value and stats are
    those of cimg_update_windows_strided_device with the same windows -- on the splice route and, with a tight destsize, through
    the hand-back to the whole route"""
    ts = T.SIZE[stored]
    po, p, chunks, ds = case(stored)
    wins = [T.typed(r, stored, stored) for r in shapes(len(chunks))]
    specs, src, vals = WT.source(wins)
    plain = [{k: s[k] for k, _ in T.StridedWindow._fields_} for s in specs]
    for s in plain:                                                          # (the strided call wants dense rows even for one row)
        assert s["out_pitch"] >= s["width"] * ts
    for dsz in (ds, [len(c) + 8 for c in chunks]):
        for order in (0, 1):
            a = update(L, p, chunks, specs, src, dsz, order=order)
            b = update(L, p, chunks, plain, src, dsz, typed=False, order=order)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), (a[0], b[0])
            assert np.array_equal(a[4], b[4]), (a[4], b[4])
    want, _ = WT.expected(po, chunks, specs, vals, ds)
    a = update(L, p, chunks, specs, src, ds)
    assert a[0] == 0 and a[2] == want


I64, I32MAX = 2 ** 63 - 1, 2 ** 31 - 1


def test_refusals_leave_everything_alone(L):
    """every refusal of the typed checks is INVALID_PARAM before anything runs: d_new, new_cbytes and status keep their canaries"""
    ts = 2
    po, p, chunks, ds = case(U16)
    n = len(chunks)
    src = np.zeros(1 << 16, np.uint8)
    ok = dict(WT.typed(rect(10, 10, 80, 20, 4, 2, nchunks=n), U16, F32, 0.5, 1.0, pitch_mult=3), out_off=8, out_pitch=20 * 12)
    nan, inf = float("nan"), float("inf")
    bad = [dict(ok, scale=0.0), dict(ok, scale=-0.0), dict(ok, scale=nan), dict(ok, scale=inf), dict(ok, scale=-inf), dict(ok, offset=nan),
           dict(ok, offset=inf), dict(ok, scale=1e-46),                                                                 # (float32(1e-46) == 0)
           dict(ok, elem_pitch=3), dict(ok, elem_pitch=0), dict(ok, elem_pitch=-4), dict(ok, elem_pitch=6),             # < size; misaligned
           dict(ok, out_pitch=19 * 12 + 3), dict(ok, out_pitch=19 * 12), dict(ok, out_pitch=242), dict(ok, elem_pitch=I64 // 4 * 4, out_pitch=I64 // 4 * 4),
           dict(ok, src_type=9), dict(ok, src_type=-1), dict(ok, out_type=9), dict(ok, out_type=-1),
           dict(ok, src_type=U8), dict(ok, src_type=F32), dict(ok, src_type=F64),                                        # not the typesize
           dict(ok, out_type=U16), dict(ok, out_type=I16), dict(ok, out_type=F64, elem_pitch=8, out_pitch=20 * 8),       # non-identity integer / F64
           dict(ok, out_type=U16, elem_pitch=2, scale=1.0, offset=0.5), dict(ok, out_type=U8, elem_pitch=1),
           dict(ok, out_off=6), dict(ok, out_off=-4),
           dict(ok, col_pitch=0), dict(ok, row_pitch=19 * 4), dict(ok, origin=-1), dict(ok, width=-1), dict(ok, chunk_count=0),
           dict(ok, chunk_count=I32MAX), dict(ok, origin=W * H - 19 * 4, height=1)]
    for b in bad:
        for specs in ([b], [ok, b]):
            rc, st, new, ncb, _, alone = update(L, p, chunks, specs, src, ds)
            assert rc == ERR_INVALID_PARAM and alone, (b, rc)
    # the source address itself must be aligned like the rest of a source element's address
    rc, _, _, _, _, alone = update(L, p, chunks, [ok], src, ds, src_shift=2)
    assert rc == ERR_INVALID_PARAM and alone
    assert update(L, p, chunks, [dict(ok, out_type=F16, elem_pitch=6)], src, ds, src_shift=2)[0] == 0
    # blocks that do not hold whole elements; a chunk that is not the plane's last and ends inside an element
    nb, bs = sizes(chunks)
    rc, _, _, _, _, alone = update(L, p, chunks, [ok], src, ds, nbytes=nb, blocksize=np.full(n, 4097, np.int32))
    assert rc == ERR_INVALID_PARAM and alone
    nb2 = nb.copy()
    nb2[0] -= 1
    rc, _, _, _, _, alone = update(L, p, chunks, [ok], src, ds, nbytes=nb2, blocksize=bs)
    assert rc == ERR_INVALID_PARAM and alone
    # the strided call's own refusals stay refusals (these have run open_update_call: status and new_cbytes are zeroed, d_new is not touched)
    for q in (cp(4, 5, 4096), cp(ts, 5, 4096, BLOSCLZ), cp(ts, 5, 4096, filt=2)):
        rc, st, new, ncb, _, _ = update(L, q, chunks, [ok], src, ds)
        assert rc == ERR_INVALID_PARAM and all(x is None for x in new)
    rc, st, new, ncb, _, _ = update(L, p, chunks, [ok], src, [ds[0], 31] + ds[2:])
    assert rc == ERR_INVALID_PARAM and all(x is None for x in new)
    # an identity window may have an integer type, one row needs no out_pitch, and a good call afterwards
    for s in (dict(ok, out_type=U16, scale=1.0, offset=0.0, elem_pitch=2), dict(ok, height=1, out_pitch=0), ok):
        specs, src2, vals = WT.source([{k: v for k, v in s.items() if k not in ("out_off", "out_pitch")}])
        want, edited = WT.expected(po, chunks, specs, vals, ds)
        rc, st, new, ncb, _, _ = update(L, p, chunks, specs, src2, ds)
        assert rc == 0 and not st.any()
        WT.check_new(po, chunks, specs, new, want, edited)
    # nothing to do: status and new_cbytes are zeroed, as the strided call zeroes them
    rc, st, new, ncb, stats, _ = update(L, p, chunks, [], src, ds)
    assert rc == 0 and not st.any() and not ncb.any() and not stats.any()


def test_under_sanitizers(tmp_path):
    """planner, schedules and kernel body once more as a stand-alone ASan / UBSan program (tests/emu/window_write_typed_asan_main.cpp):
    every buffer an allocation of its exact size -- the source ends with its last element's last byte --, LDS with zero slack; all
    three write orders"""
    exe = WT.build_emu(tmp_path, sanitize=True)
    for order in ("0", "1", "2"):
        r = subprocess.run([exe, order], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ok" in r.stdout


@pytest.mark.parametrize("stored", [U8, I16, U16])
def test_read_then_write_gives_the_old_chunks_back(L, stored):
    """memory values as a typed read makes them (numpy: v * scale + offset in two steps) written back with the same pair: every
    touched chunk comes back byte for byte, for the pairs under which every 8 / 16-bit value returns to itself"""
    from _windows_strided import element_index
    po, p, chunks, ds = case(stored)
    v = T.plane(stored)
    n = len(chunks)
    for mem, sc, of in ((F32, 1 / 255, 0.0), (F32, 1 / 65535, 0.0), (F32, 1 / (255 * 0.229), -0.485 / 0.229), (F32, 1 / 255, -0.4851),
                        (F32, 2 / 65535, -1.0), (F32, 1 / 128, -1.0)) + (((F16, 1 / 255, 0.0),) if stored == U8 else ()):
        specs, size = T.pack_typed([WT.typed(r, stored, mem, sc, of, pitch_mult=1 + k % 2) for k, r in enumerate(shapes(n))])
        src = np.random.default_rng(1).integers(0, 256, size, dtype=np.uint8)
        for s in specs:
            if s["width"] and s["height"]:
                y = T.convert(v[element_index(s)], s)
                at = T.positions(s)[..., None] + np.arange(y.dtype.itemsize, dtype=np.int64)
                src[at.ravel()] = np.ascontiguousarray(y).view(np.uint8).ravel()
        rc, st, new, ncb, stats, _ = update(L, p, chunks, specs, src, ds)
        assert rc == 0 and new == chunks, (mem, sc, of)
