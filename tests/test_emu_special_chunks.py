"""blosc2 special-value chunks (csrc/special_plan.h) on the CPU: every read route of the emulated kernels and of the mock C ABI, the
window write, the four blosc2_chunk_* constructors, and a stand-alone AddressSanitizer / UBSan program.

The chunks come from tests/_special_chunks.py, a writer that works from the format; what every route must give is the oracle's decode
of the same chunk (into a zeroed destination: an uninit chunk reads as zeros here).  emu.cpp, wide_emu.cpp, window_grouped_emu.cpp
(which includes the plain and the strided window calls) and window_write_emu.cpp are compiled into one library in a pytest temp
directory with the flags of tests/emu/Makefile.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _emu as E
import _oracle as O
import _special_chunks as S
import _window_writes as WW
from _special_chunks import CHUNK, PH, PW, TS, b2params, construct, plane_params, plane_regions, six_chunks
from _windows import CANARY, concat, expected, pack, sizes, windows
from _windows_strided import expected as sexpected
from _windows_strided import swindows
from cimg import hip

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
FLAGS = ["-std=c++17", "-fPIC", "-Wall", "-Wextra", "-fno-strict-aliasing", "-I", CSRC]
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_grouped_emu.cpp")]
ERR_DATA = S.ERR_DATA
READS = S.read_cases()
REFUSED = S.refused_cases()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("special_emu") / "libspecial_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, os.path.join(EMU, "window_write_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.wemu_decompress_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    for kind in ("", "_strided", "_grouped"):
        getattr(lib, "wnemu_windows%s_device" % kind).argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        getattr(lib, "wnemu_windows%s_host" % kind).argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    lib.wnemu_window_stats.argtypes = [vp]
    lib.wwemu_update_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.wwemu_update_host.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.wwemu_free.argtypes = [vp]
    return lib


@pytest.fixture(scope="module")
def mock(tmp_path_factory):
    """the mock C ABI (blosc2 shim + batch calls over the emulator), and blosc2_getitem_ctx over the mock window call"""
    subprocess.check_call(["make", "-s", "-C", EMU])
    lib = C.CDLL(os.path.join(EMU, "libcimg_hip_mock.so"))
    vp = C.c_void_p
    lib.blosc2_create_dctx.argtypes = [hip.Blosc2DParams]
    lib.blosc2_create_dctx.restype = vp
    lib.blosc2_free_ctx.argtypes = [vp]
    lib.blosc2_decompress_ctx.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
    lib.cimg_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.cimg_engine_destroy.argtypes = [vp]
    lib.cimg_decompress_batch_host_sized.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    lib.cimg_decompress_batch_host.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    for name in ("blosc2_chunk_zeros", "blosc2_chunk_nans", "blosc2_chunk_uninit"):
        getattr(lib, name).argtypes = [hip.Blosc2CParams, C.c_int32, vp, C.c_int32]
    lib.blosc2_chunk_repeatval.argtypes = [hip.Blosc2CParams, C.c_int32, vp, C.c_int32, vp]
    out = str(tmp_path_factory.mktemp("special_getitem") / "libgetitem_mock.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "blosc2_getitem.cpp"),
                           os.path.join(EMU, "mock_window.cpp"), "-o", out, "-L", EMU, "-lcimg_hip_mock", "-Wl,-rpath," + EMU])
    g = C.CDLL(out)
    g.blosc2_getitem_ctx.argtypes = [vp, vp, C.c_int32, C.c_int, C.c_int, vp, C.c_int32]
    lib.getitem = g.blosc2_getitem_ctx
    return lib


# ---- the batch routes ---------------------------------------------------------------------------------------------------------------

def batch(L, chunks, mis=0, sized=True):
    """the emulated batch decode (general, lean and wide launches) into outputs that sit between canaries -> (rc, status, outputs)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    gap = 16 + mis
    raw_off = np.zeros(len(chunks), np.int64)
    at = gap
    for i, n in enumerate(nb):
        raw_off[i] = at
        at += int(n) + gap
    raw = np.full(at + 64, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    rc = L.wemu_decompress_batch(len(chunks), _p(buf), _p(off), _p(cs) if sized else None, _p(nb), _p(bs), _p(raw), _p(raw_off), _p(st))
    outs, mask = [], np.ones(raw.size, bool)
    for o, n in zip(raw_off, nb):
        outs.append(raw[o:o + n].copy())
        mask[o:o + n] = False
    assert (raw[mask] == CANARY).all(), "a byte outside the outputs was written"
    return rc, st, outs


@pytest.mark.parametrize("name,chunk", READS, ids=[n for n, _ in READS])
def test_batch_read(L, name, chunk):
    want = S.want(chunk)
    for mis in (0, 1, 5, 15):
        for sized in (True, False):
            rc, st, outs = batch(L, [chunk], mis=mis, sized=sized)
            assert rc == 0 and st[0] == 0, (rc, st)
            assert np.array_equal(outs[0], want), (name, mis, sized)


def test_batch_of_all_kinds_with_regular_neighbours(L):
    """every kind in ONE batch between regular chunks: block numbering, the lean launch in front, and the canaries between outputs"""
    reg, raw = S.regular_chunk(4, S.geometry_nbytes(4))
    chunks = [reg] + [c for _, c in READS] + [reg]
    rc, st, outs = batch(L, chunks, mis=3)
    assert rc == 0 and not st.any(), (rc, st)
    for c, got in zip(chunks, outs):
        assert np.array_equal(got, S.want(c))


@pytest.mark.parametrize("name,chunk", REFUSED, ids=[n for n, _ in REFUSED])
def test_refusals_leave_the_neighbours_decoded(L, mock, name, chunk):
    assert S.want(chunk) == ERR_DATA                                             # the oracle refuses it the same way
    reg, raw = S.regular_chunk(4, S.geometry_nbytes(4))
    good = S.chunk("value", 4, S.geometry_nbytes(4), 4096)
    chunks = [reg, chunk, good, reg]
    rc, st, outs = batch(L, chunks)
    assert list(st) == [0, ERR_DATA, 0, 0], st
    assert np.array_equal(outs[0], raw) and np.array_equal(outs[3], raw) and np.array_equal(outs[2], S.want(good))
    assert (outs[1] == CANARY).all()                                             # nothing of the refused chunk was written
    rc, st, outs = mock_host(mock, chunks)
    assert rc == ERR_DATA and list(st) == [0, ERR_DATA, 0, 0]
    assert np.array_equal(outs[0], raw) and np.array_equal(outs[3], raw) and np.array_equal(outs[2], S.want(good))
    # a window into the refused chunk fails with its code; one beside it is served
    ts = chunk[3]
    nb, bs = sizes([chunk])
    elems = int(nb[0]) // ts
    for kind in ("", "_strided", "_grouped"):
        for host in (False, True):
            rc, st, out, _ = window_call(L, [chunk], [dict(chunk_first=0, chunk_count=1, origin=0, row_pitch=elems, width=min(elems, 100), height=1)], ts,
                                         kind=kind, host=host)
            assert rc == ERR_DATA and st[0] == ERR_DATA, (kind, host, rc, st)
            if not host:
                assert (out == CANARY).all()                                         # (the host form hands its staged rows over whatever the status)


def test_wide_blocks(L):
    """one special-value chunk with 192 KiB blocks: the wide decoder's twin of phase A"""
    for ts, nbytes in ((4, 2 * 196608 + 1000), (3, 2 * 196608 + 999)):
        chunk = S.chunk("value", ts, nbytes, 196608)
        rc, st, outs = batch(L, [chunk], mis=5)
        assert rc == 0 and st[0] == 0 and L.wemu_last_wide() == 1
        assert np.array_equal(outs[0], S.want(chunk))
    reg, raw = S.regular_chunk(4, 9192)
    nan = S.chunk("nan", 8, 196608 + 4096, 196608)
    rc, st, outs = batch(L, [reg, nan, S.chunk("uninit", 2, 196608 * 2, 196608)])
    assert rc == 0 and not st.any() and np.array_equal(outs[0], raw) and np.array_equal(outs[1], S.want(nan)) and not outs[2].any()


# ---- the mock C ABI: host batch calls and the blosc2 shim ------------------------------------------------------------------------------

def mock_host(mock, chunks, sized=True):
    eng = C.c_void_p()
    assert mock.cimg_engine_create(0, C.byref(eng)) == 0
    try:
        buf, off, cs = concat(chunks)
        nb, _ = sizes(chunks)
        raw_off = np.concatenate([[0], np.cumsum(nb[:-1].astype(np.int64) + 32)]).astype(np.int64) + 16
        raw = np.full(int(raw_off[-1]) + int(nb[-1]) + 64, CANARY, np.uint8)
        st = np.zeros(len(chunks), np.int32)
        if sized:
            rc = mock.cimg_decompress_batch_host_sized(eng, len(chunks), _p(buf), _p(off), _p(cs), _p(raw), _p(raw_off), _p(nb), _p(st))
        else:
            rc = mock.cimg_decompress_batch_host(eng, len(chunks), _p(buf), _p(off), _p(raw), _p(raw_off), _p(nb), _p(st))
        outs, mask = [], np.ones(raw.size, bool)
        for o, n, s in zip(raw_off, nb, st):
            outs.append(raw[o:o + n].copy())
            if s == 0:
                mask[o:o + n] = False
        assert (raw[mask] == CANARY).all()
        return rc, st, outs
    finally:
        mock.cimg_engine_destroy(eng)


@pytest.mark.parametrize("name,chunk", READS, ids=[n for n, _ in READS])
def test_mock_host_calls_and_shim(mock, name, chunk):
    want = S.want(chunk)
    for sized in (True, False):
        rc, st, outs = mock_host(mock, [chunk], sized=sized)
        assert rc == 0 and st[0] == 0 and np.array_equal(outs[0], want)
    dctx = mock.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    try:
        src = np.frombuffer(chunk, np.uint8)
        dest = np.full(want.size + 32, CANARY, np.uint8)
        assert mock.blosc2_decompress_ctx(dctx, _p(src), len(chunk), _p(dest), want.size) == want.size
        assert np.array_equal(dest[:want.size], want) and (dest[want.size:] == CANARY).all()
        ts = chunk[3]
        n = want.size // ts
        for start, k in ((0, 1), (n - 1, 1), (4096 // ts - 1, 3), (1, n - 1)):          # (the third one straddles the first block boundary)
            dest = np.full(k * ts + 16, CANARY, np.uint8)
            assert mock.getitem(dctx, _p(src), len(chunk), start, k, _p(dest), k * ts) == k * ts
            assert np.array_equal(dest[:k * ts], want[start * ts:(start + k) * ts]) and (dest[k * ts:] == CANARY).all()
    finally:
        mock.blosc2_free_ctx(dctx)


# ---- windows: a plane of 256 x 96 float32 in six 16-row chunks --------------------------------------------------------------------------
def window_call(L, chunks, specs, ts, kind="", host=False, size=None):
    specs, psize = pack(specs, ts)
    size = psize if size is None else size
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    out = np.full(size, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    w = windows(specs) if kind == "" else swindows([dict(col_pitch=1, **s) if "col_pitch" not in s else s for s in specs])
    if host:
        rc = getattr(L, "wnemu_windows%s_host" % kind)(len(chunks), _p(buf), _p(off), _p(cs), len(specs), w, _p(out), _p(st))
    else:
        rc = getattr(L, "wnemu_windows%s_device" % kind)(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), ts, len(specs), w, _p(out), _p(st))
    stats = np.zeros(3, np.int64)
    L.wnemu_window_stats(_p(stats))
    return rc, st, out, stats


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["", "_strided", "_grouped"], ids=["plain", "strided", "grouped"])
def test_windows_over_six_kinds(L, kind, host):
    chunks, plane = six_chunks()
    px = plane.view(np.uint32).reshape(PH, PW)
    sx, sy = (1, 1) if kind == "" else (3, 5)
    specs = []
    for (x, y, w, h) in plane_regions():
        s = dict(chunk_first=0, chunk_count=6, origin=y * PW + x, row_pitch=sy * PW, width=(w + sx - 1) // sx, height=(h + sy - 1) // sy)
        if kind != "":
            s["col_pitch"] = sx
        specs.append(s)
    packed, size = pack(specs, TS)
    rc, st, out, stats = window_call(L, chunks, specs, TS, kind=kind, host=host)
    assert rc == 0 and not st.any(), (rc, st)
    want = (expected if kind == "" else sexpected)([plane] * len(packed), packed, TS, size)
    assert np.array_equal(out, want)
    # ... which is numpy indexing of the oracle's decode
    for s, (x, y, w, h) in zip(packed, plane_regions()):
        got = np.stack([out[s["out_off"] + r * s["out_pitch"]:s["out_off"] + r * s["out_pitch"] + s["width"] * TS] for r in range(s["height"])])
        assert np.array_equal(got.view(np.uint32), px[y:y + h:sy, x:x + w:sx])
    assert stats[1] == 0                                                         # no chunk went the whole-chunk way: nothing was staged
    if host:
        assert stats[2] == sum(len(c) for c in chunks)                           # every chunk is touched: 32 + 4 bytes for the value chunk


def test_host_window_uploads_cbytes_of_a_value_chunk(L):
    chunks, plane = six_chunks()
    assert len(chunks[1]) == 36
    for kind in ("", "_strided", "_grouped"):
        spec = dict(chunk_first=0, chunk_count=6, origin=20 * PW + 9, row_pitch=PW, width=40, height=3)      # rows 20 .. 22: the value chunk only
        rc, st, out, stats = window_call(L, chunks, [spec], TS, kind=kind, host=True)
        assert rc == 0 and stats[2] == 32 + TS, stats
        spec = dict(chunk_first=0, chunk_count=6, origin=20 * PW + 9, row_pitch=PW, width=40, height=20)     # ... and the nan chunk
        rc, st, out, stats = window_call(L, chunks, [spec], TS, kind=kind, host=True)
        assert rc == 0 and stats[2] == 32 + TS + 32, stats


def test_special_field_is_decided_before_the_codec(L, mock):
    """a special chunk whose flags say zstd, or memcpyed, is still the special chunk -- on the host window call too, whose planner
    looks at the flags to find zstd chunks up front"""
    n = S.geometry_nbytes(4)
    for flags in (0x01 | 0x04 | 0x10 | (4 << 5), S.FLAGS_LZ4_UNSPLIT | 0x02):
        for kind in ("value", "nan", "uninit"):
            chunk = S.chunk(kind, 4, n, 4096, flags=flags)
            want = S.want(chunk)
            rc, st, outs = batch(L, [chunk])
            assert rc == 0 and st[0] == 0 and np.array_equal(outs[0], want), (flags, kind)
            rc, st, outs = mock_host(mock, [chunk])
            assert rc == 0 and np.array_equal(outs[0], want)
            spec = dict(chunk_first=0, chunk_count=1, origin=5, row_pitch=n // 4, width=n // 4 - 5, height=1)
            for wk in ("", "_strided", "_grouped"):
                for host in (False, True):
                    rc, st, out, stats = window_call(L, [chunk], [spec], 4, kind=wk, host=host)
                    assert rc == 0 and stats[1] == 0, (flags, kind, wk, host, stats)      # cut from the chunk, not decoded whole
                    packed, size = pack([spec], 4)
                    assert np.array_equal(out, expected([want], packed, 4, size))


# ---- window write ------------------------------------------------------------------------------------------------------------------------

def update(L, p, chunks, specs, src, destsize, host):
    buf, off, cs = concat(chunks)
    before = buf.copy()
    nb, bs = sizes(chunks)
    n = len(chunks)
    ds = np.asarray(destsize, np.int32)
    st = np.zeros(n, np.int32)
    ncb = np.zeros(n, np.int32)
    w = windows(specs)
    if host:
        ptrs = (C.c_void_p * n)()
        rc = L.wwemu_update_host(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(ds), len(specs), w, _p(src), ptrs, _p(ncb), _p(st))
        new = []
        for i in range(n):
            new.append(C.string_at(ptrs[i], int(ncb[i])) if ptrs[i] else None)
            if ptrs[i]:
                L.wwemu_free(ptrs[i])
    else:
        new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
        nbuf = np.full(int(new_off[-1]) + int(ds[-1]) + 64, CANARY, np.uint8)
        rc = L.wwemu_update_device(C.byref(p), n, _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(ds), len(specs), w, _p(src), _p(nbuf), _p(new_off),
                                   _p(ncb), _p(st))
        new = [nbuf[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]
    assert np.array_equal(buf, before), "the input chunks were modified"
    return rc, st, new


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_window_write_into_special_chunks(L, host):
    chunks, plane = six_chunks()
    p = plane_params()
    # rows 20 .. 39: the value chunk (rows 16 .. 31) and the nan chunk (rows 32 .. 47); nothing else is touched
    specs, src = WW.source([dict(chunk_first=0, chunk_count=6, origin=20 * PW + 30, row_pitch=PW, width=100, height=20)], TS, seed=4)
    destsize = [CHUNK + 32] * 6
    ep = E.cparams(TS, clevel=5, blocksize=4096)                                     # the same parameters in the engine's layout
    rc, st, new = update(L, ep, chunks, specs, src, destsize, host)
    assert rc == 0 and not st.any(), (rc, st)
    want, _ = WW.expected(p, chunks, specs, TS, src, destsize)
    assert [c is not None for c in new] == [False, True, True, False, False, False]
    assert new[1] == want[1] and new[2] == want[2]                                  # byte for byte the oracle's compress of the edited pixels
    after = [c if c is not None else old for c, old in zip(new, chunks)]
    edited = WW.apply({0: plane}, specs, TS, src)[0]
    assert np.array_equal(np.concatenate([S.want(c) for c in after]), edited)
    # the uninit chunk: zeros with the window written in
    specs, src = WW.source([dict(chunk_first=0, chunk_count=6, origin=85 * PW + 1, row_pitch=PW, width=7, height=3)], TS, seed=5)
    rc, st, new = update(L, ep, chunks, specs, src, destsize, host)
    assert rc == 0 and [c is not None for c in new] == [False] * 5 + [True]
    assert new[5] == WW.expected(p, chunks, specs, TS, src, destsize)[0][5]


# ---- the constructors ---------------------------------------------------------------------------------------------------------------------

CONSTRUCT = [(ts, codec, clevel, split, filt) for ts in (1, 2, 3, 4, 8, 12, 16, 255) for codec, clevel, split, filt in
             ((1, 5, 3, 1), (0, 9, 1, 1), (5, 3, 2, 0), (2, 0, 3, 2))]


def test_constructor_bytes(mock):
    dctx = mock.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    try:
        for ts, codec, clevel, split, filt in CONSTRUCT:
            if filt == 2 and split == 1:
                continue
            for nbytes in (S.geometry_nbytes(ts), ts, 0):
                cp = b2params(ts, clevel=clevel, compcode=codec, splitmode=split, filt=filt)
                po = O.cparams(ts, clevel=clevel, blocksize=4096, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
                for kind in ("zero", "value", "uninit") + (("nan",) if ts in (4, 8) else ()):
                    value = S.value_bytes(ts, seed=ts) if kind == "value" else None
                    rc, got = construct(mock, kind, cp, nbytes, value=value)
                    want = S.from_cparams(po, kind, nbytes, value=value)
                    assert rc == len(want) and got == want, (ts, codec, kind, nbytes)
                    if nbytes == 0:
                        continue
                    pixels = S.want(got)
                    dest = np.full(nbytes + 8, CANARY, np.uint8)
                    assert mock.blosc2_decompress_ctx(dctx, _p(np.frombuffer(got, np.uint8)), len(got), _p(dest), nbytes) == nbytes
                    assert np.array_equal(dest[:nbytes], pixels) and (dest[nbytes:] == CANARY).all()
                    k = nbytes // ts
                    dest = np.full(ts + 8, CANARY, np.uint8)
                    assert mock.getitem(dctx, _p(np.frombuffer(got, np.uint8)), len(got), k - 1, 1, _p(dest), ts) == ts
                    assert np.array_equal(dest[:ts], pixels[-ts:]) and (dest[ts:] == CANARY).all()
        # a zero chunk is the chunk the oracle writes for zeros
        po = O.cparams(4, clevel=5, blocksize=4096)
        r, z = O.compress(po, np.zeros(9192, np.uint8), destsize=9192 + 32)
        assert construct(mock, "zero", b2params(4), 9192)[1] == z
    finally:
        mock.blosc2_free_ctx(dctx)


def test_constructor_refusals(mock):
    cp = b2params(4)
    for kind in ("zero", "nan", "uninit"):
        assert construct(mock, kind, cp, 4096, destsize=31)[0] == ERR_DATA           # the header does not fit
        assert construct(mock, kind, cp, 4098)[0] == ERR_DATA                        # nbytes % typesize != 0
        assert construct(mock, kind, cp, 4096, destsize=32)[0] == 32
    assert construct(mock, "value", cp, 4096, destsize=35, value=b"abcd")[0] == ERR_DATA
    assert construct(mock, "value", cp, 4098, value=b"abcd")[0] == ERR_DATA
    assert construct(mock, "value", cp, 4096, destsize=36, value=b"abcd")[0] == 36
    assert construct(mock, "nan", b2params(2), 4096)[0] == ERR_DATA                  # no NaN of that width
    assert mock.blosc2_chunk_repeatval(cp, 4096, _p(np.zeros(64, np.uint8)), 64, None) == -23
    assert mock.blosc2_chunk_zeros(cp, 4096, None, 64) == -23
    bad = b2params(4)
    bad.filters[2] = 1                                                                # a filter this library does not run: as blosc2_compress_ctx
    assert construct(mock, "zero", bad, 4096)[0] == -7


def test_repeatval_with_trunc_prec_stores_the_truncated_value(mock):
    for dtype, m, M in ((np.float32, 8, 23), (np.float64, 20, 52), (np.float16, 3, 10)):
        ts = np.dtype(dtype).itemsize
        v = np.array([np.pi], dtype)
        u = v.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[ts])
        kept = (u & u.dtype.type(~((1 << (M - m)) - 1) & ((1 << (8 * ts)) - 1))).tobytes()
        assert kept != v.tobytes()
        rc, got = construct(mock, "value", b2params(ts, trunc=m), 4096, value=v.tobytes())
        assert rc == 32 + ts and got[32:] == kept
        assert got[16 + 4] == 4 and got[24 + 4] == m                                  # the header names the filter and its meta
        assert S.want(got).tobytes() == kept * (4096 // ts)


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------------

def test_pattern_fill_and_window_mode_under_sanitizers(tmp_path):
    exe = str(tmp_path / "special_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                           os.path.join(EMU, "special_asan_main.cpp"), *SOURCES, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "special asan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
