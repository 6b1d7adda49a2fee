"""blosc2's trunc-prec filter on the host lane emulator: the masked batched copy (csrc/trunc_kernel.h) tile by tile against numpy, then
whole chunks -- the pass followed by the emulated encode launches -- against the unchanged oracle on numpy-truncated pixels.

tests/emu/trunc_emu.cpp is compiled here into a pytest temp directory; the size and misalignment grid runs once more as a stand-alone
AddressSanitizer / UBSan program where every piece is an allocation of exactly its size (tests/emu/trunc_asan_main.cpp).  Every copied
piece has guard bytes around its destination."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _emu as E
import _oracle as O
import _trunc as T

SIZES = [1, 3, 15, 16, 17, 31, 4099, 16384 + 7, 40000]
LARGE = (16384 + 7, 40000)
FEW = [(0, 0), (0, 7), (9, 0), (5, 11), (3, 3), (15, 1)]
GUARD, CANARY = 48, 0x5A


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return T.build_emu(tmp_path_factory.mktemp("trunc_emu"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _aligned(size):
    raw = np.empty(size + 16, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:size]


def metas(ts):
    """smallest and largest valid `zeroed`, both ways of writing them"""
    M = T.MANTISSA[ts]
    return [-1, -(M - 1), 1, M - 1]


def run_pieces(L, pieces, ts, m, rng, in_place):
    """pieces: (bytes, source misalignment, destination misalignment).  Sources back to back at their alignments, destinations
    likewise with guard bytes between; returns nothing, asserts everything."""
    so, do, at_s, at_d = [], [], 0, GUARD
    for n, sm, dm in pieces:
        at_s = (at_s + 15) // 16 * 16 + sm
        so.append(at_s)
        at_s += n
        at_d = (at_d + 15) // 16 * 16 + dm
        do.append(at_d)
        at_d += n + GUARD
    src = _aligned(at_s + 16)
    src[:] = rng.integers(0, 256, src.size, dtype=np.uint8)
    keep = src.copy()
    nb = np.array([p[0] for p in pieces], np.int32)
    sp = (src.ctypes.data + np.array(so, np.int64)).astype(np.uint64)
    if in_place:
        assert L.tremu_pass(len(pieces), _p(sp), _p(sp), _p(nb), ts, m & 0xFF) == 0
        want = keep.copy()
        for (n, _, _), o in zip(pieces, so):
            want[o:o + n] = T.trunc(keep[o:o + n], ts, m)
        assert np.array_equal(src, want), (pieces[:3], ts, m)
        return
    dst = _aligned(at_d + 16)
    dst[:] = CANARY
    dp = (dst.ctypes.data + np.array(do, np.int64)).astype(np.uint64)
    assert L.tremu_pass(len(pieces), _p(sp), _p(dp), _p(nb), ts, m & 0xFF) == 0
    want = np.full(dst.size, CANARY, np.uint8)
    for (n, _, _), s, d in zip(pieces, so, do):
        want[d:d + n] = T.trunc(keep[s:s + n], ts, m)
    assert np.array_equal(dst, want), (pieces[:3], ts, m)
    assert np.array_equal(src, keep), "the source of a copy was written"


@pytest.mark.parametrize("ts", [2, 4, 8])
@pytest.mark.parametrize("in_place", [False, True])
def test_every_size_and_misalignment(L, ts, in_place):
    """one piece a call: every source and destination alignment 0..15 independently (so the piece start is mostly no multiple of the
    typesize, and most sizes leave nbytes % typesize != 0)"""
    rng = np.random.default_rng(ts)
    for n in SIZES:
        pairs = FEW if n in LARGE else [(s, d) for s in range(16) for d in range(16)]
        for i, (sm, dm) in enumerate(pairs):
            if in_place and dm:
                continue                                        # (in place has one address)
            run_pieces(L, [(n, sm, dm)], ts, metas(ts)[i % 4], rng, in_place)


@pytest.mark.parametrize("order", [1, 2])
def test_lane_order_does_not_matter(L, order):
    rng = np.random.default_rng(5)
    L.tremu_write_order(order)
    try:
        for ts in (2, 4, 8):
            for in_place in (False, True):
                run_pieces(L, [(n, (3 * n) % 16, (5 * n + 1) % 16) for n in SIZES], ts, -(T.MANTISSA[ts] - 1), rng, in_place)
    finally:
        L.tremu_write_order(0)


@pytest.mark.parametrize("ts", [2, 4, 8])
def test_whole_grid_in_one_call(L, ts):
    rng = np.random.default_rng(7)
    pieces = [(n, s, d) for n in SIZES for s, d in FEW] + [(0, 1, 2)]
    for in_place in (False, True):
        run_pieces(L, pieces, ts, 3, rng, in_place)


def test_work_follows_bytes(L):
    a = _aligned(4 << 20)
    one = (np.array([a.ctypes.data], np.uint64), np.array([4 << 20], np.int32))
    assert L.tremu_tiles(1, _p(one[0]), _p(one[0]), _p(one[1]), 4) == 256
    many = (np.array([a.ctypes.data + 16384 * k for k in range(256)], np.uint64), np.full(256, 16384, np.int32))
    assert L.tremu_tiles(256, _p(many[0]), _p(many[0]), _p(many[1]), 4) == 256
    tiny = (np.array([a.ctypes.data + 3, a.ctypes.data + 100], np.uint64), np.array([0, 5], np.int32))
    assert L.tremu_tiles(2, _p(tiny[0]), _p(tiny[0]), _p(tiny[1]), 8) == 1


def test_nan_with_only_low_mantissa_bits_becomes_inf(L):
    x = np.array([np.nan, 1.0, -np.inf], np.float32).view(np.uint32)
    x[0] = 0x7F800001
    raw = x.view(np.uint8).copy()
    sp = np.array([raw.ctypes.data], np.uint64)
    assert L.tremu_pass(1, _p(sp), _p(sp), _p(np.array([12], np.int32)), 4, 12) == 0
    out = raw.view(np.float32)
    assert np.isposinf(out[0]) and out[1] == 1.0 and np.isneginf(out[2])


def emu_compress(L, p, raw, destsize=None):
    work = np.array(raw, np.uint8)                              # the engine owns these pixels: the pass runs in place over them
    ds = np.array([raw.size + 32 if destsize is None else destsize], np.int32)
    comp = np.full(int(ds[0]) + 128, CANARY, np.uint8)
    cb = np.zeros(1, np.int32)
    rc = L.tremu_compress_batch(C.byref(p), 1, _p(work), _p(np.zeros(1, np.int64)), _p(np.array([raw.size], np.int32)), _p(comp),
                                _p(np.zeros(1, np.int64)), _p(ds), _p(cb))
    assert (comp[int(ds[0]):] == CANARY).all(), "bytes behind the chunk's destsize were written"
    return rc, comp[:max(int(cb[0]), 0)].tobytes(), work


@pytest.mark.parametrize("case", list(T.chunk_cases()), ids=lambda c: c[0])
def test_pass_then_encoder_equals_the_oracle(L, case):
    name, raw, ts, m, code, filt = case
    want, t = T.expected_chunk(raw, ts, m, compcode=code, filt=filt)
    assert want[16 + 4] == T.TRUNC_PREC and want[24 + 4] == m & 0xFF          # the oracle carries the filter byte and its meta
    rc, got, work = emu_compress(L, T.emu_cparams(ts, m, compcode=code, filt=filt), raw)
    assert rc == 0
    assert got == want, name
    assert np.array_equal(work, t)
    # decompress(compress(x)) == trunc(x), by the oracle and by the emulated decoder (which reads the filter as a no-op)
    assert np.array_equal(O.decompress(got)[1], t)
    rc, status, outs = E.decompress_batch([got], [raw.size], [min(32768, raw.size)])
    assert rc == 0 and status == [0] and np.array_equal(outs[0], t)
    # compress(trunc(x)) == compress(x)
    assert emu_compress(L, T.emu_cparams(ts, m, compcode=code, filt=filt), t)[1] == got


def test_memcpyed_chunk_holds_truncated_pixels(L):
    raw = T.random_patterns()
    want, t = T.expected_chunk(raw, 4, 20)
    assert want[2] & 0x02 and len(want) == 49184 and want[32:] == t.tobytes()  # the oracle's chunk is memcpyed
    assert not np.array_equal(t, raw)
    rc, got, _ = emu_compress(L, T.emu_cparams(4, 20), raw)
    assert rc == 0 and got == want
    # memcpyed up front (clevel 0) and special-zero
    want0, t0 = T.expected_chunk(raw, 4, 20, clevel=0)
    rc, got, _ = emu_compress(L, T.emu_cparams(4, 20, clevel=0), raw)
    assert rc == 0 and got == want0 and got[32:] == t0.tobytes()
    tiny = np.zeros(65536, np.uint8)
    tiny[::4] = 1                                                # denormals whose only set bits are zeroed: the chunk becomes all zero
    wantz, tz = T.expected_chunk(tiny, 4, 12)
    assert not tz.any() and len(wantz) == 32
    rc, got, _ = emu_compress(L, T.emu_cparams(4, 12), tiny)
    assert rc == 0 and got == wantz


def test_invalid_meta_is_invalid_param(L):
    raw = T.pixels("tiled", np.float32)
    for ts, m in ((4, 0), (4, 24), (4, -23), (2, 11), (8, 53), (1, 3), (3, 3)):
        rc, got, work = emu_compress(L, T.emu_cparams(ts, m), raw[:65536 // ts * ts] if ts != 3 else raw[:65535])
        assert rc == T.ERR_INVALID_PARAM and got == b""
        assert np.array_equal(work, raw[:work.size]), "pixels were touched by a refused call"


def test_the_existing_emulator_library_still_refuses_the_parameters():
    raw = T.pixels("tiled", np.float32)
    p = E.cparams(4, filters=(0, 0, 0, 0, 4, 1))
    p.filters_meta[4] = 12
    rc, cb, chunks = E.compress_batch(p, raw, [raw.size], [raw.size + 32])
    assert rc == T.ERR_CODEC_SUPPORT


def test_grid_under_address_sanitizer(tmp_path_factory):
    out = T.build_emu(tmp_path_factory.mktemp("trunc_asan"), sanitize=True)
    r = subprocess.run([out] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    small = sum(1 for n in SIZES if n <= 4099)
    assert r.stdout.split() == ["ok", str(2 * 3 * (256 * small + 4 * (len(SIZES) - small)))], r.stdout
