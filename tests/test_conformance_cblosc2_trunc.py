"""The switch for the recalled trunc-prec rules ([UPSTREAM-RECALL]): where a genuine c-blosc2 is found (the
unchanged tests/_cblosc2.py: CIMG_BLOSC2_LIB, find_library, a python blosc2 wheel), float32 / float64 chunks it writes with
filters = [0, 0, 0, 0, TRUNC_PREC, SHUFFLE] are compared byte for byte with the oracle's compress of numpy-truncated pixels (what the
emulator and the GPU are held to), and each side reads the other's chunks.  Regular chunks only: a memcpyed fallback holds
UNtruncated pixels upstream and truncated ones here (a recorded deviation).  No libblosc2 exists on the machines this was written
on, so the byte tests skip there."""
import numpy as np
import pytest

import _cblosc2 as R
import _oracle as O
import _trunc as T

B, LIBNAME = R.open_blosc2()
needs_blosc2 = pytest.mark.skipif(B is None, reason="no c-blosc2 shared library on this box: the trunc-prec rules stay recalled, not pinned")

CASES = [(np.float32, 4, 12), (np.float32, 4, -15), (np.float32, 4, 23), (np.float32, 4, 1), (np.float64, 8, 30), (np.float64, 8, -40), (np.float64, 8, 52)]


def _ctx(ts, m, code):
    cp = R.Blosc2CParamsReal()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = code, 9, ts, 1, R.BLOCK, 3
    cp.filters[4], cp.filters_meta[4], cp.filters[5] = T.TRUNC_PREC, m & 0xFF, O.SHUFFLE
    ctx = B.blosc2_create_cctx(cp)
    assert ctx, "blosc2_create_cctx failed"
    return ctx


@needs_blosc2
@pytest.mark.parametrize("family", ["tiled", "natural"])
@pytest.mark.parametrize("code", [O.LZ4, O.BLOSCLZ])
def test_regular_chunks_equal_real_cblosc2_bytes(family, code):
    print(f"c-blosc2 found: {LIBNAME} (version {R.version(B)})")
    differing = []
    d = R.dctx(B, 1)
    for dtype, ts, m in CASES:
        raw = T.pixels(family, dtype)
        ctx = _ctx(ts, m, code)
        r, ref = R.compress(B, ctx, raw, raw.size + 32)
        B.blosc2_free_ctx(ctx)
        assert r > 0, (family, dtype, m, r)
        want, t = T.expected_chunk(raw, ts, m, compcode=code)
        if ref[2] & 0x02:
            continue                                         # memcpyed upstream: the recorded deviation, not compared
        if ref != want:
            differing.append(f"{family} {np.dtype(dtype).name} m={m} codec {code}: oracle {len(want)} B vs c-blosc2 {len(ref)} B")
        assert np.array_equal(O.decompress(ref)[1], t), "the oracle reads c-blosc2's chunk to other pixels than trunc(x)"
        buf, out = np.frombuffer(want, np.uint8).copy(), np.zeros(raw.size, np.uint8)
        assert B.blosc2_decompress_ctx(d, buf.ctypes.data, 2**31 - 1, out.ctypes.data, out.size) == raw.size
        assert np.array_equal(out, t)
    B.blosc2_free_ctx(d)
    assert not differing, "oracle on truncated pixels != c-blosc2 %s:\n  " % R.version(B) + "\n  ".join(differing)


@needs_blosc2
def test_real_cblosc2_validity_rule():
    """m = 0 and |m| > M are refused upstream as here"""
    raw = T.pixels("tiled", np.float32)
    for m, ok in ((12, True), (23, True), (0, False), (24, False), (-23, False), (-22, True)):
        ctx = _ctx(4, m, O.LZ4)
        r, _ = R.compress(B, ctx, raw, raw.size + 32)
        B.blosc2_free_ctx(ctx)
        assert (r > 0) == ok, (m, r)
        assert (T.zeroed_bits(4, m) is not None) == ok
