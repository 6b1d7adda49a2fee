"""blosc2's trunc-prec filter on the MI355X: cimg_trunc_prec (csrc/trunc_kernel.h) in front of every compress route, the filter as a
no-op on every read route, and window writes over truncated chunks.

Expectations come from the unchanged oracle on numpy-truncated pixels (tests/_trunc.py).

The window write: a 64 x 64 window at (100, 40) does not fit a plane of 96 rows (rows 40 .. 103), so it is written into the 512 x 130
float32 plane of the chunk cases (65 536-byte chunks: it meets three of them), and clipped to the 56 rows that exist into the
512 x 96 one."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _trunc as T
from _window_writes import expected as ww_expected, source as ww_source
from _windows import CANARY, concat, expected as win_expected, oracle_chunks, pack, sizes
from cimg import hip

pytestmark = pytest.mark.gpu
ERR_INVALID_PARAM = -12


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def hip_cparams(ts, m, code=hip.LZ4, filt=hip.SHUFFLE, **kw):
    return hip.cparams(ts, compcode=code, filters=(0, 0, 0, 0, 0, filt), trunc_prec=m, **kw)


def device_compress(eng, p, raw, lead=0, destsize=None):
    """one chunk from a caller's device buffer that starts `lead` bytes into an allocation -> (chunk bytes, the buffer afterwards)"""
    n = raw.size
    ds = n + 32 if destsize is None else destsize
    d_raw, d_comp = eng.alloc(n + lead + 64), eng.alloc(ds + 64)
    hold = np.full(n + lead + 64, 0xC3, np.uint8)
    hold[lead:lead + n] = raw
    d_raw.upload(hold)
    d_comp.upload(np.full(ds + 64, 0x5A, np.uint8))
    cb = eng.compress_device(p, d_raw.ptr + lead, [0], [n], d_comp.ptr, [0], [ds])
    out, after = d_comp.download(), d_raw.download()
    d_raw.free(); d_comp.free()
    assert (out[ds:] == 0x5A).all()
    assert np.array_equal(after, hold), "the caller's pixels were modified"
    return out[:max(int(cb[0]), 0)].tobytes()


@pytest.mark.parametrize("case", list(T.chunk_cases()), ids=lambda c: c[0])
def test_chunks_equal_the_oracle_on_truncated_pixels(eng, case):
    name, raw, ts, m, code, filt = case
    want, t = T.expected_chunk(raw, ts, m, compcode=code, filt=filt)
    p = hip_cparams(ts, m, code, filt)
    (host,) = eng.compress_host(p, raw, [raw.size], [raw.size + 32])
    assert host == want, "host call"
    assert device_compress(eng, p, raw) == want, "device call"
    outs, st = eng.decompress_host([host])
    assert st[0] == 0 and np.array_equal(outs[0], t)


def test_memcpyed_and_special_chunks(eng):
    raw = T.random_patterns()
    want, t = T.expected_chunk(raw, 4, 20)
    assert want[2] & 0x02 and len(want) == 49184 and want[32:] == t.tobytes()      # the oracle's chunk is memcpyed
    p = hip_cparams(4, 20)
    assert eng.compress_host(p, raw, [raw.size], [raw.size + 32])[0] == want
    assert device_compress(eng, p, raw) == want
    want0, _ = T.expected_chunk(raw, 4, 20, clevel=0)                               # memcpyed up front
    assert eng.compress_host(hip_cparams(4, 20, clevel=0), raw, [raw.size], [raw.size + 32])[0] == want0
    assert device_compress(eng, hip_cparams(4, 20, clevel=0), raw) == want0
    tiny = np.zeros(65536, np.uint8)
    tiny[::4] = 1                                                                   # every set bit is zeroed: special-zero
    wantz, tz = T.expected_chunk(tiny, 4, 12)
    assert not tz.any() and len(wantz) == 32
    assert eng.compress_host(hip_cparams(4, 12), tiny, [tiny.size], [tiny.size + 32])[0] == wantz
    assert device_compress(eng, hip_cparams(4, 12), tiny) == wantz


def test_a_batch_of_uneven_chunks_device_and_two_step(eng):
    """several chunks of one call at offsets that are no multiple of 16, one of them with nbytes % typesize != 0"""
    raw = T.pixels("natural", np.float32)
    cuts = [0, 65536 + 4, 65536 + 4 + 40000, raw.size - 3]
    nb = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    want = [T.expected_chunk(raw[a:a + n], 4, 12)[0] for a, n in zip(cuts, nb)]
    p = hip_cparams(4, 12)
    assert eng.compress_host(p, raw[:cuts[-1]], nb, [n + 32 for n in nb]) == want
    d_raw, d_comp = eng.alloc(raw.size + 64), eng.alloc(3 * (70000 + 64))
    d_raw.upload(raw)
    off = [0, 70016, 140032]
    cb = eng.compress_device(p, d_raw.ptr, cuts[:-1], nb, d_comp.ptr, off, [n + 32 for n in nb])
    out = d_comp.download()
    assert [out[o:o + c].tobytes() for o, c in zip(off, cb)] == want
    eng.compress_device_begin(p, d_raw.ptr, cuts[:-1], nb, d_comp.ptr, off, [n + 32 for n in nb])
    cb = eng.compress_device_fetch(3)
    out = d_comp.download()
    assert [out[o:o + c].tobytes() for o, c in zip(off, cb)] == want
    # packed: the staging area, then the chunks back to back
    cb = eng.compress_device_packed_begin(p, d_raw.ptr, cuts[:-1], nb, [n + 32 for n in nb])
    poff = np.concatenate([[0], np.cumsum(cb)[:-1]]).astype(np.int64)
    eng.compress_device_packed_fetch(3, d_comp.ptr, poff)
    out = d_comp.download()
    assert [out[o:o + c].tobytes() for o, c in zip(poff, cb)] == want
    assert np.array_equal(d_raw.download(raw.size), raw), "the caller's pixels were modified"
    d_raw.free(); d_comp.free()


@pytest.mark.parametrize("code", [O.LZ4, O.BLOSCLZ])
@pytest.mark.parametrize("dtype,ts,m", T.DTYPES)
def test_interleaved_route(eng, code, dtype, ts, m):
    """cimg_compress_batch_host_interleaved_begin: the pixels are split into planes in the engine's staging area and truncated there,
    in place; every chunk equals the oracle on the truncated plane it covers (three channels of 512 x 40: chunks of 65 536 bytes and
    a shorter last one per plane)"""
    L = hip.load()
    npix = 512 * 40
    planes = [T.pixels(fam, dtype, 512, 96)[k * 7 * ts:][:npix * ts] for k, fam in enumerate(("tiled", "natural", "tiled"))]
    inter = np.ascontiguousarray(np.stack([p.reshape(npix, ts) for p in planes], axis=1)).ravel()
    stride = (npix * ts + 15) & ~15
    raw_off, nb = [], []
    for c in range(3):
        for o in range(0, npix * ts, 65536):
            raw_off.append(c * stride + o)
            nb.append(min(65536, npix * ts - o))
    want = [T.expected_chunk(planes[ro // stride][ro % stride:][:n], ts, m, compcode=code)[0] for ro, n in zip(raw_off, nb)]
    p = hip_cparams(ts, m, code)
    ro, nbv, ds = hip._i64(raw_off), hip._i32(nb), hip._i32([n + 32 for n in nb])
    cb = np.zeros(len(nb), np.int32)
    eng._check(L.cimg_compress_batch_host_interleaved_begin(eng.handle, C.byref(p), 3, npix, hip._ptr(inter), len(nb), hip._ptr(ro), hip._ptr(nbv),
                                                            hip._ptr(ds), hip._ptr(cb)))
    assert cb.tolist() == [len(w) for w in want]
    off = hip._i64(np.arange(len(nb)) * (65536 + 64))
    out = np.zeros(len(nb) * (65536 + 64), np.uint8)
    L.cimg_compress_batch_host_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    eng._check(L.cimg_compress_batch_host_fetch(eng.handle, len(nb), hip._ptr(out), hip._ptr(off)))
    assert [out[o:o + c].tobytes() for o, c in zip(off, cb)] == want


@pytest.mark.parametrize("code", [hip.ZSTD, hip.LZ4HC])
@pytest.mark.parametrize("dtype,ts,m", T.DTYPES)
def test_format_valid_codecs_round_trip_to_truncated_pixels(eng, code, dtype, ts, m):
    raw = T.pixels("natural", dtype)
    t = T.trunc(raw, ts, m)
    p = hip_cparams(ts, m, code)
    (c,) = eng.compress_host(p, raw, [raw.size], [raw.size + 32])
    assert len(c) > 32 and c[20] == 4 and c[28] == m & 0xFF
    assert device_compress(eng, p, raw) == c
    outs, st = eng.decompress_host([c])
    assert st[0] == 0 and np.array_equal(outs[0], t)
    if code != hip.ZSTD or O.zstd_available():                 # the checker's decoders: its LZ4 reader, the box's libzstd
        r, back = O.decompress(c)
        assert r == raw.size and np.array_equal(back, t)
    # compress(trunc(x)) == compress(x)
    assert eng.compress_host(p, t, [t.size], [t.size + 32])[0] == c


def test_wide_route(eng):
    """unfiltered 128 KiB blocks are single streams beyond the normal encoder (and beyond the oracle's, which writes byU16 streams
    only): cimg_encode_wide behind the same pass.  NO BYTE-EXACT ORACLE exists for these streams, so the real check is the pixel
    comparison: the checker's own decoder reads the chunk back to trunc(x).  The byte comparison beside it is against code under test
    (the engine's compress of numpy-truncated pixels without the filter, but for the two header bytes) and only says that the pass
    changes nothing else."""
    raw = T.pixels("tiled", np.float32, 512, 256)
    t = T.trunc(raw, 4, 12)
    p = hip_cparams(4, 12, filt=hip.NOFILTER, blocksize=131072)
    eng.enable_timing(1)
    eng.reset_timing()
    (host,) = eng.compress_host(p, raw, [raw.size], [raw.size + 32])
    wide, passes = eng.kernel_time(hip.K_ENCODE_WIDE)[1], eng.kernel_time(hip.K_TRUNC_PREC)[1]
    eng.enable_timing(0)
    assert wide >= 1 and passes >= 1
    assert len(host) > 32 and host[20] == 4 and host[28] == 12
    r, back = O.decompress(host)
    assert r == raw.size and np.array_equal(back, t)
    (plain,) = eng.compress_host(hip.cparams(4, filters=(0, 0, 0, 0, 0, 0), blocksize=131072), t, [t.size], [t.size + 32])
    assert host == plain[:20] + bytes([4]) + plain[21:28] + bytes([12]) + plain[29:]
    assert device_compress(eng, p, raw) == host
    outs, st = eng.decompress_host([host])
    assert st[0] == 0 and np.array_equal(outs[0], t)


@pytest.mark.parametrize("lead", [1, 3, 7, 13])
def test_callers_buffer_at_an_odd_offset_is_left_alone(eng, lead):
    raw = T.pixels("natural", np.float32)[:100000 + lead]
    want, _ = T.expected_chunk(raw, 4, -15)
    assert device_compress(eng, hip_cparams(4, -15), raw, lead=lead) == want


def test_invalid_meta_is_refused_and_the_engine_stays_usable(eng):
    raw = T.pixels("tiled", np.float32)
    want, _ = T.expected_chunk(raw, 4, 12)
    for ts, m in ((4, 0), (4, 24), (4, -23), (4, -128), (2, 11), (8, 53), (8, -52), (1, 3), (3, 2), (16, 4)):
        n = raw.size // ts * ts
        with pytest.raises(hip.CodecError) as ei:
            eng.compress_host(hip_cparams(ts, m), raw[:n], [n], [n + 32])
        assert ei.value.code == ERR_INVALID_PARAM, (ts, m)
        with pytest.raises(hip.CodecError) as ei:
            device_compress(eng, hip_cparams(ts, m), raw[:n])
        assert ei.value.code == ERR_INVALID_PARAM, (ts, m)
        assert eng.compress_host(hip_cparams(4, 12), raw, [raw.size], [raw.size + 32])[0] == want
    # a misplaced filter stays CODEC_SUPPORT
    for filters in ((0, 0, 0, 0, 0, 4), (4, 0, 0, 0, 0, 1), (0, 0, 0, 4, 0, 1), (1, 0, 0, 0, 4, 1)):
        with pytest.raises(hip.CodecError) as ei:
            eng.compress_host(hip.cparams(4, filters=filters), raw, [raw.size], [raw.size + 32])
        assert ei.value.code == -7, filters


def test_no_pass_without_the_filter(eng):
    raw = T.pixels("tiled", np.float32)
    eng.enable_timing(1)
    eng.reset_timing()
    eng.compress_host(hip.cparams(4), raw, [raw.size], [raw.size + 32])
    n = eng.kernel_time(hip.K_TRUNC_PREC)[1]
    eng.compress_host(hip_cparams(4, 12), raw, [raw.size], [raw.size + 32])
    m = eng.kernel_time(hip.K_TRUNC_PREC)[1]
    eng.enable_timing(0)
    assert n == 0 and m == 1


# ---- read side: oracle-written chunks whose header names the filter ------------------------------------------------------------

def oracle_set(dtype, ts, m, code=O.LZ4, chunk_bytes=65536, height=96):
    t = T.trunc(T.pixels("tiled", dtype, 512, height), ts, m)
    return t, oracle_chunks(T.oracle_cparams(ts, m, compcode=code), t, chunk_bytes)


@pytest.mark.parametrize("code", [O.LZ4, O.BLOSCLZ, O.LZ4HC, O.ZSTD])
@pytest.mark.parametrize("dtype,ts,m", [(np.float32, 4, 12), (np.float16, 2, 5), (np.float64, 8, 30)])
def test_read_batch_windows_strided_getitem(eng, code, dtype, ts, m):
    if code == O.ZSTD and not O.zstd_available():
        pytest.skip("no libzstd for the checker to write zstd chunks with")
    t, chunks = oracle_set(dtype, ts, m, code)
    assert all(c[20] == 4 and c[28] == m for c in chunks)
    outs, st = eng.decompress_host(chunks)
    assert not st.any() and np.array_equal(np.concatenate(outs), t)
    elems = t.size // ts
    specs, size = pack([dict(chunk_first=0, chunk_count=len(chunks), origin=40 * 512 + 100, row_pitch=512, width=64, height=40),
                        dict(chunk_first=0, chunk_count=len(chunks), origin=0, row_pitch=elems, width=elems, height=1)], ts)
    want = win_expected([t, t], specs, ts, size)
    out = np.full(size, CANARY, np.uint8)
    eng.decompress_windows_host(chunks, specs, out)
    assert np.array_equal(out, want)
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp, d_out = eng.alloc(buf.size), eng.alloc(size)
    d_comp.upload(buf)
    d_out.upload(np.full(size, CANARY, np.uint8))
    eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs)
    assert np.array_equal(d_out.download(), want)
    # strided: every third element of every second row
    s = dict(chunk_first=0, chunk_count=len(chunks), origin=5 * 512 + 7, row_pitch=1024, col_pitch=3, width=150, height=40,
             out_off=5, out_pitch=150 * ts + 9)
    ssize = 5 + 40 * s["out_pitch"] + 64
    swant = np.full(ssize, CANARY, np.uint8)
    el = t.reshape(-1, ts)
    for r in range(40):
        row = el[s["origin"] + r * 1024:][:450:3]
        swant[5 + r * s["out_pitch"]:][:150 * ts] = row.reshape(-1)
    sout = np.full(ssize, CANARY, np.uint8)
    eng.decompress_windows_host(chunks, [s], sout, strided=True)
    assert np.array_equal(sout, swant)
    d_out2 = eng.alloc(ssize)
    d_out2.upload(np.full(ssize, CANARY, np.uint8))
    eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, [s], d_out2.ptr, comp_size=cs, strided=True)
    assert np.array_equal(d_out2.download(), swant)
    d_comp.free(); d_out.free(); d_out2.free()
    # blosc2_decompress_ctx / blosc2_getitem_ctx
    L = hip.load()
    dctx = L.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    try:
        c = chunks[1]
        src = np.frombuffer(c, np.uint8)
        n = int(nb[1])
        full = np.zeros(n, np.uint8)
        assert L.blosc2_decompress_ctx(dctx, hip._ptr(src), len(c), hip._ptr(full), n) == n
        assert np.array_equal(full, t[65536:65536 + n])
        for start, k in ((0, 1), (1234, 3000), (n // ts - 3, 3)):
            dest = np.full(k * ts + 16, CANARY, np.uint8)
            assert L.blosc2_getitem_ctx(dctx, hip._ptr(src), len(c), start, k, hip._ptr(dest), k * ts + 16) == k * ts
            assert np.array_equal(dest[:k * ts], full[start * ts:(start + k) * ts]) and (dest[k * ts:] == CANARY).all()
    finally:
        L.blosc2_free_ctx(dctx)


def test_shim_compresses_with_the_filter(eng):
    L = hip.load()
    raw = T.pixels("natural", np.float32)
    want, t = T.expected_chunk(raw, 4, 12)
    cp = hip.Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = hip.LZ4, 9, 4, 1, 32768, 3
    cp.filters[4], cp.filters_meta[4], cp.filters[5] = 4, 12, 1
    cctx = L.blosc2_create_cctx(cp)
    try:
        dest = np.zeros(raw.size + 32, np.uint8)
        r = L.blosc2_compress_ctx(cctx, hip._ptr(raw.copy()), raw.size, hip._ptr(dest), dest.size)
        assert r == len(want) and dest[:r].tobytes() == want
    finally:
        L.blosc2_free_ctx(cctx)
    cp.filters_meta[4] = 0
    cctx = L.blosc2_create_cctx(cp)
    try:
        assert L.blosc2_compress_ctx(cctx, hip._ptr(raw.copy()), raw.size, hip._ptr(dest), dest.size) == ERR_INVALID_PARAM
    finally:
        L.blosc2_free_ctx(cctx)


def test_truncated_chunks_stay_on_the_lean_path():
    """float16 with the low mantissa byte zeroed (m = 2): the low plane of every block is a run, the high one coded -- the lean
    kernel's case.  The same pixels written without the filter byte are the yardstick: naming the filter must not send one more
    block to the general decoder."""
    t = T.trunc(T.pixels("tiled", np.float16, 512, 128), 2, 2)
    left = {}
    for named in (False, True):
        p = T.oracle_cparams(2, 2) if named else O.cparams(2)
        chunks = oracle_chunks(p, t, 65536)
        assert all(c[20] == (4 if named else 0) for c in chunks)
        e = hip.Engine(0)
        for _ in range(3):
            outs, st = e.decompress_host(chunks)
            assert not st.any() and np.array_equal(np.concatenate(outs), t)
        left[named] = e.decode_stats()
        e.close()
    assert left[True]["lean_batches"] == left[False]["lean_batches"] > 0
    assert left[True]["blocks_total"] == left[False]["blocks_total"] > 0
    assert left[True]["blocks_left_to_general"] == left[False]["blocks_left_to_general"] < left[True]["blocks_total"]


# ---- window writes ---------------------------------------------------------------------------------------------------------

def run_update_device(eng, p, chunks, specs, src, ds):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    ds = np.asarray(ds, np.int32)
    new_off = np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64)[:-1]]).astype(np.int64)
    total = int(new_off[-1]) + int(ds[-1]) + 64
    d_comp, d_src, d_new = eng.alloc(buf.size), eng.alloc(max(src.size, 1)), eng.alloc(total)
    d_comp.upload(buf)
    d_src.upload(src)
    d_new.upload(np.full(total, 0x5A, np.uint8))
    rc, ncb, st = eng.update_windows_device(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr, d_new.ptr, new_off, comp_size=cs, check=False)
    out = d_new.download()
    assert np.array_equal(d_src.download(src.size), src), "the caller's window source was modified"
    d_comp.free(); d_src.free(); d_new.free()
    return rc, st, [out[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]


@pytest.mark.parametrize("height,rows", [(130, 64), (96, 56)])
@pytest.mark.parametrize("code,clevel", [(O.LZ4, 9), (O.BLOSCLZ, 9), (O.ZSTD, 5), (O.LZ4, 0)])
def test_window_write(eng, height, rows, code, clevel):
    """splice route (lz4, blosclz) and whole route (zstd, memcpyed chunks): each new chunk is the from-scratch compress of (old pixels
    with the window written in), truncated.  lz4 / blosclz: the oracle's bytes.  zstd: NO BYTE-EXACT ORACLE exists for the engine's
    frames, so its expected bytes come from code under test and the real check is the last one -- the new chunks decode to the
    edited pixels, truncated."""
    if code == O.ZSTD and not O.zstd_available():
        pytest.skip("no libzstd for the checker to write zstd chunks with")
    ts, m = 4, 12
    t = T.trunc(T.pixels("tiled", np.float32, 512, height), ts, m)
    po = T.oracle_cparams(ts, m, compcode=code, clevel=clevel)
    p = hip_cparams(ts, m, code, clevel=clevel)
    chunks = oracle_chunks(po, t, 65536)
    ds = [65536 + 32] * len(chunks)
    specs, src = ww_source([dict(chunk_first=0, chunk_count=len(chunks), origin=40 * 512 + 100, row_pitch=512, width=64, height=rows)], ts)
    if code == O.ZSTD:             # no byte-exact oracle for the engine's zstd frames: its own compress of numpy-truncated pixels
        compress = lambda raw, d: eng.compress_host(hip.cparams(ts, compcode=code, clevel=clevel), T.trunc(raw, ts, m), [raw.size], [d])[0]
    else:
        compress = lambda raw, d: O.compress(po, T.trunc(raw, ts, m), destsize=d)[1]
    want, edited = ww_expected(None, chunks, specs, ts, src, ds, compress=compress)
    if code == O.ZSTD:             # ... which carries no filter byte: patch the two header bytes in
        want = [None if c is None else c[:20] + bytes([4]) + c[21:28] + bytes([m]) + c[29:] for c in want]
    assert sum(c is not None for c in want) == (3 if height == 130 else 2)
    rc, st, new = run_update_device(eng, p, chunks, specs, src, ds)
    assert rc == 0 and not st.any(), (rc, st, eng.last_error())
    assert new == want, "device call"
    stats = eng.update_stats()
    assert (stats["chunks_whole"] == 0) == (code != O.ZSTD and clevel != 0)
    new, st = eng.update_windows_host(p, chunks, ds, specs, src)
    assert not st.any() and new == want, "host call"
    # the new chunks decode to the edited pixels, truncated
    merged = [n if n is not None else c for n, c in zip(new, chunks)]
    outs, st = eng.decompress_host(merged)
    assert not st.any() and np.array_equal(np.concatenate(outs), T.trunc(edited[0], ts, m))


def test_window_write_with_disagreeing_cparams_is_invalid_param(eng):
    ts, m = 4, 12
    t = T.trunc(T.pixels("tiled", np.float32, 512, 130), ts, m)
    chunks = oracle_chunks(T.oracle_cparams(ts, m), t, 65536)
    plain = oracle_chunks(O.cparams(ts), t, 65536)
    ds = [65536 + 32] * len(chunks)
    specs, src = ww_source([dict(chunk_first=0, chunk_count=len(chunks), origin=40 * 512 + 100, row_pitch=512, width=64, height=64)], ts)
    for p, cs in ((hip_cparams(ts, 11), chunks), (hip_cparams(ts, -11), chunks), (hip.cparams(ts), chunks), (hip_cparams(ts, m), plain),
                  (hip_cparams(ts, 0), chunks)):
        rc, st, new = run_update_device(eng, p, cs, specs, src, ds)
        assert rc == ERR_INVALID_PARAM and all(n is None for n in new)
        rc, new, st = eng.update_windows_host(p, cs, ds, specs, src, check=False)
        assert rc == ERR_INVALID_PARAM and all(n is None for n in new)
    rc, st, new = run_update_device(eng, hip_cparams(ts, m), chunks, specs, src, ds)       # -11 zeroes 11 bits like 12 kept: the META differs
    assert rc == 0 and not st.any()
