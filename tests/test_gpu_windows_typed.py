"""Typed windows on the MI355X: cimg_decompress_windows_typed_device (csrc/window_kernel.h: cimg_decode_window_typed,
csrc/window_plan.h: run_windows_typed).

The cases of tests/test_emu_windows_typed.py at the same small shapes through the real engine.  Every element is compared bit for
bit with numpy's two-ufunc conversion of the decoded plane (NaN where numpy gives NaN); every other byte of the output keeps its
canary; blocks_decoded is the brute-force count of distinct blocks.  Every hostile input here is one the host refuses before
anything is launched."""
import numpy as np
import pytest

import _oracle as O
import _windows_grouped as G
import _windows_typed as T
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from _windows_grouped import LZ4, ZSTD, H, W, rect
from _windows_typed import F16, F32, F64, I8, I16, I32, U8, U16, U32  # noqa: F401
from cimg import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def engine_chunks(eng, ts, raw, chunk_bytes, **kw):
    p = hip.cparams(ts, **kw)
    nb = [min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)]
    chunks = eng.compress_host(p, np.ascontiguousarray(raw), nb, [n + 64 for n in nb])
    assert all(len(c) > 0 for c in chunks)
    return chunks


def zstd_by(eng):
    return lambda ts, raw, bsize: engine_chunks(eng, ts, raw, raw.size, clevel=5, blocksize=bsize, compcode=ZSTD)[0]


def call(eng, chunks, specs, ts, size, grouped=False, nbytes=None, blocksize=None):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    if grouped:
        rc, st = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False, grouped=True)
    else:
        rc, st = eng.decompress_windows_typed_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False)
    stats = eng.window_stats()
    out = d_out.download()
    d_comp.free(); d_out.free()
    return rc, st, out, stats


def check(eng, chunks, values, specs, ts, whole=False):
    nb, bs = sizes(chunks)
    specs, size = T.pack_typed(specs)
    distinct = G.touched_blocks(specs, nb, bs, ts)
    rc, st, out, stats = call(eng, chunks, specs, ts, size)
    assert rc == 0 and not st.any(), (rc, st, eng.last_error())
    T.check_output(out, [values] * len(specs) if isinstance(values, np.ndarray) else values, specs)
    if whole:
        assert stats["blocks_decoded"] == 0 and stats["chunks_whole"] == len({c for c, _ in distinct})
    else:
        assert stats["blocks_decoded"] == len(distinct) and stats["chunks_whole"] == 0, (stats, len(distinct))
    return specs, size


def test_kernel_name_and_one_launch_per_call(eng):
    assert hip.K_DECODE_WINDOW_TYPED == 27 and hip.KERNELS[27] == "cimg_decode_window_typed"
    assert hip.load().cimg_kernel_name(27).decode() == "cimg_decode_window_typed"
    vals, chunks, n = T.three_planes()
    specs, size = T.pixel_major([(10, 5, 200, 60, 1, 1), (100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5)], n, U8, F32, (1 / 255, 0.5, 2.0),
                                (0.0, -1.0, 0.25))
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp, d_out = eng.alloc(buf.size), eng.alloc(size)
    d_comp.upload(buf)
    kinds = (hip.K_DECODE_WINDOW, hip.K_DECODE_WINDOW_STRIDED, hip.K_DECODE_WINDOW_GROUPED, hip.K_DECODE_WINDOW_TYPED)
    eng.enable_timing(1)
    try:
        eng.reset_timing()
        eng.decompress_windows_typed_device(d_comp.ptr, off, nb, bs, 1, specs, d_out.ptr, comp_size=cs)
        assert [eng.kernel_time(k)[1] for k in kinds] == [0, 0, 0, 1]
        assert eng.kernel_time(hip.K_INTERLEAVE)[1] == 0
    finally:
        eng.enable_timing(0)
        d_comp.free(); d_out.free()


@pytest.mark.parametrize("out", [F32, F16])
@pytest.mark.parametrize("src", [U8, I8, U16, I16, U32, I32, F16, F32, F64])
def test_every_source_type(eng, src, out):
    ts = T.SIZE[src]
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(src)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), T.raw_of(v), cbytes)
    rects = G.matrix_windows(len(chunks)) + [rect(7, 3, 300, 100, 3, 2, nchunks=len(chunks))]
    check(eng, chunks, v, T.dress(rects, src, out, k0=src), ts)


def test_not_contracted_subnormals_and_float16_ties(eng):
    """The cases a fused multiply-add gets wrong, each against numpy and against the exact product-then-sum in float64: a product
    that rounds before the sum (uint8 / 255 - 0.4851 differs from the fused result for many v), sums that land on float16 ties,
    float32 subnormal products (3.0e-41 * v) that a flushed multiply would zero, and float16 subnormal results."""
    v8 = np.arange(512 * 8, dtype=np.uint8)
    s, o = np.float32(1 / 255), np.float32(-0.4851)
    two = (v8.astype(np.float32) * s + o)
    fused = (v8.astype(np.float64) * np.float64(s) + np.float64(o)).astype(np.float32)
    assert (two != fused).any()                                              # (the case can tell the two apart)
    chunks = oracle_chunks(O.cparams(1, clevel=5, blocksize=4096), v8, 4096)
    n = len(chunks)
    whole = rect(0, 0, W, 8, nchunks=n)
    specs = [T.typed(whole, U8, F32, 1 / 255, -0.4851), T.typed(whole, U8, F16, 1 / 255, -0.4851), T.typed(whole, U8, F32, 3.0e-41, 0.0),
             T.typed(whole, U8, F16, 2.0 ** -24, 2.0 ** -25), T.typed(whole, U8, F16, 1 / 3, 1 / 2048), T.typed(whole, U8, F32, 0.1, 3.0e-41)]
    specs, size = check(eng, chunks, v8, specs, 1)
    rc, st, out, _ = call(eng, chunks, specs, 1, size)
    got = out[T.positions(specs[0])[..., None] + np.arange(4)].view(np.float32)[..., 0].ravel()
    assert np.array_equal(got.view(np.uint32), two.view(np.uint32))
    sub = out[T.positions(specs[2])[..., None] + np.arange(4)].view(np.float32)[..., 0].ravel()
    assert (sub[v8 > 0] > 0).all() and (sub[v8 > 0] < np.finfo(np.float32).tiny).all()
    f32 = T.plane(F32)[:512 * 16]
    chunks = oracle_chunks(O.cparams(4, clevel=5, blocksize=8192), T.raw_of(f32), 16384)
    whole = rect(0, 0, W, 16, nchunks=len(chunks))
    check(eng, chunks, f32, [T.typed(whole, F32, F16, 1.0, 2.0 ** -11), T.typed(whole, F32, F16, 3.0, 0.0), T.typed(whole, F32, F32, 3.0e-41, 0.0),
                             T.typed(whole, F32, F16, 2.0 ** -14, 0.0), T.typed(whole, F32, F16, 7e4, 0.0)], 4)


def test_rows_that_begin_mid_block(eng):
    v = T.plane(U8)
    chunks = oracle_chunks(O.cparams(1, clevel=5, blocksize=4096), T.raw_of(v), 16384)
    n = len(chunks)
    rows = v.size // 100
    rects = [rect(0, 0, 100, rows, nchunks=n, row_len=100), rect(13, 30, 80, 200, nchunks=n, row_len=100), rect(5, 7, 90, 400, 3, 2, nchunks=n, row_len=100),
             rect(99, rows - 1, 1, 1, nchunks=n, row_len=100), rect(60, 160, 40, 10, nchunks=n, row_len=100)]
    check(eng, chunks, v, T.dress(rects, U8, F32), 1)
    check(eng, chunks, v, T.dress(rects, U8, F16, k0=3), 1)


@pytest.mark.parametrize("src", [U8, I16, U32, F16, F32, F64])
def test_identity_keeps_every_bit_and_equals_the_grouped_call(eng, src):
    ts = T.SIZE[src]
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(src)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), T.raw_of(v), cbytes)
    rects = G.matrix_windows(len(chunks))
    specs, size = check(eng, chunks, v, [T.typed(r, src, src) for r in rects], ts)
    rc, st, out, stats = call(eng, chunks, specs, ts, size)
    plain = [{k: s[k] for k, _ in T.StridedWindow._fields_} for s in specs]
    rc0, st0, out0, stats0 = call(eng, chunks, plain, ts, size, grouped=True)
    assert rc == rc0 == 0 and np.array_equal(st, st0) and np.array_equal(out, out0) and stats == stats0
    check(eng, chunks, v, [T.typed(r, src, src, pitch_mult=(3, 4)[k % 2]) for k, r in enumerate(rects)], ts)


@pytest.mark.parametrize("src,out", [(U16, F32), (F32, F16), (F16, F32), (F64, F32), (U8, F16), (F32, F32)])
def test_every_byte_at_mode(eng, src, out):
    ts = T.SIZE[src]
    chunks, v = T.modes_chunks(zstd_by(eng), src)
    n = len(chunks)
    rects = [rect(0, 0, W, 128, nchunks=n), rect(5, 3, 400, 120, 3, 2, nchunks=n), rect(100, 14, 50, 100, nchunks=n)]
    rects += [rect(17 * k % W, 16 * k + 15, 9, 2, nchunks=n) for k in range(7)]
    nb, bs = sizes(chunks)
    specs, size = T.pack_typed(T.dress(rects, src, out) + [T.typed(r, src, src, pitch_mult=2) for r in rects[:2]])
    rc, st, outb, stats = call(eng, chunks, specs, ts, size)
    assert rc == 0 and not st.any(), eng.last_error()
    T.check_output(outb, [v] * len(specs), specs)
    assert stats["chunks_whole"] == 1
    assert stats["blocks_decoded"] == len({cb for cb in G.touched_blocks(specs, nb, bs, ts) if cb[0] != 7})


def test_wide_block_chunk(eng):
    v = T.plane(I16, 128 * 1024, seed=2)
    chunks = engine_chunks(eng, 2, T.raw_of(v), 262144, clevel=5, blocksize=262144, compcode=LZ4)
    nb, bs = sizes(chunks)
    assert len(chunks) == 1 and bs[0] == 262144
    rects = [rect(3, 1, 500, 250, 7, 5, nchunks=1), rect(0, 255, W, 1, nchunks=1), rect(100, 100, 64, 64, nchunks=1)]
    check(eng, chunks, v, T.dress(rects, I16, F32) + T.dress(rects, I16, F16, k0=2), 2, whole=True)


def test_pixel_major_batch_of_overlapping_regions(eng):
    vals, chunks, n = T.three_planes()
    nb, bs = sizes(chunks)
    regions = [(10, 5, 200, 60, 1, 1), (100, 20, 224, 64, 1, 1), (100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5), (W - 1, H - 1, 1, 1, 1, 1),
               (0, 0, W, H, 2, 3)]
    scales, offsets = (1 / 255, 1 / 58.395, -0.4851), (-0.485, 0.406, 3.0e-41)
    for out in (F32, F16, U8):
        sc, of = (scales, offsets) if out != U8 else ((1.0,) * 3, (0.0,) * 3)                # (uint8: the identity, pixel-major)
        specs, size = T.pixel_major(regions, n, U8, out, sc, of)
        rc, st, outb, stats = call(eng, chunks, specs, 1, size)
        assert rc == 0 and not st.any(), eng.last_error()
        T.check_output(outb, [vals[k % 3] for k in range(len(specs))], specs)
        assert stats["blocks_decoded"] == len(G.touched_blocks(specs, nb, bs, 1)) and stats["chunks_whole"] == 0


def test_empty_calls(eng):
    vals, chunks, n = T.three_planes()
    specs, size = T.pack_typed([T.typed(rect(5, 5, 0, 4, nchunks=n), U8, F32), T.typed(rect(5, 5, 4, 0, 2, 3, nchunks=n), U8, F16, 2.0)])
    rc, st, out, stats = call(eng, chunks, specs, 1, size)
    assert rc == 0 and not st.any() and (out == CANARY).all() and not any(stats.values())
    rc, st, out, stats = call(eng, chunks, [], 1, 64)
    assert rc == 0 and (out == CANARY).all() and not any(stats.values())


I64, I32MAX = 2 ** 63 - 1, 2 ** 31 - 1


def test_refusals_leave_the_engine_usable(eng):
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(U16)
    chunks = oracle_chunks(O.cparams(ts, blocksize=bsize), T.raw_of(v), cbytes)
    n = len(chunks)
    ok = dict(T.typed(rect(10, 10, 80, 20, 4, 2, nchunks=n), U16, F32, 0.5, 1.0, pitch_mult=3), out_off=8, out_pitch=20 * 12)
    good, size = [ok], 8 + 10 * 240 + 64
    bad = [dict(ok, elem_pitch=3), dict(ok, elem_pitch=0), dict(ok, elem_pitch=-4), dict(ok, elem_pitch=6),
           dict(ok, out_pitch=19 * 12 + 3), dict(ok, out_pitch=19 * 12), dict(ok, out_pitch=242), dict(ok, elem_pitch=I64 // 4 * 4, out_pitch=I64 // 4 * 4),
           dict(ok, src_type=9), dict(ok, src_type=-1), dict(ok, out_type=9), dict(ok, out_type=-1),
           dict(ok, src_type=U8), dict(ok, src_type=F32), dict(ok, src_type=F64),
           dict(ok, out_type=U16), dict(ok, out_type=I16), dict(ok, out_type=F64, elem_pitch=8, out_pitch=20 * 8),
           dict(ok, out_type=U16, elem_pitch=2, scale=1.0, offset=0.5), dict(ok, out_type=U8, elem_pitch=1),
           dict(ok, out_off=6), dict(ok, out_off=-4),
           dict(ok, col_pitch=0), dict(ok, row_pitch=19 * 4), dict(ok, origin=-1), dict(ok, width=-1), dict(ok, chunk_count=0),
           dict(ok, chunk_count=I32MAX), dict(ok, origin=W * H - 19 * 4, height=1)]
    for b in bad:
        for specs in ([b], [ok, b]):
            rc, st, out, stats = call(eng, chunks, specs, ts, size)
            assert rc == ERR_INVALID_PARAM, (b, rc)
            assert (out == CANARY).all() and not any(stats.values())          # nothing run
    nb, bs = sizes(chunks)
    rc, st, out, stats = call(eng, chunks, good, ts, size, nbytes=nb, blocksize=np.full(n, 4097, np.int32))
    assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
    nb2 = nb.copy()
    nb2[0] -= 1
    rc, st, out, stats = call(eng, chunks, good, ts, size, nbytes=nb2, blocksize=bs)
    assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
    # a misaligned output address
    buf, off, cs = concat(chunks)
    d_comp, d_out = eng.alloc(buf.size), eng.alloc(size + 8)
    d_comp.upload(buf)
    rc, st = eng.decompress_windows_typed_device(d_comp.ptr, off, nb, bs, ts, good, d_out.ptr + 2, comp_size=cs, check=False)
    assert rc == ERR_INVALID_PARAM
    d_comp.free(); d_out.free()
    for s in (ok, dict(ok, out_type=U16, scale=1.0, offset=0.0, elem_pitch=2), dict(ok, height=1, out_pitch=0)):
        rc, st, out, _ = call(eng, chunks, [s], ts, size)
        assert rc == 0 and not st.any()
        T.check_output(out, [v], [s])
