"""Typed windows (csrc/window_plan.h: run_windows_typed; csrc/window_kernel.h: TypedWindowBlock) on the host lane emulator.

tests/emu/window_typed_emu.cpp (which includes the grouped, strided and plain window emulators), emu.cpp and wide_emu.cpp are
compiled into a library in a pytest temp directory (_windows_typed.build_emu, -ffp-contract=off).  Every element of every window
is compared bit for bit with numpy's two-ufunc conversion of the oracle's decode (NaN where numpy gives NaN), every other byte of
the output must keep its canary, and blocks_decoded must equal the brute-force count of distinct blocks.  Planner, grouping, unit
order and kernel body run once more in a stand-alone AddressSanitizer / UBSan program (tests/emu/window_typed_asan_main.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import _windows_grouped as G
import _windows_typed as T
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, plane_of, sizes
from _windows_grouped import LZ4, ZSTD, H, W, rect
from _windows_strided import swindows
from _windows_typed import F16, F32, F64, I8, I16, I32, U8, U16, U32  # noqa: F401


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return T.build_emu(tmp_path_factory.mktemp("window_typed_emu"))


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return T.build_emu(tmp_path_factory.mktemp("window_typed_asan"), sanitize=True)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def engine_chunks(L, ts, raw, chunk_bytes, compcode=LZ4, clevel=5, blocksize=8192, splitmode=3, filt=1):
    """raw cut into chunks and compressed by the emulated engine kernels -> list of bytes"""
    p = G.EmuCParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    nb = np.array([min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)], np.int32)
    n = nb.size
    raw_off = np.concatenate([[0], np.cumsum(nb[:-1])]).astype(np.int64)
    dest = (nb + 96).astype(np.int32)
    comp_off = np.concatenate([[0], np.cumsum(dest[:-1].astype(np.int64))]).astype(np.int64)
    comp = np.zeros(int(dest.sum()) + 64, np.uint8)
    cb = np.zeros(n, np.int32)
    rc = L.wemu_compress_batch(C.byref(p), n, _p(np.ascontiguousarray(raw)), _p(raw_off), _p(nb), _p(comp), _p(comp_off), _p(dest), _p(cb))
    assert rc == 0, rc
    return [comp[comp_off[i]:comp_off[i] + cb[i]].tobytes() for i in range(n)]


def zstd_by(L):
    return lambda ts, raw, bsize: engine_chunks(L, ts, raw, raw.size, compcode=ZSTD, blocksize=bsize)[0]


def call(L, chunks, specs, ts, size, grouped=False, nbytes=None, blocksize=None, order=0):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    out = np.full(size, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    L.emu_set_write_order(order)
    try:
        if grouped:
            rc = L.wnemu_windows_grouped_device(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), ts, len(specs), swindows(specs), _p(out), _p(st))
        else:
            rc = L.wnemu_windows_typed_device(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), ts, len(specs), T.twindows(specs), _p(out),
                                              _p(st))
    finally:
        L.emu_set_write_order(0)
    stats = np.zeros(3, np.int64)
    L.wnemu_window_stats(_p(stats))
    return rc, st, out, stats


def check(L, chunks, values, specs, ts, whole=False, orders=(0,)):
    nb, bs = sizes(chunks)
    specs, size = T.pack_typed(specs)
    distinct = G.touched_blocks(specs, nb, bs, ts)
    for order in orders:
        rc, st, out, stats = call(L, chunks, specs, ts, size, order=order)
        assert rc == 0 and not st.any(), (rc, st)
        T.check_output(out, [values] * len(specs) if isinstance(values, np.ndarray) else values, specs)
        if whole:
            assert stats[0] == 0 and stats[1] == len({c for c, _ in distinct})
        else:
            assert stats[0] == len(distinct) and stats[1] == 0, (stats, len(distinct))
    return specs, size


@pytest.mark.parametrize("out", [F32, F16])
@pytest.mark.parametrize("src", [U8, I8, U16, I16, U32, I32, F16, F32, F64])
def test_every_source_type(L, src, out):
    """the matrix windows -- tiles, overlaps, col_pitch 3 with row_pitch 2 rows, the whole plane, 1 x 1, empty -- over oracle chunks
    (lz4 + shuffle, several chunks, leftover blocks), every scale / offset pair and elem_pitch of 1, 3 and 4 output sizes"""
    ts = T.SIZE[src]
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(src)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), T.raw_of(v), cbytes)
    nb, bs = sizes(chunks)
    assert len(chunks) >= 3 and sum(-(-int(n) // int(b)) for n, b in zip(nb, bs)) >= 9
    assert np.array_equal(plane_of(chunks), T.raw_of(v))
    rects = G.matrix_windows(len(chunks)) + [rect(7, 3, 300, 100, 3, 2, nchunks=len(chunks))]
    check(L, chunks, v, T.dress(rects, src, out, k0=src), ts, orders=(0, 1, 2) if src in (U8, F16, F64) else (0,))


def test_rows_that_begin_mid_block(L):
    """typesize 1, plane rows of 100 elements: 4096-byte blocks begin mid-row, window rows cross block and chunk borders"""
    v = T.plane(U8)
    chunks = oracle_chunks(O.cparams(1, clevel=5, blocksize=4096), T.raw_of(v), 16384)
    n = len(chunks)
    rows = v.size // 100
    rects = [rect(0, 0, 100, rows, nchunks=n, row_len=100), rect(13, 30, 80, 200, nchunks=n, row_len=100), rect(5, 7, 90, 400, 3, 2, nchunks=n, row_len=100),
             rect(99, rows - 1, 1, 1, nchunks=n, row_len=100), rect(60, 160, 40, 10, nchunks=n, row_len=100)]
    check(L, chunks, v, T.dress(rects, U8, F32), 1, orders=(0, 2))
    check(L, chunks, v, T.dress(rects, U8, F16, k0=3), 1)


@pytest.mark.parametrize("src", [U8, I16, U32, F16, F32, F64])
def test_identity_keeps_every_bit_and_equals_the_grouped_call(L, src):
    """out_type == src_type, scale 1, offset 0: NaN payloads and -0 survive (compared as bits, no NaN allowance); with elem_pitch ==
    typesize the bytes, status and stats are the grouped call's"""
    ts = T.SIZE[src]
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(src)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), T.raw_of(v), cbytes)
    rects = G.matrix_windows(len(chunks))
    dense = [T.typed(r, src, src) for r in rects]
    specs, size = check(L, chunks, v, dense, ts, orders=(0, 1))
    rc, st, out, stats = call(L, chunks, specs, ts, size)
    plain = [{k: s[k] for k, _ in T.StridedWindow._fields_} for s in specs]
    for s in plain:                                                          # (the grouped call wants dense rows even for one row)
        assert s["out_pitch"] >= s["width"] * ts
    rc0, st0, out0, stats0 = call(L, chunks, plain, ts, size, grouped=True)
    assert rc == rc0 == 0 and np.array_equal(st, st0) and np.array_equal(out, out0) and np.array_equal(stats, stats0)
    check(L, chunks, v, [T.typed(r, src, src, pitch_mult=(3, 4)[k % 2]) for k, r in enumerate(rects)], ts)


@pytest.mark.parametrize("src,out", [(U16, F32), (F32, F16), (F16, F32), (F64, F32), (U8, F16), (F32, F32)])
def test_every_byte_at_mode(L, src, out):
    ts = T.SIZE[src]
    chunks, v = T.modes_chunks(zstd_by(L), src)
    n = len(chunks)
    rects = [rect(0, 0, W, 128, nchunks=n), rect(5, 3, 400, 120, 3, 2, nchunks=n), rect(100, 14, 50, 100, nchunks=n)]
    rects += [rect(17 * k % W, 16 * k + 15, 9, 2, nchunks=n) for k in range(7)]          # the border of every two chunks
    nb, bs = sizes(chunks)
    specs, size = T.pack_typed(T.dress(rects, src, out) + [T.typed(r, src, src, pitch_mult=2) for r in rects[:2]])
    for order in (0, 1):
        rc, st, outb, stats = call(L, chunks, specs, ts, size, order=order)
        assert rc == 0 and not st.any()
        T.check_output(outb, [v] * len(specs), specs)
        assert stats[1] == 1 and stats[0] == len({cb for cb in G.touched_blocks(specs, nb, bs, ts) if cb[0] != 7})


def test_wide_block_chunk(L):
    """one chunk of one 256 KiB block: decoded whole, the windows cut from it (copy mode)"""
    v = T.plane(I16, 128 * 1024, seed=2)
    chunks = engine_chunks(L, 2, T.raw_of(v), 262144, compcode=LZ4, blocksize=262144)
    nb, bs = sizes(chunks)
    assert len(chunks) == 1 and bs[0] == 262144
    rects = [rect(3, 1, 500, 250, 7, 5, nchunks=1), rect(0, 255, W, 1, nchunks=1), rect(100, 100, 64, 64, nchunks=1)]
    check(L, chunks, v, T.dress(rects, I16, F32) + T.dress(rects, I16, F16, k0=2), 2, whole=True)


def test_pixel_major_batch_of_overlapping_regions(L):
    """three channels with their own scale and offset, a batch of overlapping crops written as (N, oh, ow, C) float32 in one call:
    every slot exact, nothing else written, one block staged per distinct block; and the launch visits the units in the order of the
    addresses they write, so the three channels of a block position are neighbours in the grid"""
    vals, chunks, n = T.three_planes()
    nb, bs = sizes(chunks)
    regions = [(10, 5, 200, 60, 1, 1), (100, 20, 224, 64, 1, 1), (100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5), (W - 1, H - 1, 1, 1, 1, 1),
               (0, 0, W, H, 2, 3)]
    scales, offsets = (1 / 255, 1 / 58.395, -0.4851), (-0.485, 0.406, 3.0e-41)
    for out in (F32, F16):
        specs, size = T.pixel_major(regions, n, U8, out, scales, offsets)
        rc, st, outb, stats = call(L, chunks, specs, 1, size, order=1)
        assert rc == 0 and not st.any()
        T.check_output(outb, [vals[k % 3] for k in range(len(specs))], specs)
        assert stats[0] == len(G.touched_blocks(specs, nb, bs, 1)) and stats[1] == 0
    first = np.zeros(4096, np.int64)
    k = L.wnemu_typed_unit_order(len(chunks), _p(nb), _p(bs), 1, len(specs), T.twindows(specs), _p(first), first.size)
    assert k == stats[0] and (np.diff(first[:k]) >= 0).all()
    one, _ = T.pixel_major(regions[:1], n, U8, F32, scales, offsets)
    k = L.wnemu_typed_unit_order(len(chunks), _p(nb), _p(bs), 1, 3, T.twindows(one), _p(first), first.size)
    assert k % 3 == 0 and all(first[i + 1] - first[i] == 4 and first[i + 2] - first[i] == 8 for i in range(0, k, 3))


def test_empty_calls(L):
    vals, chunks, n = T.three_planes()
    specs, size = T.pack_typed([T.typed(rect(5, 5, 0, 4, nchunks=n), U8, F32), T.typed(rect(5, 5, 4, 0, 2, 3, nchunks=n), U8, F16, 2.0)])
    rc, st, out, stats = call(L, chunks, specs, 1, size)
    assert rc == 0 and not st.any() and (out == CANARY).all() and not stats.any()
    rc, st, out, stats = call(L, chunks, [], 1, 64)
    assert rc == 0 and (out == CANARY).all() and not stats.any()


I64, I32MAX = 2 ** 63 - 1, 2 ** 31 - 1


def test_refusals_leave_the_engine_usable(L):
    ts = 2
    cbytes, bsize = G.GEOMETRY[ts]
    v = T.plane(U16)
    chunks = oracle_chunks(O.cparams(ts, blocksize=bsize), T.raw_of(v), cbytes)
    n = len(chunks)
    ok = dict(T.typed(rect(10, 10, 80, 20, 4, 2, nchunks=n), U16, F32, 0.5, 1.0, pitch_mult=3), out_off=8, out_pitch=20 * 12)
    good, size = [ok], 8 + 10 * 240 + 64
    bad = [dict(ok, elem_pitch=3), dict(ok, elem_pitch=0), dict(ok, elem_pitch=-4), dict(ok, elem_pitch=6),       # < size; misaligned
           dict(ok, out_pitch=19 * 12 + 3), dict(ok, out_pitch=19 * 12), dict(ok, out_pitch=242), dict(ok, elem_pitch=I64 // 4 * 4, out_pitch=I64 // 4 * 4),
           dict(ok, src_type=9), dict(ok, src_type=-1), dict(ok, out_type=9), dict(ok, out_type=-1),
           dict(ok, src_type=U8), dict(ok, src_type=F32), dict(ok, src_type=F64),                                  # not the typesize
           dict(ok, out_type=U16), dict(ok, out_type=I16), dict(ok, out_type=F64, elem_pitch=8, out_pitch=20 * 8), # non-identity integer / F64
           dict(ok, out_type=U16, elem_pitch=2, scale=1.0, offset=0.5), dict(ok, out_type=U8, elem_pitch=1),
           dict(ok, out_off=6), dict(ok, out_off=-4),
           dict(ok, col_pitch=0), dict(ok, row_pitch=19 * 4), dict(ok, origin=-1), dict(ok, width=-1), dict(ok, chunk_count=0),
           dict(ok, chunk_count=I32MAX), dict(ok, origin=W * H - 19 * 4, height=1)]
    for b in bad:
        for specs in ([b], [ok, b]):
            rc, st, out, stats = call(L, chunks, specs, ts, size)
            assert rc == ERR_INVALID_PARAM, (b, rc)
            assert (out == CANARY).all() and not stats.any()                  # nothing run
    # an identity window may have an integer type; one row needs no out_pitch
    for s in (dict(ok, out_type=U16, scale=1.0, offset=0.0, elem_pitch=2), dict(ok, height=1, out_pitch=0)):
        rc, st, out, _ = call(L, chunks, [s], ts, size)
        assert rc == 0
        T.check_output(out, [v], [s])
    # blocks that do not hold whole elements: a plane of typesize 2 in 4097-byte blocks (sizes handed in as the caller states them)
    nb, bs = sizes(chunks)
    rc, st, out, stats = call(L, chunks, good, ts, size, nbytes=nb, blocksize=np.full(n, 4097, np.int32))
    assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
    nb2 = nb.copy()
    nb2[0] -= 1                                                               # a chunk that is not the plane's last ends inside an element
    rc, st, out, stats = call(L, chunks, good, ts, size, nbytes=nb2, blocksize=bs)
    assert rc == ERR_INVALID_PARAM and (out == CANARY).all()
    rc, st, out, _ = call(L, chunks, good, ts, size)
    assert rc == 0 and not st.any()
    T.check_output(out, [v], good)


def case_blob(chunks, specs, ts, size):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    w = T.twindows(specs)
    return b"".join([np.array([len(chunks), ts, size, len(specs)], np.int64).tobytes(), off.tobytes(), cs.tobytes(), nb.tobytes(), bs.tobytes(),
                     bytes(w)[:C.sizeof(T.TypedWindow) * len(specs)], np.array([buf.size], np.int64).tobytes(), buf.tobytes()])


def test_planner_order_and_kernel_under_asan(L, asan_exe, tmp_path):
    """Outputs that end at the last element's last byte (no slack for a store that is too wide): the matrix, pixel-major rows whose
    last slot ends the buffer, every byte_at mode, and refusals.  The sanitizers are the check, with numpy's answer for the bytes."""
    path, outp = tmp_path / "case.bin", tmp_path / "out.bin"

    def run(chunks, specs, ts, size, order=0):
        path.write_bytes(case_blob(chunks, specs, ts, size))
        r = subprocess.run([asan_exe, str(path), str(outp), str(order)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [int(x) for x in r.stdout.split()], np.fromfile(outp, np.uint8)

    def tight(specs):
        specs, _ = T.pack_typed(specs, gap=0, lead=0)
        last = specs[-1]
        return specs, int(T.positions(last).max()) + T.out_size(last) if last["width"] and last["height"] else 64

    for src, out, order in ((U8, F32, 0), (F32, F16, 1), (F64, F32, 2), (I32, F16, 0)):
        ts = T.SIZE[src]
        cbytes, bsize = G.GEOMETRY[ts]
        v = T.plane(src)
        chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize, filters=(0, 0, 0, 0, 0, 1 + order % 2)), T.raw_of(v), cbytes)
        rects = [r for r in G.matrix_windows(len(chunks)) if r["width"] and r["height"]]
        specs, size = tight(T.dress(rects, src, out) + [T.typed(rects[0], src, src)])
        res, got = run(chunks, specs, ts, size, order)
        assert not any(res)
        T.check_output(got, [v] * len(specs), specs)
    vals, chunks, n = T.three_planes()
    specs, size = T.pixel_major([(100, 20, 224, 64, 1, 1), (3, 1, 500, 128, 7, 5)], n, U8, F16, (1 / 255, 0.5, 2.0), (0.0, -1.0, 0.25))
    res, got = run(chunks, specs, 1, size - 64, 1)
    assert not any(res)
    T.check_output(got, [vals[k % 3] for k in range(len(specs))], specs)
    chunks, v = T.modes_chunks(zstd_by(L), F16)
    rects = [rect(0, 0, W, 128, nchunks=len(chunks)), rect(5, 3, 400, 120, 3, 2, nchunks=len(chunks))]
    specs, size = tight(T.dress(rects, F16, F32))
    res, got = run(chunks, specs, 2, size)
    assert not any(res)
    T.check_output(got, [v] * len(specs), specs)
    ok = specs[0]
    for b in (dict(ok, elem_pitch=2), dict(ok, out_type=U16), dict(ok, src_type=F32), dict(ok, width=-1), dict(ok, chunk_count=I32MAX)):
        res, got = run(chunks, [ok, b], 2, size)
        assert res[0] == ERR_INVALID_PARAM and (got == CANARY).all(), b
