"""Strided windows (csrc/window_plan.h: plan_windows over StridedWindowSpec; csrc/window_kernel.h: StridedWindowBlock) on the host
lane emulator.

tests/emu/window_strided_emu.cpp (which includes window_emu.cpp), emu.cpp and wide_emu.cpp are compiled here into a library in a pytest temp
directory, with the flags of tests/emu/Makefile; planner and kernel body run once more in an AddressSanitizer / UBSan build
(tests/emu/window_strided_asan_main.cpp) with buffers that end at their last used byte.  Expected pixels are always numpy
indexing into the oracle's decode of the same chunks; every byte outside the sampled elements must keep its canary, and the stats
must equal a brute-force count of the blocks that hold a byte of a sampled element.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _windows as W1
from _windows import CANARY, ERR_INVALID_PARAM, concat, oracle_chunks, pack, plane_of, sizes, standard_windows
from _windows_strided import expected, sampled_blocks, strided_windows, swindows
from cimg import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
BLOSCLZ, LZ4, LZ4HC, ZSTD = 0, 1, 2, 5
FLAGS = ["-std=c++17", "-fPIC", "-Wall", "-Wextra", "-fno-strict-aliasing", "-I", CSRC]
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_strided_emu.cpp")]


class CParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32),
                ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("window_strided_emu") / "libwindow_strided_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, "-o", out])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.wnemu_windows_device.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.wnemu_windows_host.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    lib.wnemu_windows_strided_device.argtypes = lib.wnemu_windows_device.argtypes
    lib.wnemu_windows_strided_host.argtypes = lib.wnemu_windows_host.argtypes
    lib.wnemu_window_stats.argtypes = [vp]
    lib.wemu_compress_batch.argtypes = [C.POINTER(CParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("window_strided_asan") / "window_strided_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                           os.path.join(EMU, "window_strided_asan_main.cpp"), *SOURCES, "-o", out])
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def engine_chunks(L, ts, raw, chunk_bytes, compcode=LZ4, clevel=9, blocksize=8192, splitmode=3, filt=1):
    """raw cut into chunks and compressed by the emulated engine kernels -> list of bytes"""
    p = CParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    nb = np.array([min(chunk_bytes, raw.size - o) for o in range(0, raw.size, chunk_bytes)], np.int32)
    n = nb.size
    raw_off = np.concatenate([[0], np.cumsum(nb[:-1])]).astype(np.int64)
    dest = (nb + 96).astype(np.int32)
    comp_off = np.concatenate([[0], np.cumsum(dest[:-1].astype(np.int64))]).astype(np.int64)
    comp = np.zeros(int(dest.sum()) + 64, np.uint8)
    cb = np.zeros(n, np.int32)
    rc = L.wemu_compress_batch(C.byref(p), n, _p(raw), _p(raw_off), _p(nb), _p(comp), _p(comp_off), _p(dest), _p(cb))
    assert rc == 0, rc
    return [comp[comp_off[i]:comp_off[i] + cb[i]].tobytes() for i in range(n)]


def call(L, chunks, specs, ts, size, host=False, nbytes=None, blocksize=None, old=False):
    """one call; old: the specs are cimg_window and go through the unstrided entry points"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks) if nbytes is None else (nbytes, blocksize)
    out = np.full(size, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    w = W1.windows(specs) if old else swindows(specs)
    if host:
        fn = L.wnemu_windows_host if old else L.wnemu_windows_strided_host
        rc = fn(len(chunks), _p(buf), _p(off), _p(cs), len(specs), w, _p(out), _p(st))
    else:
        fn = L.wnemu_windows_device if old else L.wnemu_windows_strided_device
        rc = fn(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), ts, len(specs), w, _p(out), _p(st))
    stats = np.zeros(3, np.int64)
    L.wnemu_window_stats(_p(stats))
    return rc, st, out, stats


def pixels(ts, elems, seed=0):
    rng = np.random.default_rng(seed)
    base = synth.tiled_channel(np.float16, 64, max(elems * ts // 128 + 1, 1)).view(np.uint8).ravel()
    raw = base[:elems * ts].copy()
    raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)      # some entropy, still compressible
    return raw


def geometry(ts):
    chunk_elems = 13000
    elems = 2 * chunk_elems + 5001                                           # a ragged last chunk
    raw = pixels(ts, elems)
    if ts > 1:
        raw = np.concatenate([raw, np.arange(ts - 1, dtype=np.uint8)])     # ... whose nbytes is no multiple of the typesize
    return raw, chunk_elems * ts, elems, chunk_elems


def check_matrix(L, chunks, ts, elems, chunk_elems, host=False, whole=False):
    nb, bs = sizes(chunks)
    specs, size = pack(strided_windows(elems, chunk_elems, len(chunks), int(bs[0]) // ts), ts)
    rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
    assert rc == 0 and not st.any(), (rc, st)
    want = expected([plane_of(chunks)] * len(specs), specs, ts, size)
    assert np.array_equal(out, want)
    count, touched = sampled_blocks(specs, nb, bs, ts)
    if whole:
        assert stats[0] == 0 and stats[1] == len(touched)
    else:
        assert stats[0] == count and stats[1] == 0
    if host:
        assert stats[2] == sum(len(chunks[i]) for i in touched)
    return stats


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_oracle_chunks(L, codec, ts, filt):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    p = O.cparams(ts, clevel=5, blocksize=8192, compcode=codec, filters=(0, 0, 0, 0, 0, filt))
    chunks = oracle_chunks(p, raw, cbytes)
    for host in (False, True):
        check_matrix(L, chunks, ts, elems, chunk_elems, host=host)


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ, ZSTD])
@pytest.mark.parametrize("ts,filt,split", [(4, 1, 3), (4, 1, 1), (4, 1, 2), (2, 2, 3), (3, 1, 3), (8, 0, 3), (1, 1, 3)])
def test_engine_chunks(L, codec, ts, filt, split):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = engine_chunks(L, ts, raw, cbytes, compcode=codec, clevel=5, splitmode=split, filt=filt)
    for host in (False, True):
        check_matrix(L, chunks, ts, elems, chunk_elems, host=host, whole=codec == ZSTD)   # zstd: the whole route, cut with the stride


def test_memcpyed_and_zero_chunks(L):
    raw, cbytes, elems, chunk_elems = geometry(4)
    chunks = oracle_chunks(O.cparams(4, clevel=0, blocksize=8192), raw, cbytes)             # memcpyed
    for host in (False, True):
        check_matrix(L, chunks, 4, elems, chunk_elems, host=host)
    zeros = np.zeros(raw.size // 4 * 4, np.uint8)                                           # all-zero chunks (special value)
    chunks = engine_chunks(L, 4, zeros, cbytes)
    for host in (False, True):
        check_matrix(L, chunks, 4, zeros.size // 4, chunk_elems, host=host)


def test_256k_blocks_go_the_whole_route(L):
    ts = 4
    raw = pixels(ts, 3 * 65536 + 1000)
    chunks = engine_chunks(L, ts, raw, 262144, compcode=LZ4, blocksize=262144)
    specs, size = pack([dict(chunk_first=0, chunk_count=len(chunks), origin=70000, row_pitch=1000, col_pitch=3, width=300, height=40),
                        dict(chunk_first=0, chunk_count=len(chunks), origin=5, row_pitch=1, col_pitch=65536, width=3, height=1)], ts)
    for host in (False, True):
        rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
        assert rc == 0 and not st.any()
        assert np.array_equal(out, expected([plane_of(chunks)] * 2, specs, ts, size))
        assert stats[0] == 0 and stats[1] == 3                # samples at 5, 65541 and 131077: chunks 0, 1 and 2


def test_several_planes_in_one_call(L):
    ts = 2
    planes, allchunks, specs = [], [], []
    for k in range(3):
        raw = pixels(ts, 20000, seed=k)
        ch = oracle_chunks(O.cparams(ts, blocksize=4096), raw, 16384)
        specs.append(dict(chunk_first=len(allchunks), chunk_count=len(ch), origin=100 * k + 7, row_pitch=200, col_pitch=1 + 2 * k, width=30,
                          height=60))
        allchunks += ch
        planes.append(plane_of(ch))
    specs, size = pack(specs, ts)
    for host in (False, True):
        rc, st, out, _ = call(L, allchunks, specs, ts, size, host=host)
        assert rc == 0 and not st.any()
        assert np.array_equal(out, expected(planes, specs, ts, size))


@pytest.mark.parametrize("ts", [1, 3, 4])
def test_col_pitch_1_equals_the_unstrided_call(L, ts):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=8192), raw, cbytes)
    old, size = pack(standard_windows(elems, 180, chunk_elems, len(chunks)), ts)
    new = [dict(s, col_pitch=1) for s in old]
    for host in (False, True):
        rc0, st0, out0, stats0 = call(L, chunks, old, ts, size, host=host, old=True)
        rc1, st1, out1, stats1 = call(L, chunks, new, ts, size, host=host)
        assert rc0 == 0 and rc1 == 0 and np.array_equal(st0, st1)
        assert np.array_equal(out0, out1)
        assert np.array_equal(stats0, stats1), (stats0, stats1)


def test_selectivity_worked_case(L):
    """8 float16 chunks of 4 MiB (1024 blocks of 32 KiB, 16 777 216 elements); one row, col_pitch 49152 (three blocks), width 342:
    exactly 342 blocks are decoded, and the host call uploads only the chunks that hold one."""
    ts, chunk = 2, 4 << 20
    raw = np.tile(pixels(ts, chunk // ts // 8), 64)
    assert raw.size == 8 * chunk
    chunks = oracle_chunks(O.cparams(ts, clevel=1, blocksize=32768), raw, chunk)
    nb, bs = sizes(chunks)
    assert (bs == 32768).all() and nb.sum() // ts == 16777216
    specs, size = pack([dict(chunk_first=0, chunk_count=8, origin=0, row_pitch=1, col_pitch=49152, width=342, height=1)], ts)
    count, touched = sampled_blocks(specs, nb, bs, ts)
    assert count == 342
    for host in (False, True):
        rc, st, out, stats = call(L, chunks, specs, ts, size, host=host)
        assert rc == 0 and not st.any()
        assert np.array_equal(out, expected([raw], specs, ts, size))
        assert stats[0] == 342 and stats[1] == 0
        if host:
            assert stats[2] == sum(len(chunks[i]) for i in touched)


def test_far_apart_samples_skip_whole_chunks(L):
    raw, cbytes, elems, chunk_elems = geometry(4)
    chunks = oracle_chunks(O.cparams(4, blocksize=8192), raw, cbytes)
    nb, bs = sizes(chunks)
    # chunk 1 is garbage behind its header: samples in chunks 0 and 2 only, so nothing of it may be read, reported or uploaded
    bad = [bytes(c[:32]) + bytes([0xFF]) * (len(c) - 32) if i == 1 else c for i, c in enumerate(chunks)]
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=100, row_pitch=1, col_pitch=2 * chunk_elems + 50, width=2, height=1)], 4)
    for host in (False, True):
        rc, st, out, stats = call(L, bad, specs, 4, size, host=host, nbytes=nb, blocksize=bs)
        assert rc == 0 and not st.any(), st
        assert np.array_equal(out, expected([plane_of(chunks)], specs, 4, size))
        assert stats[0] == 2 and stats[1] == 0
        if host:
            assert stats[2] == len(chunks[0]) + len(chunks[2])


def test_zero_sized_window_is_a_no_op(L):
    raw, cbytes, elems, chunk_elems = geometry(2)
    chunks = oracle_chunks(O.cparams(2, blocksize=8192), raw, cbytes)
    specs, size = pack([dict(chunk_first=0, chunk_count=3, origin=5, row_pitch=10, col_pitch=3, width=0, height=4),
                        dict(chunk_first=0, chunk_count=3, origin=5, row_pitch=10, col_pitch=3, width=4, height=0)], 2)
    for host in (False, True):
        rc, st, out, stats = call(L, chunks, specs, 2, size, host=host)
        assert rc == 0 and not st.any() and (out == CANARY).all() and stats[0] == 0


I64, I32 = 2 ** 63 - 1, 2 ** 31 - 1


def invalid_cases(elems, ts):
    ok = dict(chunk_first=0, chunk_count=3, origin=10, row_pitch=100, col_pitch=4, width=20, height=5, out_off=0, out_pitch=20 * ts)
    bad = [
        dict(ok, col_pitch=0),
        dict(ok, col_pitch=-1),
        dict(ok, col_pitch=-I64),
        dict(ok, col_pitch=0, width=0),                       # col_pitch is checked before the window is found empty
        dict(ok, row_pitch=19 * 4),                           # row_pitch < span = 19 * 4 + 1, height > 1
        dict(ok, origin=elems - 19 * 4, height=1),            # the last sample one element past the plane
        dict(ok, origin=elems - 400 - 19 * 4),                # ... of the last row
        dict(ok, col_pitch=I64),
        dict(ok, col_pitch=I64 // 19 + 1),                    # (width - 1) * col_pitch overflows
        dict(ok, col_pitch=I64, width=I32, height=I32, out_pitch=I64),
        dict(ok, col_pitch=I32, width=I32, height=1, out_pitch=I64),
        dict(ok, col_pitch=2, width=I32, height=1, out_pitch=I64),
        dict(ok, row_pitch=I64, col_pitch=1),
        dict(ok, row_pitch=I64 // 4 + 1),                     # (height - 1) * row_pitch overflows
        dict(ok, origin=I64, height=1),
        dict(ok, origin=-1),
        dict(ok, width=-1),
        dict(ok, height=-2),
        dict(ok, out_pitch=20 * ts - 1),
        dict(ok, chunk_first=1),                              # chunk range outside the batch
        dict(ok, chunk_first=-1),
        dict(ok, chunk_count=0),
        dict(ok, chunk_count=I32),
        dict(ok, chunk_first=I32, chunk_count=I32),
    ]
    return ok, bad


@pytest.mark.parametrize("host", [False, True])
def test_invalid_windows_are_refused(L, host):
    ts = 2
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, blocksize=8192), raw, cbytes)
    plane = plane_of(chunks)
    ok, bad = invalid_cases(elems, ts)
    good, size = pack([ok], ts)
    for b in bad:
        rc, st, out, stats = call(L, chunks, [b], ts, 4096 * 8, host=host)
        assert rc == ERR_INVALID_PARAM, (b, rc)
        assert (out == CANARY).all() and not stats.any()                      # nothing run
        # ... also as the second window of a call whose first is good: nothing of the good one is written either
        rc, st, out, stats = call(L, chunks, [good[0], b], ts, size, host=host)
        assert rc == ERR_INVALID_PARAM and (out == CANARY).all() and not stats.any(), b
        # the engine stays usable
        rc, st, out, _ = call(L, chunks, good, ts, size, host=host)
        assert rc == 0 and np.array_equal(out, expected([plane], good, ts, size))
    # the edge itself is fine: the last sample is the plane's last element
    edge, size = pack([dict(ok, origin=elems - 1 - 19 * 4, height=1), dict(ok, origin=elems - 1 - 400 - 19 * 4)], ts)
    rc, st, out, _ = call(L, chunks, edge, ts, size, host=host)
    assert rc == 0 and np.array_equal(out, expected([plane] * 2, edge, ts, size))
    # a width-1 window never forms a product with its col_pitch
    one, size = pack([dict(ok, col_pitch=I64, width=1, height=3, out_pitch=ts)], ts)
    rc, st, out, _ = call(L, chunks, one, ts, size, host=host)
    assert rc == 0 and np.array_equal(out, expected([plane], one, ts, size))


def damaged(ts=4):
    raw, cbytes, elems, chunk_elems = geometry(ts)
    chunks = oracle_chunks(O.cparams(ts, blocksize=8192), raw, cbytes)
    good = plane_of(chunks)
    c = bytearray(chunks[1])
    j = 2                                                     # block 2 of chunk 1: elements chunk_elems + [4096, 6144)
    start = int.from_bytes(c[32 + 4 * j:36 + 4 * j], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")  # block 2's first stream claims more bytes than the chunk holds
    chunks[1] = bytes(c)
    # samples every 1000 elements over the whole plane: one of them (chunk_elems + 5000) lies in the damaged block
    inside = dict(chunk_first=0, chunk_count=3, origin=0, row_pitch=1, col_pitch=1000, width=31, height=1)
    # rows of chunk 1's elements [1000, 3000): its blocks 0 and 1 only
    outside = dict(chunk_first=0, chunk_count=3, origin=chunk_elems + 1000, row_pitch=50, col_pitch=3, width=7, height=40)
    return chunks, inside, outside, good, chunk_elems


@pytest.mark.parametrize("host", [False, True])
def test_damaged_chunk(L, host):
    chunks, inside, outside, good, chunk_elems = damaged()
    specs, size = pack([inside], 4)
    rc, st, out, _ = call(L, chunks, specs, 4, size, host=host)
    assert rc < 0 and st[1] == rc and st[0] == 0 and st[2] == 0
    # the others are still written: every sample outside chunk 1 is there
    want = expected([good], specs, 4, size)
    o = specs[0]["out_off"]
    for c in range(31):
        if not chunk_elems <= c * 1000 < 2 * chunk_elems:
            assert np.array_equal(out[o + 4 * c:o + 4 * c + 4], want[o + 4 * c:o + 4 * c + 4]), c
    assert (out[:o] == CANARY).all() and (out[o + 31 * 4:] == CANARY).all()
    specs, size = pack([outside], 4)
    rc, st, out, _ = call(L, chunks, specs, 4, size, host=host)
    assert rc == 0 and not st.any()
    assert np.array_equal(out, expected([good], specs, 4, size))


def case_blob(chunks, spec, ts, size, comp_size=None):
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    return b"".join([np.array([len(chunks), ts, size], np.int64).tobytes(), off.tobytes(),
                     (cs if comp_size is None else comp_size).tobytes(), nb.tobytes(), bs.tobytes(),
                     np.array([spec["chunk_first"], spec["chunk_count"]], np.int32).tobytes(),
                     np.array([spec["origin"], spec["row_pitch"], spec["col_pitch"]], np.int64).tobytes(),
                     np.array([spec["width"], spec["height"]], np.int32).tobytes(),
                     np.array([spec["out_off"], spec["out_pitch"]], np.int64).tobytes(),
                     np.array([buf.size], np.int64).tobytes(), buf.tobytes()])


def test_planner_and_kernel_under_asan(asan_exe, tmp_path):
    """Every window of the matrix, one call each, with outputs that end at the window's last byte; then the damaged chunk and
    truncated buffers.  The executable compares nothing: the sanitizers are the check, and the return codes."""
    path = tmp_path / "case.bin"

    def run(chunks, spec, ts, comp_size=None):
        spec = dict(spec, out_off=0, out_pitch=spec["width"] * ts)
        size = spec["width"] * ts * spec["height"]
        path.write_bytes(case_blob(chunks, spec, ts, size, comp_size))
        r = subprocess.run([asan_exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [int(x) for x in r.stdout.split()[:2]]

    for ts, filt in ((3, 1), (4, 2), (2, 0)):
        raw, cbytes, elems, chunk_elems = geometry(ts)
        chunks = oracle_chunks(O.cparams(ts, clevel=5, blocksize=8192, filters=(0, 0, 0, 0, 0, filt)), raw, cbytes)
        for spec in strided_windows(elems, chunk_elems, len(chunks), 8192 // ts):
            assert run(chunks, spec, ts) == [0, 0], spec
    chunks, inside, outside, _, _ = damaged()
    _, _, cs = concat(chunks)
    for spec, fails in ((inside, True), (outside, False)):
        for trunc in (0, 1):
            sz = cs.copy()
            if trunc:
                sz[1] = 100
            dev, hst = run(chunks, spec, 4, sz)
            if fails or trunc:
                assert dev < 0 and hst < 0, (spec, trunc, dev, hst)
            else:
                assert dev == 0 and hst == 0
    ok, bad = invalid_cases(31001, 4)
    for b in bad:
        path.write_bytes(case_blob(chunks, b, 4, 4096))
        r = subprocess.run([asan_exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert [int(x) for x in r.stdout.split()[:2]] == [ERR_INVALID_PARAM] * 2, b
