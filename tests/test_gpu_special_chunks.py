"""blosc2 special-value chunks (csrc/special_plan.h) on the MI355X: the read-route matrix of tests/test_emu_special_chunks.py through
cimg.hip -- batch device and host calls, the blosc2 shim, the wide route, the three window kernels on the six-chunk plane -- the
window write, and a DeviceChannel.full in a child process.  One engine serves the file; every device output sits between
canaries; the expectation is the oracle's decode of the same chunks (tests/_special_chunks.py writes them from the format).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
import _special_chunks as S
import _window_writes as WW
from _windows import CANARY, concat, expected, pack, sizes
from _windows_strided import expected as sexpected
from _special_chunks import CHUNK, PW, TS, b2params, construct, plane_params, plane_regions, six_chunks
from cimg import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_DATA = S.ERR_DATA
READS = S.read_cases()


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def batch_device(eng, chunks, mis=0, sized=True, two_step=False):
    """one device batch into outputs `16 + mis` canary bytes apart -> (status, outputs)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    gap = 16 + mis
    raw_off = np.zeros(len(chunks), np.int64)
    at = gap
    for i, n in enumerate(nb):
        raw_off[i] = at
        at += int(n) + gap
    total = at + 64
    d_comp, d_raw = eng.alloc(buf.size), eng.alloc(total)
    try:
        d_comp.upload(buf)
        d_raw.upload(np.full(total, CANARY, np.uint8))
        if two_step:
            eng.decompress_device_begin(d_comp.ptr, off, nb, bs, d_raw.ptr, raw_off)
            st = eng.decompress_device_fetch(len(chunks), check=False)
        else:
            st = eng.decompress_device(d_comp.ptr, off, nb, bs, d_raw.ptr, raw_off, check=False, comp_size=cs if sized else None)
        raw = d_raw.download()
    finally:
        d_comp.free()
        d_raw.free()
    outs, mask = [], np.ones(raw.size, bool)
    for o, n in zip(raw_off, nb):
        outs.append(raw[o:o + n].copy())
        mask[o:o + n] = False
    assert (raw[mask] == CANARY).all(), "a byte outside the outputs was written"
    return np.asarray(st), outs


def test_batch_device_every_kind(eng):
    """every kind and typesize in one batch between regular chunks, at four output alignments, sized, unsized and in two steps"""
    reg, raw = S.regular_chunk(4, S.geometry_nbytes(4))
    chunks = [reg] + [c for _, c in READS] + [reg]
    want = [S.want(c) for c in chunks]
    for mis, sized, two_step in ((0, True, False), (1, False, False), (5, True, True), (15, True, False)):
        st, outs = batch_device(eng, chunks, mis=mis, sized=sized, two_step=two_step)
        assert not st.any(), (mis, st, eng.last_error())
        for (name, _), got, w in zip([("regular", 0)] + READS + [("regular", 0)], outs, want):
            assert np.array_equal(got, w), (name, mis, sized, two_step)


def test_batch_host_every_kind(eng):
    chunks = [c for _, c in READS]
    outs, st = eng.decompress_host(chunks)
    assert not st.any()
    for (name, c), got in zip(READS, outs):
        assert np.array_equal(got, S.want(c)), name


def test_refusals_leave_the_neighbours_decoded(eng):
    reg, raw = S.regular_chunk(4, S.geometry_nbytes(4))
    good = S.chunk("value", 4, S.geometry_nbytes(4), 4096)
    for name, bad in S.refused_cases():
        chunks = [reg, bad, good, reg]
        st, outs = batch_device(eng, chunks)
        assert list(st) == [0, ERR_DATA, 0, 0], (name, st)
        assert np.array_equal(outs[0], raw) and np.array_equal(outs[3], raw) and np.array_equal(outs[2], S.want(good))
        assert (outs[1] == CANARY).all()
        outs, st = eng.decompress_host(chunks, check=False)
        assert list(st) == [0, ERR_DATA, 0, 0], (name, st)
        assert np.array_equal(outs[0], raw) and np.array_equal(outs[3], raw) and np.array_equal(outs[2], S.want(good))


def test_wide_blocks(eng):
    chunks = [S.chunk("value", 4, 2 * 196608 + 1000, 196608), S.chunk("value", 3, 2 * 196608 + 999, 196608),
              S.chunk("nan", 8, 196608 + 4096, 196608), S.chunk("uninit", 2, 2 * 196608, 196608)]
    st, outs = batch_device(eng, chunks, mis=5)
    assert not st.any(), (st, eng.last_error())
    for c, got in zip(chunks, outs):
        assert np.array_equal(got, S.want(c))


def test_shim_reads_and_constructors(eng):
    L = hip.load()
    dctx = L.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    try:
        for name, chunk in READS:
            want = S.want(chunk)
            src = np.frombuffer(chunk, np.uint8)
            dest = np.full(want.size + 32, CANARY, np.uint8)
            assert L.blosc2_decompress_ctx(dctx, hip._ptr(src), len(chunk), hip._ptr(dest), want.size) == want.size, name
            assert np.array_equal(dest[:want.size], want) and (dest[want.size:] == CANARY).all(), name
            ts = chunk[3]
            n = want.size // ts
            for start, k in ((n - 1, 1), (4096 // ts - 1, 3)):
                dest = np.full(k * ts + 16, CANARY, np.uint8)
                assert L.blosc2_getitem_ctx(dctx, hip._ptr(src), len(chunk), start, k, hip._ptr(dest), k * ts) == k * ts
                assert np.array_equal(dest[:k * ts], want[start * ts:(start + k) * ts]) and (dest[k * ts:] == CANARY).all(), name
        # the constructors of the product library write the bytes of the test's own writer
        for ts in (1, 3, 4, 8, 255):
            nbytes = S.geometry_nbytes(ts)
            po = O.cparams(ts, clevel=5, blocksize=4096)
            for kind in ("zero", "value", "uninit") + (("nan",) if ts in (4, 8) else ()):
                value = S.value_bytes(ts, seed=ts) if kind == "value" else None
                rc, got = construct(L, kind, b2params(ts), nbytes, value=value)
                assert rc == len(got) and got == S.from_cparams(po, kind, nbytes, value=value), (ts, kind)
        assert construct(L, "zero", b2params(4), 4096, destsize=31)[0] == ERR_DATA
        assert construct(L, "value", b2params(4), 4098, value=b"abcd")[0] == ERR_DATA
    finally:
        L.blosc2_free_ctx(dctx)


def window_specs(strided):
    sx, sy = (3, 5) if strided else (1, 1)
    specs = []
    for (x, y, w, h) in plane_regions():
        s = dict(chunk_first=0, chunk_count=6, origin=y * PW + x, row_pitch=sy * PW, width=(w + sx - 1) // sx, height=(h + sy - 1) // sy)
        if strided:
            s["col_pitch"] = sx
        specs.append(s)
    return pack(specs, TS)


@pytest.mark.parametrize("kind", ["plain", "strided", "grouped"])
def test_windows_over_six_kinds(eng, kind):
    chunks, plane = six_chunks()
    strided = kind != "plain"
    specs, size = window_specs(strided)
    want = (sexpected if strided else expected)([plane] * len(specs), specs, TS, size)
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp, d_out = eng.alloc(buf.size), eng.alloc(size)
    try:
        d_comp.upload(buf)
        d_out.upload(np.full(size, CANARY, np.uint8))
        rc, st = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, TS, specs, d_out.ptr, comp_size=cs, check=False,
                                               strided=kind == "strided", grouped=kind == "grouped")
        out = d_out.download()
    finally:
        d_comp.free()
        d_out.free()
    assert rc == 0 and not st.any(), (rc, st, eng.last_error())
    assert np.array_equal(out, want)
    assert eng.window_stats()["chunks_whole"] == 0
    out = np.full(size, CANARY, np.uint8)
    rc, st = eng.decompress_windows_host(chunks, specs, out, check=False, strided=kind == "strided", grouped=kind == "grouped")
    assert rc == 0 and not st.any(), (rc, st, eng.last_error())
    assert np.array_equal(out, want)
    stats = eng.window_stats()
    assert stats["chunks_whole"] == 0 and stats["comp_bytes_uploaded"] == sum(len(c) for c in chunks)
    # rows 20 .. 22 lie in the value chunk alone: 32 + 4 bytes cross the bus
    spec, size1 = pack([dict(chunk_first=0, chunk_count=6, origin=20 * PW + 9, row_pitch=PW, width=40, height=3, **(dict(col_pitch=1) if strided else {}))], TS)
    out = np.full(size1, CANARY, np.uint8)
    eng.decompress_windows_host(chunks, spec, out, strided=kind == "strided", grouped=kind == "grouped")
    assert eng.window_stats()["comp_bytes_uploaded"] == 32 + TS
    assert np.array_equal(out, (sexpected if strided else expected)([plane], spec, TS, size1))


def test_window_write_into_special_chunks(eng):
    chunks, plane = six_chunks()
    po = plane_params()
    p = hip.cparams(TS, clevel=5, blocksize=4096)
    specs, src = WW.source([dict(chunk_first=0, chunk_count=6, origin=20 * PW + 30, row_pitch=PW, width=100, height=20)], TS, seed=4)
    destsize = [CHUNK + 32] * 6
    new, st = eng.update_windows_host(p, chunks, destsize, specs, src)
    assert not st.any()
    want, _ = WW.expected(po, chunks, specs, TS, src, destsize)
    assert [c is not None for c in new] == [False, True, True, False, False, False]
    assert new[1] == want[1] and new[2] == want[2]                                  # byte for byte the oracle's compress of the edited pixels


def test_device_channel_full_in_a_child_process():
    case = "gpu_full_set_region"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_special.py"), case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
