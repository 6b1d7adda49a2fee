"""The GPU decode paths on spec-built LZ4 and BloscLZ chunks (tests/_streams.py), seeded as in test_emu_stream_conformance.py.

Every generated plane goes through Engine.decompress_host and decompress_device (with comp_size, into a canary-filled buffer) on a
normal engine and on one created with CIMG_NO_LEAN=1, through blosc2_decompress_ctx and blosc2_getitem_ctx one chunk at a time,
and through decompress_windows_device / _host with the standard windows of tests/_windows.py.  Blocks of 192 and 256 KiB take the
wide kernel (far BloscLZ matches, long length headers, long LZ4 matches); a batch mixes generated chunks with oracle chunks.  Pixel
bytes, the status of every chunk and the canary around the outputs are asserted.  Nothing here is meant to fault: the invalid
streams are ordinary decode traffic that must be reported.
"""
import os

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _windows import concat, expected, pack, sizes, standard_windows
from cimg import hip

pytestmark = pytest.mark.gpu
CANARY = S.CANARY
PLANES = S.plane_cases() + S.wide_cases()


@pytest.fixture(scope="module")
def engines():
    e = hip.Engine(0)
    os.environ["CIMG_NO_LEAN"] = "1"
    try:
        e2 = hip.Engine(0)
    finally:
        del os.environ["CIMG_NO_LEAN"]
    yield {"lean": e, "nolean": e2}
    e2.close()
    e.close()


@pytest.fixture(scope="module")
def dctx():
    L = hip.load()
    d = L.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    yield d
    L.blosc2_free_ctx(d)


def split_plane(chunks, plane):
    nb, _ = sizes(chunks)
    return np.split(plane, np.cumsum(nb)[:-1])


def device_batch(eng, chunks, gap=48, check=True):
    """decompress_device with comp_size into a canary-filled device buffer -> (status, whole buffer, raw_off)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    raw_off, at = [], gap
    for n in nb:
        raw_off.append(at)
        at += int(n) + gap
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_raw = eng.alloc(at)
    d_raw.upload(np.full(at, CANARY, np.uint8))
    st = eng.decompress_device(d_comp.ptr, off, nb, bs, d_raw.ptr, raw_off, comp_size=cs, check=check)
    out = d_raw.download()
    d_comp.free()
    d_raw.free()
    return st, out, raw_off


def want_buffer(parts, raw_off, size):
    want = np.full(size, CANARY, np.uint8)
    for o, p in zip(raw_off, parts):
        want[o:o + p.size] = p
    return want


def windows_both(eng, chunks, ts, specs_in):
    specs, size = pack(specs_in, ts)
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    d_comp = eng.alloc(buf.size)
    d_comp.upload(buf)
    d_out = eng.alloc(size)
    d_out.upload(np.full(size, CANARY, np.uint8))
    rc_d, st_d = eng.decompress_windows_device(d_comp.ptr, off, nb, bs, ts, specs, d_out.ptr, comp_size=cs, check=False)
    out_d = d_out.download()
    d_comp.free()
    d_out.free()
    out_h = np.full(size, CANARY, np.uint8)
    rc_h, st_h = eng.decompress_windows_host(chunks, specs, out_h, check=False)
    return (rc_d, st_d, out_d), (rc_h, st_h, out_h), specs, size


@pytest.mark.parametrize("case", PLANES, ids=[c[0] for c in PLANES])
def test_generated_chunks_every_gpu_path(engines, dctx, case):
    name, codec, ts, kw = case
    chunks, plane, counts = S.build_plane(name, codec, ts, kw)
    parts = split_plane(chunks, plane)
    for which, eng in engines.items():
        outs, st = eng.decompress_host(chunks, check=False)
        assert not st.any(), (which, st, eng.last_error())
        for o, p in zip(outs, parts):
            assert np.array_equal(o, p), which
        st, out, raw_off = device_batch(eng, chunks)
        assert not st.any(), (which, st)
        assert np.array_equal(out, want_buffer(parts, raw_off, out.size)), which
    eng = engines["lean"]
    # the blosc2 entry points, one chunk per call
    L = hip.load()
    rng = np.random.default_rng(len(name))
    for c, p in zip(chunks, parts):
        src = np.frombuffer(c, np.uint8)
        dest = np.full(p.size + 64, CANARY, np.uint8)
        assert L.blosc2_decompress_ctx(dctx, hip._ptr(src), len(c), hip._ptr(dest), p.size) == p.size
        assert np.array_equal(dest[:p.size], p) and (dest[p.size:] == CANARY).all()
        items = p.size // ts
        for start, nitems in ((0, 1), (items - 1, 1), (int(rng.integers(0, items)), 0), (0, items)) + tuple(
                (int(a), int(rng.integers(1, items - a + 1))) for a in rng.integers(0, items, 3)):
            nitems = min(nitems, items - start)
            dest = np.full(nitems * ts + 32, CANARY, np.uint8)
            rc = L.blosc2_getitem_ctx(dctx, hip._ptr(src), len(c), start, nitems, hip._ptr(dest), dest.size)
            assert rc == nitems * ts, (start, nitems, rc)
            assert np.array_equal(dest[:rc], p[start * ts:start * ts + rc]) and (dest[rc:] == CANARY).all()
    # windows
    elems = plane.size // ts
    dev, host, specs, size = windows_both(eng, chunks, ts, standard_windows(elems, 180, int(sizes(chunks)[0][0]) // ts, len(chunks)))
    want = expected([plane] * len(specs), specs, ts, size)
    for what, (rc, st, out) in (("device", dev), ("host", host)):
        assert rc == 0 and not st.any(), (what, rc, st)
        assert np.array_equal(out, want), what


def test_generated_chunks_behind_oracle_chunks(engines):
    """generated chunks of several geometries, each behind an oracle chunk, in one batch (also with wide ones in it)"""
    rng = np.random.default_rng(5)
    batch, want = [], []
    for k, (name, codec, ts, kw) in enumerate(PLANES[::5] + PLANES[-3:]):
        chunks, plane, _ = S.build_plane(name, codec, ts, kw, nchunks=2)
        raw = (np.arange(20000 + 1000 * k) % (7 + k)).astype(np.uint8)
        raw[::13] = rng.integers(0, 256, raw[::13].size, dtype=np.uint8)
        r, oc = O.compress(O.cparams(2, clevel=5, blocksize=8192, compcode=O.BLOSCLZ if k % 2 else O.LZ4), raw)
        assert r > 0
        for c, p in zip(chunks, split_plane(chunks, plane)):
            batch += [oc, c]
            want += [raw, p]
    for which, eng in engines.items():
        st, out, raw_off = device_batch(eng, batch)
        assert not st.any(), (which, st)
        assert np.array_equal(out, want_buffer(want, raw_off, out.size)), which
        outs, st = eng.decompress_host(batch, check=False)
        assert not st.any() and all(np.array_equal(o, w) for o, w in zip(outs, want)), which


def test_invalid_streams_are_reported(engines, dctx):
    L = hip.load()
    good_chunks, good_plane, _ = S.build_plane(*PLANES[0][:3], PLANES[0][3], nchunks=1)
    for name, codec, chunk, _, n in S.bad_chunks():
        for which, eng in engines.items():
            st, out, raw_off = device_batch(eng, [good_chunks[0], chunk, good_chunks[0]], check=False)
            assert st[0] == 0 and st[1] < 0 and st[2] == 0, (name, which, st)
            for k in (0, 2):
                assert np.array_equal(out[raw_off[k]:raw_off[k] + good_plane.size], good_plane), (name, which, k)
            assert (out[:raw_off[0]] == CANARY).all() and (out[raw_off[2] + good_plane.size:] == CANARY).all()
            outs, st = eng.decompress_host([chunk], check=False)
            assert st[0] < 0, (name, which)
        src = np.frombuffer(chunk, np.uint8)
        dest = np.zeros(2 * n + 64, np.uint8)
        assert L.blosc2_decompress_ctx(dctx, hip._ptr(src), len(chunk), hip._ptr(dest), dest.size) < 0, name
        elems = 2 * n
        dev, host, _, _ = windows_both(engines["lean"], [chunk], 1, [dict(chunk_first=0, chunk_count=1, origin=0, row_pitch=elems,
                                                                          width=elems, height=1)])
        for what, (rc, st, _) in (("device", dev), ("host", host)):
            assert rc < 0 and st[0] < 0, (name, what, rc, st)
