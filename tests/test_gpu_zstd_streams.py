"""The GPU read paths on spec-built zstd chunks (tests/_zstd_streams.py, tests/_streams.py: zstd_plane_cases), seeded as in
test_emu_zstd_streams.py; the digests of tests/golden/zstd_streams_digests.json tie both legs to the bytes libzstd validated.

Every plane goes through Engine.decompress_host and decompress_device (with comp_size, into a canary-filled buffer), through
blosc2_decompress_ctx and blosc2_getitem_ctx one chunk at a time, and through decompress_windows_device / _host with the standard
windows of tests/_windows.py; then once per form of the zstd read path (one engine per form, the environment set by monkeypatch, as
test_every_form_of_the_zstd_read_path_on_the_gpu does).  The frames every decoder must refuse run in a batch between good chunks.
Pixel bytes, the status of every chunk and the canary around the outputs are asserted.  Nothing here is meant to fault: the invalid
frames are ordinary decode traffic that must be reported.

Then every frame on its own (tests/_zstd_streams.py: frame_chunk_cases): each spec-built frame a chunk can carry, the frames libzstd
made of the golden inputs up to 160 KiB and the frames the repository's encoder makes of the mix streams -- among the last two groups
every frame whose literal copies the host emulator got wrong in its descending and shuffled write orders -- one
stream per chunk, all of them in ONE batch per entry point and per form of the read path, canaries around every output.  Expected
bytes: what the frames' sequences define, the golden inputs, the streams; never anything the code under test computed.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import _streams as S
import _zstd_streams as Z
from _windows import expected, sizes, standard_windows
from cimg import hip
from test_gpu_stream_conformance import device_batch, split_plane, want_buffer, windows_both

pytestmark = pytest.mark.gpu
CANARY = S.CANARY
PLANES = S.zstd_plane_cases()
FORMS = {"lanes_8": {}, "lanes_3": {"CIMG_ZSTD_LANES": "3"}, "walkers_decode_sequences": {"CIMG_ZSTD_LANES": "0"},
         "fused": {"CIMG_ZSTD_FUSED": "1"}, "plans_overflow": {"CIMG_ZSTD_PLAN_CAP": "256"},
         "groups_of_9_blocks": {"CIMG_ZSTD_PLAN_MIB": "1"}, "no_memory_for_plans": {"CIMG_ZSTD_PLAN_FAIL": "1"}}
FORM_KEYS = ("CIMG_ZSTD_LANES", "CIMG_ZSTD_FUSED", "CIMG_ZSTD_PLAN_CAP", "CIMG_ZSTD_PLAN_MIB", "CIMG_ZSTD_PLAN_FAIL")


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dctx():
    L = hip.load()
    d = L.blosc2_create_dctx(hip.Blosc2DParams(1, None, None, None))
    yield d
    L.blosc2_free_ctx(d)


@pytest.fixture(scope="module")
def planes():
    """every plane built once: name -> (chunks, pixels, parts)"""
    out = {}
    for name, codec, ts, kw in PLANES:
        chunks, plane, counts = S.build_plane(name, codec, ts, kw)
        assert counts["coded"] >= 2
        out[name] = (chunks, plane, split_plane(chunks, plane))
    return out


def test_generated_bytes_are_the_ones_libzstd_validated(planes, golden_dir):
    with open(os.path.join(golden_dir, "zstd_streams_digests.json")) as f:
        pinned = json.load(f)
    for name, (chunks, plane, _) in planes.items():
        assert pinned["planes"][name] == [hashlib.sha256(b"".join(chunks)).hexdigest(), hashlib.sha256(plane.tobytes()).hexdigest()], name
    assert {name: hashlib.sha256(fr).hexdigest() for name, fr, _, _ in Z.bad_frames()} == pinned["bad_frames"]


@pytest.mark.parametrize("case", PLANES, ids=[c[0] for c in PLANES])
def test_generated_zstd_chunks_every_gpu_path(eng, dctx, planes, case):
    name, codec, ts, kw = case
    chunks, plane, parts = planes[name]
    outs, st = eng.decompress_host(chunks, check=False)
    assert not st.any(), (st, eng.last_error())
    for o, p in zip(outs, parts):
        assert np.array_equal(o, p)
    st, out, raw_off = device_batch(eng, chunks)
    assert not st.any(), st
    assert np.array_equal(out, want_buffer(parts, raw_off, out.size))
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
                (int(a), int(rng.integers(1, items - a + 1))) for a in rng.integers(0, items, 2)):
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


@pytest.mark.parametrize("form", list(FORMS))
def test_generated_zstd_chunks_every_form_of_the_read_path(form, planes, monkeypatch):
    """one engine per form; every plane in its own batch (host and device route), then the negative frames between good chunks"""
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    e = hip.Engine(0)
    try:
        for name, codec, ts, kw in PLANES:
            chunks, plane, parts = planes[name]
            st, out, raw_off = device_batch(e, chunks, check=False)
            if form == "no_memory_for_plans" and kw["blocksize"] > 163840:
                # (blocks beyond LDS have no fused kernel to fall back on: without plan memory their chunks say BLOSC2_ERROR_MEMORY_ALLOC,
                # engine.hip: decompress_finish_wide_zstd)
                assert (st == -4).all(), (form, name, st)
                continue
            assert not st.any(), (form, name, st)
            assert np.array_equal(out, want_buffer(parts, raw_off, out.size)), (form, name)
            outs, st = e.decompress_host(chunks, check=False)
            assert not st.any() and all(np.array_equal(o, p) for o, p in zip(outs, parts)), (form, name, st)
        check_bad_frames(e, planes, form)
        st = e.zstd_stats()
        assert st["zstd_batches"] >= 1
        # (plans that do not fit their slot go to the fused kernel in every form that walks: a split block of eight frames with
        # several compressed blocks each -- zstd_ts8_f1 -- needs more tables than a slot holds; with 256-byte plans nearly all do)
        if form == "plans_overflow":
            assert st["blocks_refused"] > 100, (form, st)
        if form in ("fused", "no_memory_for_plans"):
            assert st["blocks_refused"] == 0, (form, st)
    finally:
        e.close()


def check_bad_frames(e, planes, what):
    good, gplane, _ = planes[PLANES[0][0]]
    batch, bad_at = [], []
    for name, fr, n, code in Z.bad_frames():
        batch += [good[0], S.chunk_of_streams(S.ZSTD, [(fr, np.zeros(n, np.uint8))])]
        bad_at.append((len(batch) - 1, name, code))
    batch.append(good[0])
    gp = split_plane(good, gplane)[0]
    st, out, raw_off = device_batch(e, batch, check=False)
    nb, _ = sizes(batch)
    bad = {k for k, _, _ in bad_at}
    for k, name, code in bad_at:
        assert st[k] < 0 and (code is None or st[k] == code), (what, name, st[k])
    for k in range(len(batch)):
        if k not in bad:
            assert st[k] == 0 and np.array_equal(out[raw_off[k]:raw_off[k] + gp.size], gp), (what, k)
        assert (out[raw_off[k] - 48:raw_off[k]] == CANARY).all() and (out[raw_off[k] + nb[k]:raw_off[k] + nb[k] + 48] == CANARY).all(), (what, k)
    outs, st = e.decompress_host(batch, check=False)
    for k in range(len(batch)):
        assert (st[k] < 0) == (k in bad), (what, k, st[k])
        if k not in bad:
            assert np.array_equal(outs[k], gp), (what, k)


def test_bad_frames_are_reported_on_every_entry_point(eng, dctx, planes):
    check_bad_frames(eng, planes, "default")
    L = hip.load()
    for name, fr, n, code in Z.bad_frames():
        chunk = S.chunk_of_streams(S.ZSTD, [(fr, np.zeros(n, np.uint8))])
        src = np.frombuffer(chunk, np.uint8)
        dest = np.full(n + 64, CANARY, np.uint8)
        assert L.blosc2_decompress_ctx(dctx, hip._ptr(src), len(chunk), hip._ptr(dest), n) < 0, name
        assert (dest[n:] == CANARY).all(), name
        dev, host, _, _ = windows_both(eng, [chunk], 1, [dict(chunk_first=0, chunk_count=1, origin=0, row_pitch=n, width=n, height=1)])
        for what, (rc, st, _) in (("device", dev), ("host", host)):
            assert rc < 0 and st[0] < 0, (name, what, rc, st)


# ---- every frame as the one stream of a chunk --------------------------------------------------------------------------------------
LDS_BLOCK_MAX, FORM_BLOCK_MAX = Z.LDS_BLOCK_MAX, Z.FORM_BLOCK_MAX


@pytest.fixture(scope="module")
def frame_chunks(golden_dir):
    """(name, chunk, expected bytes): the spec-built frames against the digests libzstd validated, before anything is decoded"""
    import _emu as Em
    cases = Z.frame_chunk_cases(golden_dir, Em.zstd_encode)
    with open(os.path.join(golden_dir, "zstd_streams_digests.json")) as f:
        pinned = json.load(f)["frames"]
    seen = 0
    for name, chunk, want in cases:
        assert want.size == int.from_bytes(chunk[4:8], "little") and 0 < len(chunk) - 40 < want.size, name
        if name in pinned:
            assert pinned[name] == [hashlib.sha256(chunk[40:]).hexdigest(), hashlib.sha256(want.tobytes()).hexdigest()], name
            seen += 1
    names = {c[0] for c in cases}
    assert seen >= 150 and len(cases) >= 300 and "kat|nibbles_16k|L1" in names and "mix18" in names
    return cases


def check_frame_batch(e, cases, what, refused_wide=False):
    """one decompress_device call (canaries between the outputs) and one decompress_host call over all the chunks"""
    chunks = [c for _, c, _ in cases]
    st, out, raw_off = device_batch(e, chunks, check=False)
    if refused_wide:
        assert (st == -4).all(), (what, st)
        return
    assert not st.any(), (what, [(n, int(s)) for (n, _, _), s in zip(cases, st) if s])
    for (name, _, w), o in zip(cases, raw_off):
        assert np.array_equal(out[o:o + w.size], w), (what, name)
    assert np.array_equal(out, want_buffer([w for _, _, w in cases], raw_off, out.size)), what       # (the canaries)
    outs, st = e.decompress_host(chunks, check=False)
    assert not st.any(), (what, st)
    for (name, _, w), o in zip(cases, outs):
        assert np.array_equal(o, w), (what, name, "host")


def test_every_frame_as_the_one_stream_of_a_chunk(eng, frame_chunks):
    normal = [c for c in frame_chunks if c[2].size <= LDS_BLOCK_MAX]
    wide = [c for c in frame_chunks if c[2].size > LDS_BLOCK_MAX]
    assert len(wide) == 3 and min(c[2].size for c in normal) <= 100 and max(c[2].size for c in normal) >= 140000
    check_frame_batch(eng, normal, "default")
    check_frame_batch(eng, wide, "default, wide route")


@pytest.mark.parametrize("form", list(FORMS))
def test_every_frame_as_the_one_stream_of_a_chunk_every_form_of_the_read_path(form, frame_chunks, monkeypatch):
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    e = hip.Engine(0)
    try:
        cases = [c for c in frame_chunks if c[2].size <= FORM_BLOCK_MAX]
        assert len(cases) >= len(frame_chunks) - 10          # (left to the default engine: 139 084 .. 150 000 bytes, and the wide three)
        check_frame_batch(e, cases, form)
    finally:
        e.close()


def test_mix_chunks_written_on_the_gpu_are_the_emulators_and_decode(eng):
    """codec::zstd over mix streams (every fifth one, mix18 among them), a chunk each: byte for byte what the kernel sources write on
    the host lane emulator; the GPU reads them back (one batch, canaries), and so does libzstd where the box has one"""
    import _emu as Em
    import _oracle as O
    mix = Z.mix_streams()
    picked = [mix["mix%d" % k] for k in range(3, 120, 5)]
    assert mix["mix18"] is picked[3]
    raw = np.concatenate(picked)
    sizes_ = [p.size for p in picked]
    dest = [n + 32 for n in sizes_]
    got = eng.compress_host(hip.cparams(1, clevel=9, compcode=hip.ZSTD), raw, sizes_, dest)
    rc, cb, emu = Em.compress_batch(Em.cparams(1, clevel=9, compcode=hip.ZSTD), raw, sizes_, dest)
    assert rc == 0 and got == emu
    assert sum(1 for c in got if not c[2] & 0x02) >= 12                    # (most of them shrink: coded, not memcpyed)
    st, out, raw_off = device_batch(eng, got, check=False)
    assert not st.any(), st
    assert np.array_equal(out, want_buffer(picked, raw_off, out.size))
    outs, st = eng.decompress_host(got, check=False)
    assert not st.any() and all(np.array_equal(o, p) for o, p in zip(outs, picked))
    if O.zstd_available():
        for c, p in zip(got, picked):
            r, px = O.decompress(c)
            assert r == p.size and np.array_equal(px, p)

