"""Every form of the emulated zstd read path on spec-built frames and chunks (tests/_zstd_streams.py, tests/_streams.py).

The frames are written from block and sequence lists by a writer that follows RFC 8878 and shares nothing with csrc/ or oracle/,
so they are not what any one encoder happens to produce: every literals and sequences mode, table descriptions with "less than 1"
probabilities and chained zero runs, every length code, repeat offsets in every position, raw and RLE blocks between compressed
ones, and last blocks of a few bytes behind a full one at exact capacity.  The expected output is the buffer the sequences define.

  * the writer: libzstd (where the box has one) decodes every positive frame to the expected bytes; a negative frame it refuses or
    decodes to the expected bytes.  The sha256 of every frame and output is pinned in tests/golden/zstd_streams_digests.json, written
    (tests/golden/make_zstd_streams_digests.py) only after libzstd 1.4.8 accepted them all -- the GPU leg, which may have no
    libzstd, asserts the same digests.  One candidate was not legal and is left out: a compressed block of two bytes (no literals
    behind a 1-byte header, no sequences), which libzstd refuses as shorter than its minimum of three.  Two named cases cannot
    exist as worded: a compressed block WITH sequences regenerates at least 3 bytes (tails 3 and 7 stand in for 1), and literal
    length code 35 with match length code 52 is 131075 bytes, three more than a block holds (15 + 16 + 17 and 16 + 16 + 16 extra
    bits are run instead of 16 + 16 + 17).
  * every frame through emu_zstd_decode (the decoder in place, through a stage like the kernel's, through a tiny stage, all copies
    serial, and walked + replayed; they must agree) at capacity n and n + 8, and refused at n - 1
  * every chunk plane through the emulated batch decode under the five forms of the read path of test_emu_zstd.py, and through the
    wide route (blocks of 192 KiB) with canaries around every output
  * the frames of the tail-block defect once more as a stand-alone AddressSanitizer / UBSan program
"""
import ctypes as C
import ctypes.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _emu as E
import _oracle as O
import _streams as S
import _zstd_streams as Z
from _windows import concat, sizes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
CANARY = S.CANARY
PLANES = S.zstd_plane_cases()
FORMS = ["planned", "planned_3_lanes", "walkers_decode_sequences", "fused", "plans_overflow"]


@pytest.fixture(scope="module")
def frames():
    return Z.frame_cases()


@pytest.fixture(scope="module")
def libzstd():
    name = ctypes.util.find_library("zstd")
    if not name:
        return None
    z = C.CDLL(name)
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    z.ZSTD_compressBound.restype = C.c_size_t
    z.ZSTD_compressBound.argtypes = [C.c_size_t]
    z.ZSTD_compress.restype = C.c_size_t
    z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    return z


@pytest.fixture(scope="module")
def ZW(tmp_path_factory):
    """emu.cpp + wide_emu.cpp + zstd_wide_emu.cpp (as test_emu_zstd_wide_blocks.py builds them): zwemu_decompress_batch routes normal
    chunks to the kernels of emu.cpp and blocks beyond LDS to the wide kernel and the wide zstd read path, as the engine does"""
    out = str(tmp_path_factory.mktemp("zstd_streams_emu") / "libzstd_streams_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-I", CSRC, os.path.join(EMU, "emu.cpp"),
                           os.path.join(EMU, "wide_emu.cpp"), os.path.join(EMU, "zstd_wide_emu.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    L = C.CDLL(out)
    vp = C.c_void_p
    L.zwemu_decompress_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


@pytest.fixture(params=FORMS)
def zstd_read_path(request):
    """the forms of the read path, as in test_emu_zstd.py"""
    E.set_zstd_plan({"fused": 0, "plans_overflow": 256}.get(request.param, -1))
    E.set_zstd_lanes({"planned_3_lanes": 3, "walkers_decode_sequences": 0}.get(request.param, 8))
    E.zstd_refused()
    yield request.param
    E.set_zstd_plan(-1)
    E.set_zstd_lanes(8)


ORDERS = (0, 1, 2)


def in_every_write_order(fn):
    """Run the test once in each order in which the emulator visits the lanes of a FOR_LANES_W body (csrc/wave.h, R2: ascending,
    descending, shuffled) and put the ascending order back.  The test keeps its name and its other arguments; one that names a
    `write_order` argument is told the order.  A result must not depend on it: positive frames give their input's BYTES in every
    order (two copy loops that read what another lane of the same body had stored returned the right length over wrong bytes in
    the other two orders)."""
    import functools
    import inspect
    sig = inspect.signature(fn)
    wants = "write_order" in sig.parameters

    @functools.wraps(fn)
    def run(*args, **kw):
        try:
            for order in ORDERS:
                E.set_write_order(order)
                try:
                    fn(*args, **kw, **({"write_order": order} if wants else {}))
                except AssertionError as e:
                    raise AssertionError("in write order %d: %s" % (order, e)) from e
        finally:
            E.set_write_order(0)
    del run.__wrapped__
    run.__signature__ = sig.replace(parameters=[p for name, p in sig.parameters.items() if name != "write_order"])
    return run


@pytest.fixture(params=ORDERS, ids=["ascending", "descending", "shuffled"])
def write_order(request):
    """the same as a parameter (the library of the wide route keeps an order of its own: emu_batch sets it)"""
    E.set_write_order(request.param)
    yield request.param
    E.set_write_order(0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def out_layout(nbytes, gap=48):
    offs, at = [], gap
    for n in nbytes:
        offs.append(at)
        at += int(n) + gap
    return np.array(offs, np.int64), at


def want_buffer(parts, raw_off, size):
    want = np.full(size, CANARY, np.uint8)
    for o, p in zip(raw_off, parts):
        want[o:o + p.size] = p
    return want


def emu_batch(chunks, wide=None, order=0):
    """the emulated batch decode into a canary-filled buffer -> (rc, status, whole buffer, raw_off); order: the write order of the
    wide route's library (the write_order fixture sets the other one)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    raw_off, size = out_layout(nb)
    raw = np.full(size, CANARY, np.uint8)
    st = np.zeros(len(chunks), np.int32)
    if wide is None:
        rc = E.lib().emu_decompress_batch(len(chunks), _p(buf), _p(off), _p(nb), _p(bs), _p(raw), _p(raw_off), _p(st))
    else:
        wide.emu_set_write_order(order)
        try:
            rc = wide.zwemu_decompress_batch(len(chunks), _p(buf), _p(off), _p(cs), _p(nb), _p(bs), _p(raw), _p(raw_off), _p(st))
        finally:
            wide.emu_set_write_order(0)
    return rc, st, raw, raw_off


def split_plane(chunks, plane):
    nb, _ = sizes(chunks)
    return np.split(plane, np.cumsum(nb)[:-1])


def local_tail_frames(z):
    """what the issue measured: 128 KiB + t bytes compressed by the box's libzstd (two blocks, the second a few bytes)"""
    out = []
    for t in (15, 17, 33):
        n = 131072 + t
        src = np.tile(np.random.default_rng(1).integers(0, 64, 997), 140)[:n].astype(np.uint8)
        for level in (1, 3, 19):
            dst = np.zeros(z.ZSTD_compressBound(n), np.uint8)
            r = z.ZSTD_compress(_p(dst), dst.size, _p(src), n, level)
            assert not z.ZSTD_isError(r)
            out.append(("libzstd_%d_L%d" % (n, level), dst[:r].tobytes(), src))
    return out


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def test_every_named_case_is_there_and_coded(frames):
    names = {c[0] for c in frames}
    assert len(frames) >= 180
    for need in ("frame_A", "frame_B", "frame_C", "block_128k", "raw_rle_between", "eight_blocks", "empty", "only_raw", "only_rle",
                 "nseq_three_bytes", "rep_run70", "rep_initial_history", "every_length_code_predef", "every_length_code_fse9",
                 "max_extra_bits_of16", "max_extra_bits_of17_rle52", "offset_codes_2_to_17", "offset_1_overlap_and_position",
                 "fse_log5", "fse_log_max", "fse_zero_runs_minus_one", "fse_two_symbols", "fse_last_symbols", "fse_rle_largest",
                 "fse_repeat_after_fse", "fse_repeat_after_rle", "fse_repeat_after_predef", "huf_2sym", "huf_3sym", "huf_128sym",
                 "huf_255sym", "huf_256sym", "huf_len11", "huf_20k_tree_then_treeless", "seq_stream_above_8k", "checksum_two_blocks"):
        assert need in names, need
    for t in Z.TAILS:
        for kind in ("lits", "raw", "rle"):
            assert "tail_%s%d_s0" % (kind, t) in names and "tail_%s%d_s1" % (kind, t) in names
        if t > 1:
            assert "tail_seq%d_s0" % t in names and "tail_seq%d_s1" % t in names
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        assert "nseq%d_s0" % n in names and "nseq%d_s1" % n in names
    for n in (6, 7, 1023, 1024, 16383, 16384, 20001):
        assert any(c.startswith("huf_regen%d_" % n) for c in names)
    # nothing fell back to a raw block: every frame but the four that are about raw / RLE / empty has a compressed block, and the
    # frames named after an encoding carry its marks (Huffman: literals type 2 in the first block; treeless: type 3 in the second)
    for name, fr, want in frames:
        if name in ("empty", "only_raw", "only_rle") or (name.startswith("fcs") and want.size < 40):
            continue
        single, flag = fr[4] & 0x20, fr[4] >> 6
        at = 5 + (0 if single else 1) + ((1 if single else 0) if flag == 0 else (0, 2, 4, 8)[flag])
        types = []
        first_lit = []
        while True:
            bh = int.from_bytes(fr[at:at + 3], "little")
            types.append((bh >> 1) & 3)
            if types[-1] == 2:
                first_lit.append(fr[at + 3] & 3)
            at += 3 + (1 if types[-1] == 1 else bh >> 3)
            if bh & 1:
                break
        assert 2 in types, name
        if name.startswith("huf_"):
            assert first_lit[0] == 2 and 3 in first_lit[1:], name


def test_frames_A_B_C_are_the_issues_bytes():
    assert Z.FRAME_A.hex() == "28b52ffd200e5c00002061626364015404020007450000207778797a01fc07"
    assert Z.FRAME_C.hex() == "28b52ffd200b5c00002061626364015404020007350000207778797a00"
    assert Z.FRAME_B[:20] == Z.FRAME_A[:20] and Z.FRAME_B[20:].hex() == "5d0000207778797a015404020007"


def test_xxh64_known_answers():
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999
    assert Z.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert Z.xxh64(b"abc") == 0x44BC2CF5AD770999
    assert Z.xxh64(b"Nobody inspects the spammish repetition") == 0xFBCEA83C8A378BF1


def test_libzstd_decodes_every_frame(frames, libzstd):
    if libzstd is None:
        pytest.skip("no system libzstd on this box: the writer is pinned by the digests libzstd 1.4.8 validated")
    for name, fr, want in frames:
        out = np.full(want.size + 64, CANARY, np.uint8)
        r = libzstd.ZSTD_decompress(_p(out), want.size, fr, len(fr))
        assert not libzstd.ZSTD_isError(r) and r == want.size, (name, r)
        assert np.array_equal(out[:r], want) and (out[r:] == CANARY).all(), name
    for name, fr, n, _ in Z.bad_frames():
        out = np.zeros(n + 64, np.uint8)
        r = libzstd.ZSTD_decompress(_p(out), n, fr, len(fr))
        # (refused -- or, where libzstd does not look: the frame decodes to the n bytes its good twin decodes to)
        assert libzstd.ZSTD_isError(r) or r == n, name


def test_digests_match_the_committed_ones(frames, golden_dir):
    with open(os.path.join(golden_dir, "zstd_streams_digests.json")) as f:
        pinned = json.load(f)
    mine = Z.digests(frames)
    assert sorted(mine) == sorted(pinned["frames"])
    for name in mine:
        assert mine[name] == pinned["frames"][name], name
    bad = {name: Z.hashlib.sha256(fr).hexdigest() for name, fr, _, _ in Z.bad_frames()}
    assert bad == pinned["bad_frames"]
    planes = {}
    for name, codec, ts, kw in PLANES:
        chunks, plane, _ = S.build_plane(name, codec, ts, kw)
        planes[name] = [Z.hashlib.sha256(b"".join(chunks)).hexdigest(), Z.hashlib.sha256(plane.tobytes()).hexdigest()]
    assert planes == pinned["planes"]


# ---- bare frames ------------------------------------------------------------------------------------------------------------------
@in_every_write_order
def test_every_frame_at_exact_capacity_and_with_room_and_not_without(frames):
    for name, fr, want in frames:
        for cap in (want.size, want.size + 8):
            r, out = E.zstd_decode(fr, cap)
            assert r == want.size and out == want.tobytes(), (name, cap, r)
        if want.size:
            r, _ = E.zstd_decode(fr, want.size - 1)
            assert r < 0, (name, r)


@in_every_write_order
def test_tail_frames_made_by_the_local_libzstd(libzstd):
    if libzstd is None:
        pytest.skip("no system libzstd on this box")
    for name, fr, src in local_tail_frames(libzstd):
        r, out = E.zstd_decode(fr, src.size)
        assert r == src.size and out == src.tobytes(), (name, r)


@in_every_write_order
def test_bad_frames_are_refused():
    for name, fr, n, code in Z.bad_frames():
        for cap in (n, n + 8):
            r, _ = E.zstd_decode(fr, cap)
            assert r < 0 and (code is None or r == code), (name, cap, r)


def test_tail_frames_under_address_sanitizer(frames, libzstd, tmp_path_factory):
    """frames A - C, the short-last-block frames and (where there is a libzstd) the 128 KiB + 15 / 17 / 33 ones through emu_zstd_decode
    in a stand-alone ASan / UBSan program: every buffer an allocation of its exact size; once in each write order"""
    d = tmp_path_factory.mktemp("zstd_frames_asan")
    exe = str(d / "zstd_frames_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", "-std=c++17",
                           "-fno-strict-aliasing", "-I", CSRC, os.path.join(EMU, "zstd_frames_asan_main.cpp"), os.path.join(EMU, "emu.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    picked = [c for c in frames if c[0] in ("frame_A", "frame_B", "frame_C", "tail_seq15_s0", "tail_seq17_s0", "tail_seq33_s1", "tail_lits15_s0",
                                            "tail_raw1_s0", "tail_rle16_s0", "tail_rlelits17_s1", "raw_rle_between", "eight_blocks", "rep_run70",
                                            "huf_256sym", "fse_zero_runs_minus_one", "empty", "nseq1_s0", "nseq64_s1")]
    assert len(picked) == 18
    if libzstd is not None:
        picked += local_tail_frames(libzstd)[::4]               # (131087 at level 1, 131089 at 3, 131105 at 19)
    path = str(d / "frames.bin")
    with open(path, "wb") as f:
        f.write(len(picked).to_bytes(4, "little"))
        for _, fr, want in picked:
            f.write(len(fr).to_bytes(4, "little") + want.size.to_bytes(4, "little") + fr + want.tobytes())
    # ... and chunks through the kernels of the read path, LDS at its exact size: four planes (a tight-tail one among them) with the
    # frames that must be refused between their chunks
    batch = []
    for name, codec, ts, kw in [c for c in PLANES if c[0] in ("zstd_ts1_f0", "zstd_ts4_f1", "zstd_ts8_f2", "zstd_tail15")]:
        chunks, plane, _ = S.build_plane(name, codec, ts, kw)
        batch += [(c, p.tobytes(), 0) for c, p in zip(chunks, split_plane(chunks, plane))]
    for k, (name, fr, n, _) in enumerate(Z.bad_frames()):
        batch.insert(2 * k + 1, (S.chunk_of_streams(S.ZSTD, [(fr, np.zeros(n, np.uint8))]), bytes(n), 1))
    cpath = str(d / "chunks.bin")
    with open(cpath, "wb") as f:
        f.write(len(batch).to_bytes(4, "little"))
        for c, px, refused in batch:
            f.write(len(c).to_bytes(4, "little") + len(px).to_bytes(4, "little") + c[8:12] + refused.to_bytes(4, "little") + c + px)
    for order in ORDERS:
        r = subprocess.run([exe, path, cpath, str(order)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(picked)), "ok", str(len(batch))], (order, r.stdout[-2000:] + r.stderr[-3000:])


# ---- chunks -----------------------------------------------------------------------------------------------------------------------
def test_chunk_header_is_the_oracles():
    data = (np.arange(40000) % 7).astype(np.uint8)
    if not O.zstd_available():
        pytest.skip("the checker writes zstd chunks with the box's libzstd: none here")
    for ts in (1, 2, 4, 8):
        for filt in (S.NOFILTER, S.SHUFFLE, S.BITSHUFFLE):
            for split in (False, True):
                bs = 4096
                p = O.cparams(ts, clevel=5, blocksize=bs, compcode=O.ZSTD, splitmode=O.ALWAYS_SPLIT if split else O.NEVER_SPLIT,
                              filters=(0, 0, 0, 0, 0, filt))
                r, chunk = O.compress(p, data)
                assert r > 0 and not chunk[2] & 0x02
                assert bytes(S.header(S.ZSTD, ts, data.size, bs, r, filt, split)) == chunk[:32], (ts, filt, split)


@pytest.mark.parametrize("case", PLANES, ids=[c[0] for c in PLANES])
@in_every_write_order
def test_generated_chunks_every_form(case, zstd_read_path, write_order):
    name, codec, ts, kw = case
    chunks, plane, counts = S.build_plane(name, codec, ts, kw)
    assert counts["coded"] >= (2 if kw["policy"] == "all" else 3), counts
    parts = split_plane(chunks, plane)
    if O.zstd_available() and zstd_read_path == "planned" and write_order == 0:
        for c, p in zip(chunks, parts):
            r, out = O.decompress(c)
            assert r == p.size and np.array_equal(out, p)
    rc, st, raw, raw_off = emu_batch(chunks)
    if kw["blocksize"] > 163840:
        # (blocks beyond LDS: the normal planner refuses the batch and the engine takes the wide route -- test_generated_chunks_wide_route)
        assert rc == -7
        return
    assert rc == 0 and not any(st), (zstd_read_path, st)
    assert np.array_equal(raw, want_buffer(parts, raw_off, raw.size))


@pytest.mark.parametrize("case", PLANES, ids=[c[0] for c in PLANES])
@in_every_write_order
def test_generated_chunks_wide_route(ZW, case, write_order):
    """the route the engine takes with comp_size (blocks beyond LDS: the wide kernel leaves zstd blocks to the wide walk + replay)"""
    name, codec, ts, kw = case
    chunks, plane, _ = S.build_plane(name, codec, ts, kw)
    parts = split_plane(chunks, plane)
    rc, st, raw, raw_off = emu_batch(chunks, wide=ZW, order=write_order)
    assert rc == 0 and not any(st), st
    assert np.array_equal(raw, want_buffer(parts, raw_off, raw.size))


def test_every_frame_as_the_one_stream_of_a_chunk_in_one_batch(ZW, zstd_read_path, write_order, golden_dir):
    """what tests/test_gpu_zstd_streams.py sends to the GPU, here through the emulated kernels: every spec-built frame a chunk can
    carry, the golden libzstd frames up to 160 KiB and the encoder's frames of the mix streams, one stream per chunk, all chunks of
    up to 128 KiB + 33 in ONE batch (canaries around every output) in every form; the seven larger ones that fit LDS in a batch of
    their own in the planned form (Z.FORM_BLOCK_MAX says why), the three frames beyond LDS through the wide route"""
    cases = Z.frame_chunk_cases(golden_dir, E.zstd_encode)
    assert len(cases) >= 300 and {"frame_A", "kat|nibbles_16k|L1", "mix18"} - {c[0] for c in cases} == {"frame_A"}   # (frame A is longer than its output)
    normal = [c for c in cases if c[2].size <= Z.FORM_BLOCK_MAX]
    if zstd_read_path == "planned":
        large = [c for c in cases if Z.FORM_BLOCK_MAX < c[2].size <= Z.LDS_BLOCK_MAX]
        assert len(large) == 7
        rc, st, raw, raw_off = emu_batch([c for _, c, _ in large])
        assert rc == 0 and not st.any(), st
        assert np.array_equal(raw, want_buffer([w for _, _, w in large], raw_off, raw.size))
    rc, st, raw, raw_off = emu_batch([c for _, c, _ in normal])
    assert rc == 0 and not st.any(), [(n, int(s)) for (n, _, _), s in zip(normal, st) if s]
    want = want_buffer([w for _, _, w in normal], raw_off, raw.size)
    for (name, _, w), o in zip(normal, raw_off):
        assert np.array_equal(raw[o:o + w.size], w), name
    assert np.array_equal(raw, want)
    if zstd_read_path == "planned":
        wide = [c for c in cases if c[2].size > Z.LDS_BLOCK_MAX]
        assert len(wide) == 3
        rc, st, raw, raw_off = emu_batch([c for _, c, _ in wide], wide=ZW, order=write_order)
        assert rc == 0 and not st.any(), st
        assert np.array_equal(raw, want_buffer([w for _, _, w in wide], raw_off, raw.size))


@in_every_write_order
def test_bad_frames_in_a_batch_between_good_chunks(ZW, zstd_read_path, write_order):
    good, gplane, _ = S.build_plane(*PLANES[0][:3], PLANES[0][3], nchunks=1)
    batch, want, bad_at = [], [], []
    for name, fr, n, code in Z.bad_frames():
        batch += [good[0], S.chunk_of_streams(S.ZSTD, [(fr, np.zeros(n, np.uint8))])]
        want += [gplane, None]
        bad_at.append((len(batch) - 1, name, code))
    batch.append(good[0])
    want.append(gplane)
    for wide in (None, ZW):
        rc, st, raw, raw_off = emu_batch(batch, wide=wide, order=write_order)
        assert rc == 0
        for k, name, code in bad_at:
            assert st[k] < 0 and (code is None or st[k] == code), (name, st[k])
        nb, _ = sizes(batch)
        for k, p in enumerate(want):
            if p is not None:
                assert st[k] == 0 and np.array_equal(raw[raw_off[k]:raw_off[k] + p.size], p), k
            # canaries around every output, the refused chunks' too
            assert (raw[raw_off[k] - 48:raw_off[k]] == CANARY).all() and (raw[raw_off[k] + nb[k]:raw_off[k] + nb[k] + 48] == CANARY).all(), k


def test_sequence_bit_streams_longer_than_a_lanes_lds(tmp_path_factory):
    """the emulator built with 256 bytes of a job's bit stream in the lane's LDS instead of 4 KiB (test_emu_zstd.py: every stream is
    refilled many times) runs the chunk tests of this file again, in the forms that have lanes.  (Built into a directory of its
    own: test_emu_zstd.py keeps its build of the same name in tests/emu, and a run of both files side by side must not write it twice.)"""
    lib = str(tmp_path_factory.mktemp("zstd_streams_stream256") / "libcimg_emu_stream256.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-w", "-fno-strict-aliasing", "-DCIMG_ZSTD_SEQ_STREAM=256",
                           "-I", CSRC, os.path.join(EMU, "emu.cpp"), "-o", lib])
    env = dict(os.environ, CIMG_EMU_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "test_generated_chunks_every_form and (planned or lanes)"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
