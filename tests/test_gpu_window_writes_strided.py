"""Strided window writes on the MI355X: cimg_update_windows_strided_device / _host (csrc/update_plan.h over StridedWindowSpec,
cimg_update_patch_strided in csrc/update_kernel.h).

New chunks must equal a from-scratch compress of the edited pixels -- numpy assignment plane[origin + r * row_pitch + c * col_pitch] =
src[r, c] in call order into the oracle's decode --: the oracle's for lz4 and blosclz, the engine's own for lz4hc, zstd and wide
blocks.  The stats show which blocks were staged and re-encoded, the timing ids which patch kernel ran."""
import numpy as np
import pytest

import _oracle as O
import _window_writes_strided as S
from _window_writes import BLOSCLZ, LZ4, LZ4HC, ZSTD
from _windows import ERR_INVALID_PARAM, concat, oracle_chunks, sizes
from cimg import hip, synth

pytestmark = pytest.mark.gpu
CANARY = 0x5A


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def pixels(ts, elems, seed=0):
    rng = np.random.default_rng(seed)
    raw = synth.tiled_channel(np.float16, 64, max(elems * ts // 128 + 1, 1)).view(np.uint8).ravel()[:elems * ts].copy()
    raw[::97] ^= rng.integers(0, 255, raw[::97].size, dtype=np.uint8)
    return raw


def run_device(eng, p, chunks, specs, src, ds, strided=True):
    """-> (rc, status, new chunks, new_cbytes, every byte of d_new outside the new chunks is still the canary)"""
    buf, off, cs = concat(chunks)
    nb, bs = sizes(chunks)
    ds = np.asarray(ds, np.int32)
    new_off = 64 + np.concatenate([[0], np.cumsum((ds.astype(np.int64) + 63) // 64 * 64 + 64)[:-1]]).astype(np.int64)   # canaries around each
    total = int(new_off[-1]) + int(ds[-1]) + 64
    d_comp, d_src, d_new = eng.alloc(buf.size), eng.alloc(max(src.size, 1)), eng.alloc(total)
    d_comp.upload(buf)
    d_src.upload(src)
    d_new.upload(np.full(total, CANARY, np.uint8))
    fn = eng.update_windows_strided_device if strided else eng.update_windows_device
    rc, ncb, st = fn(p, d_comp.ptr, off, nb, bs, ds, specs, d_src.ptr, d_new.ptr, new_off, comp_size=cs, check=False)
    out = d_new.download()
    back = d_comp.download()
    d_comp.free(); d_src.free(); d_new.free()
    assert np.array_equal(back, buf), "the input chunks were modified"
    new = [out[o:o + c].tobytes() if c > 0 else None for o, c in zip(new_off, ncb)]
    keep = np.ones(total, bool)
    if rc != ERR_INVALID_PARAM:                   # (a refused call writes nothing at all; any other only inside the chunks' capacities)
        for o, d in zip(new_off, ds):
            keep[o:o + d] = False
    return rc, st, new, ncb, bool((out[keep] == CANARY).all())


def both(eng, p, chunks, specs, src, ds, strided=True):
    rc, st, new, ncb, intact = run_device(eng, p, chunks, specs, src, ds, strided)
    assert intact, "bytes outside the new chunks were written"
    yield "device", rc, st, new, ncb, eng.update_stats()
    fn = eng.update_windows_strided_host if strided else eng.update_windows_host
    before = [bytes(c) for c in chunks]
    rc, new, st = fn(p, chunks, ds, specs, src, check=False)
    assert before == [bytes(c) for c in chunks], "the input chunks were modified"
    yield "host", rc, st, new, np.array([len(c) if c else 0 for c in new], np.int32), eng.update_stats()


_cases = {}


def case(ts, codec=LZ4, filt=1, split=3, clevel=5):
    key = (ts, codec, filt, split, clevel)
    if key not in _cases:
        po = O.cparams(ts, clevel=clevel, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
        chunks = oracle_chunks(po, pixels(ts, S.ELEMS), S.CHUNK_ELEMS * ts)
        p = hip.cparams(ts, clevel=clevel, blocksize=8192, compcode=codec, splitmode=split, filters=(0, 0, 0, 0, 0, filt))
        _cases[key] = (po, p, chunks, [S.CHUNK_ELEMS * ts + 32] * len(chunks))
    return _cases[key]


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ])
@pytest.mark.parametrize("ts,filt,split", S.MATRIX)
def test_matrix_matches_oracle(eng, codec, ts, filt, split):
    po, p, chunks, ds = case(ts, codec, filt, split)
    specs, src = S.source(S.matrix_windows(ts), ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    nb, bs = sizes(chunks)
    blocks = len(S.touched_blocks(specs, nb, bs, ts))
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and not st.any(), (how, rc, st, eng.last_error())
        assert new == want, how
        if stats["chunks_whole"] == 0:
            assert stats["blocks_encoded"] == blocks, (how, stats, blocks)


@pytest.mark.parametrize("codec,bs,clevel", [(LZ4HC, 8192, 5), (ZSTD, 8192, 5), (LZ4, 131072, 9), (LZ4, 262144, 9), (ZSTD, 262144, 5),
                                             (LZ4, 8192, 0)])
def test_other_routes_match_engine_compress(eng, codec, bs, clevel):
    ts = 4
    chunk = 1 << 20
    raw = pixels(ts, (3 * chunk + 40000) // ts)
    p = hip.cparams(ts, clevel=clevel, blocksize=bs, compcode=codec)
    nb = [min(chunk, raw.size - o) for o in range(0, raw.size, chunk)]
    ds = [chunk + 32] * len(nb)
    chunks = eng.compress_host(p, raw, nb, ds)
    elems = raw.size // ts
    n = len(nb)
    wins = [S.win(100000 + 7, 100, 130, row_pitch=3000, col_pitch=3, nchunks=n), S.win(100000 + 5000, 300, 40, row_pitch=1000, nchunks=n),
            S.win(9, 4, 1, col_pitch=chunk // ts + 11, nchunks=n), S.win(elems - 19, 10, 1, col_pitch=2, nchunks=n)]
    wins += [S.win(400000 + 37 * k, 1, 1, nchunks=n) for k in range(40)] + [S.win(400000 + 37 * 5, 1, 1, nchunks=n)]
    specs, src = S.source(wins, ts)
    comp = lambda piece, d: eng.compress_host(p, np.ascontiguousarray(piece), [piece.size], [d])[0]     # noqa: E731
    want, _ = S.expected(None, chunks, specs, ts, src, ds, compress=comp, planes={0: raw})
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and not st.any(), (how, rc, eng.last_error())
        assert new == want, how
        if codec == LZ4HC:
            assert stats["chunks_whole"] == 0 and stats["blocks_encoded"] > 0
        elif codec == ZSTD or clevel == 0:
            assert stats["chunks_whole"] == sum(x is not None for x in want)
        elif bs == 262144:                        # (the short last chunk has one small block: spliced)
            assert stats["chunks_whole"] == sum(x is not None and b == bs for x, b in zip(want, sizes(chunks)[1]))


def unit_windows(ts, n, dup, seed=7):
    rng = np.random.default_rng(seed)
    epb = 8192 // ts
    at = epb + 3 + rng.choice(epb - 10, n, replace=False)
    at = np.concatenate([at, rng.choice(at, dup)])
    return [S.win(int(a), 1, 1) for a in at]


@pytest.mark.parametrize("ts", [2, 3])
@pytest.mark.parametrize("dup", [0, 20])
def test_unit_of_300_pixels(eng, ts, dup):
    """300 distinct 1 x 1 windows in one block (the disjoint schedule: more than four waves' worth), and the same with 20 duplicates
    (the ordered schedule: the last value wins)"""
    po, p, chunks, ds = case(ts)
    specs, src = S.source(unit_windows(ts, 300, dup), ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and new == want, (how, rc, eng.last_error())
        assert stats["blocks_decoded"] == 1 and stats["blocks_encoded"] == 1 and stats["chunks_whole"] == 0, (how, stats)


@pytest.mark.parametrize("ts", [1, 2, 3, 4])
def test_disjoint_unit_of_strided_windows(eng, ts):
    """windows with cpitch != typesize, more than 64 samples a row, no common byte, in one block: the per-element overlay under the
    disjoint schedule (the emulator test of the same name pins the schedule)"""
    po, p, chunks, ds = case(ts)
    specs, src = S.source(S.disjoint_strided_unit(ts), ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds)
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and new == want, (how, rc, eng.last_error())
        assert stats["blocks_decoded"] == 1 and stats["blocks_encoded"] == 1 and stats["chunks_whole"] == 0, (how, stats)


def plain_shapes(nchunks, W_=S.ROW, elems=S.ELEMS, chunk_elems=S.CHUNK_ELEMS):
    mid = chunk_elems // W_
    s = [dict(origin=elems // 2 + 5, row_pitch=1, width=1, height=1), dict(origin=3 * W_ + 7, row_pitch=W_, width=W_ - 20, height=1),
         dict(origin=W_ * 4 + 17, row_pitch=W_, width=1, height=60), dict(origin=W_ * 50, row_pitch=W_, width=W_, height=9),
         dict(origin=max(mid - 2, 0) * W_ + W_ - 37, row_pitch=W_, width=53, height=5),
         dict(origin=W_ * 70 + 3, row_pitch=W_, width=40, height=12), dict(origin=W_ * 75 + 20, row_pitch=W_, width=40, height=12),
         dict(origin=0, row_pitch=1, width=8192, height=1)]
    for d in s:
        d["chunk_first"], d["chunk_count"] = 0, nchunks
    return s


@pytest.mark.parametrize("ts,codec,clevel", [(1, LZ4, 5), (3, BLOSCLZ, 5), (4, LZ4, 5), (4, LZ4, 0)])
def test_col_pitch_1_equals_the_plain_call(eng, ts, codec, clevel):
    po, p, chunks, ds = case(ts, codec, clevel=clevel)
    specs, src = S.source(plain_shapes(len(chunks)), ts)
    for dsz in (ds, [len(c) + 8 for c in chunks]):
        a = list(both(eng, p, chunks, specs, src, dsz, strided=False))
        b = list(both(eng, p, chunks, S.with_col_pitch(specs), src, dsz, strided=True))
        for x, y in zip(a, b):
            assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3] and np.array_equal(x[4], y[4]), (x[0], x[1], y[1])
            assert x[5] == y[5], (x[0], x[5], y[5])


def launches(eng, kid):
    return eng.kernel_time(kid)[1]


def test_each_call_launches_its_own_patch_kernel(eng):
    ts = 2
    po, p, chunks, ds = case(ts)
    specs, src = S.source(plain_shapes(len(chunks)), ts)
    eng.enable_timing(1)
    try:
        list(both(eng, p, chunks, specs, src, ds, strided=False))            # (timing takes hold at the first batch step after it is enabled)
        for strided in (False, True):
            eng.reset_timing()
            for how, rc, st, new, ncb, stats in both(eng, p, chunks, S.with_col_pitch(specs) if strided else specs, src, ds, strided=strided):
                assert rc == 0
            plain, strd = launches(eng, hip.K_UPDATE_PATCH), launches(eng, hip.K_UPDATE_PATCH_STRIDED)
            assert (plain, strd) == ((0, 2) if strided else (2, 0)), (strided, plain, strd)
    finally:
        eng.enable_timing(0)
        eng.reset_timing()
    assert hip.KERNELS[hip.K_UPDATE_PATCH_STRIDED] == "cimg_update_patch_strided"
    assert hip.load().cimg_kernel_name(hip.K_UPDATE_PATCH_STRIDED).decode() == "cimg_update_patch_strided"


def test_refusals_and_a_damaged_chunk(eng):
    ts = 2
    po, p, chunks, ds = case(ts)
    src = np.zeros(1 << 16, np.uint8)
    ok = dict(S.win(11, 20, 5, row_pitch=100, col_pitch=3), out_off=0, out_pitch=20 * ts)
    bad = [dict(ok, col_pitch=0), dict(ok, row_pitch=57), dict(ok, origin=S.ELEMS - 57), dict(ok, out_pitch=20 * ts - 1), dict(ok, col_pitch=S.ELEMS),
           dict(ok, chunk_first=1), dict(ok, chunk_count=0)]
    for b in bad:
        for how, rc, st, new, ncb, stats in both(eng, p, chunks, [b], src, ds):
            assert rc == ERR_INVALID_PARAM and all(x is None for x in new) and not ncb.any(), (how, b)
    for q in (hip.cparams(4, clevel=5, blocksize=8192), hip.cparams(ts, clevel=5, blocksize=8192, compcode=BLOSCLZ),
              hip.cparams(ts, clevel=5, blocksize=4096), hip.cparams(ts, clevel=5, blocksize=8192, filters=(0, 0, 0, 0, 0, 2))):
        for how, rc, st, new, ncb, stats in both(eng, q, chunks, [ok], src, ds):
            assert rc == ERR_INVALID_PARAM and all(x is None for x in new), how
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, [ok], src, [ds[0], 31, ds[2]]):
        assert rc == ERR_INVALID_PARAM, how
    # a damaged touched chunk: its status, and the others are still written
    ts = 4
    po, p, chunks, ds = case(ts)
    c = bytearray(chunks[1])
    start = int.from_bytes(c[32 + 8:36 + 8], "little")
    c[start:start + 4] = (0x7FFF0000).to_bytes(4, "little")
    damaged = chunks[:1] + [bytes(c)] + chunks[2:]
    specs, src2 = S.source([S.win(100, (S.CHUNK_ELEMS + 4200) // 3, 1, col_pitch=3)], ts)
    want, _ = S.expected(po, chunks, specs, ts, src2, ds)
    for how, rc, st, new, ncb, stats in both(eng, p, damaged, specs, src2, ds):
        assert rc < 0 and st[1] < 0 and st[0] == 0 and new[1] is None and new[0] == want[0], how
    # the engine stays usable
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src2, ds):
        assert rc == 0 and new == want, how


def test_granularity_4096_float16(eng):
    """every 8th of 64 rows of a 4096-wide float16 plane, 32 KiB blocks (four 8 KiB rows each), one 4 MiB chunk: only the blocks that
    hold a written byte are staged and re-encoded -- counted here from the block geometry"""
    ts, W = 2, 4096
    rng = np.random.default_rng(3)
    plane = synth.tiled_channel(np.float16, W, 512).view(np.uint8).ravel().copy()
    plane[::301] ^= rng.integers(0, 255, plane[::301].size, dtype=np.uint8)
    chunk = 4 << 20
    po = O.cparams(ts)
    chunks = oracle_chunks(po, plane, chunk)
    assert len(chunks) == 1
    ds = [chunk + 32]
    p = hip.cparams(ts)
    x0, y0, w = 100, 66, 640
    spec = S.win(y0 * W + x0, (w + 3) // 4, 64 // 8, row_pitch=8 * W, col_pitch=4, nchunks=1)
    rows = [y0 + 8 * r for r in range(8)]
    blocks = {(y * W + x) * ts // 32768 for y in rows for x in (x0, x0 + 4 * ((w + 3) // 4 - 1))}       # a row lies inside one block
    assert len(blocks) == 8
    specs, src = S.source([spec], ts)
    want, _ = S.expected(po, chunks, specs, ts, src, ds, planes={0: plane})
    for how, rc, st, new, ncb, stats in both(eng, p, chunks, specs, src, ds):
        assert rc == 0 and new == want, how
        assert stats["blocks_encoded"] == len(blocks) and stats["blocks_decoded"] == len(blocks) and stats["chunks_whole"] == 0, (how, stats)
        if how == "host":
            assert stats["bytes_uploaded"] == len(chunks[0]) + spec["width"] * spec["height"] * ts
