"""Idle waves place stored planes of busy waves (encode_kernel.h: encode_emit_own, EncodeArgs::placed), on the host emulator.

A stored plane of a chunk assembled inside the encode launch is a byte-select of the launch's input, so any wave may place it: a
wave with nothing of its own left takes blocks whose mark is not set, places their stored planes and sets the mark; an owner that
finds its block marked skips them.  Nothing is claimed -- a stale mark costs a plane written twice, with the same bytes.

The driver (tests/emu/helpers_emu.cpp) stops the waves of a launch between their codec phase and their placing phase and runs the
placing phases in a chosen order.  Under every schedule, under plane items, whole-block items and the mixed queue, and with the
switch off, the chunks must be the oracle's byte for byte, decode to the pixels and leave the bytes behind destsize alone; the
emulator's counters must show that the intended path produced them.  The same driver runs under AddressSanitizer / UBSan as a
stand-alone program with every chunk destination an allocation of exactly destsize (tests/emu/helpers_asan_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _emu as E
import _oracle as O
import _stored_cases as S

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_SRC = os.path.join(_EMU, "helpers_emu.cpp")
_LIB = os.path.join(_EMU, "libcimg_helpers_emu.so")
_MAIN = os.path.join(_EMU, "helpers_asan_main.cpp")
_EXE = os.path.join(_EMU, "helpers_asan")

PLAIN, HELPER_FIRST, HELPER_LAST, STALE = 0, 1, 2, 3
PLANES, WHOLE, MIXED = 0, 1, 2


def _deps():
    return [_SRC, E._SRC] + [os.path.join(E._CSRC, f) for f in os.listdir(E._CSRC) if f.endswith(".h")]


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def L():
    if _stale(_LIB, _deps()):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-I", E._CSRC,
                               "-I", _EMU, _SRC, "-o", _LIB])
    lib = C.CDLL(_LIB)
    vp = C.c_void_p
    lib.emu_helpers_compress_batch.argtypes = [C.POINTER(E.CParams), C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.emu_helpers_compress_batch.restype = C.c_int
    return lib


def _cases():
    """tests/_stored_cases.py, and what it does not have: three stored planes in a 4-byte type, a special-zero chunk between coded
    ones, a chunk that does not fit.  (name, typesize, filters, splitmode, pixels, chunk sizes, destsize per chunk, comp stride or
    None, stored streams left for placing, of those placed)"""
    rng = np.random.Generator(np.random.PCG64(20250107))
    out = []
    for name, ts, filters, split, raw, sizes, dest, stride, left, placed_ in S.cases():
        out.append((name, ts, filters, split, raw, sizes, [dest] * len(sizes), stride, left, placed_))
    # typesize 4: byte 3 of every element repeats a short pattern (coded), bytes 0 .. 2 are noise: three stored planes a block
    n = 3 * S.CHUNK
    f32 = rng.integers(0, 256, n, dtype=np.uint8)
    for b in range(n // S.BLOCK):
        blk = f32[b * S.BLOCK:(b + 1) * S.BLOCK].reshape(-1, 4)
        blk[:, 3] = np.resize(rng.integers(0, 256, 40 + b, dtype=np.uint8), len(blk))
    out.append(("j_three_stored_planes_f32", 4, S.SHUFFLE, S.AUTO, f32, [S.CHUNK] * 3, [S.CHUNK + 32] * 3, None, 36, 36))
    tiled16 = S._u8(S.synth.tiled_channel(np.float16, 1024, 192))
    z = np.concatenate([tiled16[:S.CHUNK], np.zeros(S.CHUNK, np.uint8), tiled16[S.CHUNK:2 * S.CHUNK]])
    out.append(("k_special_zero_between", 2, S.SHUFFLE, S.AUTO, z, [S.CHUNK] * 3, [S.CHUNK + 32] * 3, None, 8, 8))
    # the middle chunk's capacity holds neither its streams nor its pixels: cbytes 0, nothing of it placed
    out.append(("l_does_not_fit_between", 2, S.SHUFFLE, S.AUTO, tiled16, [S.CHUNK] * 3, [S.CHUNK + 32, 20000, S.CHUNK + 32], None, 12, 8))
    return out


CASES = _cases()
# per case: the stored streams that lie in chunks a helper may touch -- assembled in the launch, on a 4-byte boundary, regular layout
# (h: only chunk 0 is aligned; b, k, l: the memcpyed / special-zero / failed chunk is out; g: the chunk with a leftover block is out)
_HELPABLE = {
    "a_tiled_f16": 12, "b_random_chunk_memcpyed": 8, "c_natural_f16": 0, "d_zero": 0, "e_tiled_f32": 12, "f_nofilter_ts2": 12,
    "g_leftover_chunk_between": 8, "h_odd_comp_off": 4, "i_only_last_block": 1, "j_three_stored_planes_f32": 36,
    "k_special_zero_between": 8, "l_does_not_fit_between": 8,
}


@pytest.fixture(scope="module")
def expected():
    """The oracle's chunks of every case, computed once (b"" where the oracle says the chunk does not fit)."""
    want = {}
    for name, ts, filters, split, raw, sizes, dests, _, _, _ in CASES:
        po = O.cparams(ts, splitmode=split, filters=filters)
        off, chunks = 0, []
        for n, dest in zip(sizes, dests):
            r, c = O.compress(po, raw[off:off + n], destsize=dest)
            chunks.append(c[:r] if r > 0 else b"")
            off += n
        want[name] = chunks
    return want


def _compress(lib, p, raw, sizes, dests, stride, schedule, items, helpers):
    n = len(sizes)
    nb = np.asarray(sizes, np.int32)
    ds = np.asarray(dests, np.int32)
    raw_off = np.concatenate([[0], np.cumsum(nb[:-1], dtype=np.int64)]).astype(np.int64)
    stride = max(dests) + 64 if stride is None else stride
    comp_off = np.arange(n, dtype=np.int64) * stride
    comp = np.full(n * stride + 64, 0x5A, np.uint8)
    cbytes = np.zeros(n, np.int32)
    stats = (C.c_long * 5)()
    rc = lib.emu_helpers_compress_batch(C.byref(p), n, E._p(raw), E._p(raw_off), E._p(nb), E._p(comp), E._p(comp_off), E._p(ds),
                                        E._p(cbytes), schedule, items, helpers, stats)
    chunks = [comp[comp_off[i]:comp_off[i] + max(cbytes[i], 0)].tobytes() for i in range(n)]
    guard = [comp[comp_off[i] + dests[i]:comp_off[i] + stride] for i in range(n)]
    return rc, chunks, guard, tuple(stats)


@pytest.mark.parametrize("items", [PLANES, WHOLE, MIXED], ids=["planes", "whole", "mixed"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_helpers_place_stored_planes(L, expected, case, items):
    name, ts, filters, split, raw, sizes, dests, stride, want_left, want_placed = case
    helpable = _HELPABLE[name]
    p = E.cparams(ts, splitmode=split, filters=filters)
    chunks = None
    for schedule in (PLAIN, HELPER_FIRST, HELPER_LAST, STALE):
        for helpers in (1, 0):
            rc, chunks, guard, stats = _compress(L, p, raw, sizes, dests, stride, schedule, items, helpers)
            tag = (name, schedule, helpers, stats)
            assert rc == 0, tag
            assert chunks == expected[name], tag
            assert all((g == 0x5A).all() for g in guard), tag          # nothing written past a chunk's capacity
            left, placed, by_owner, by_helper, skipped = stats
            assert left == want_left and placed == by_owner + by_helper, tag
            if not helpers:
                # the switch: every wave its own, as before helpers existed
                assert (placed, by_owner, by_helper, skipped) == (want_placed, want_placed, 0, 0), tag
            elif schedule in (PLAIN, HELPER_LAST):
                # the owners were first: nothing left for a helper, nothing placed twice
                assert by_helper == 0 and skipped == 0 and by_owner == want_placed, tag
            elif schedule == HELPER_FIRST:
                # the helper took every plane it may touch, their owners skipped exactly those; the rest as ever
                assert by_helper == helpable and skipped == helpable and by_owner == want_placed - helpable, tag
                if helpable:
                    assert by_helper > 0 and skipped > 0, tag
            else:
                # the second helper worked from marks as they were before the first: every plane of theirs was placed twice
                assert by_helper == 2 * helpable and skipped == helpable and by_owner == want_placed - helpable, tag
                assert placed - want_placed == helpable, tag           # the duplicates
    live = [i for i, c in enumerate(chunks) if c]
    rc, status, outs = E.decompress_batch([chunks[i] for i in live], [sizes[i] for i in live], [S.BLOCK] * len(live))
    assert rc == 0 and not any(status)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for i, o in zip(live, outs):
        assert o.tobytes() == raw[offs[i]:offs[i] + sizes[i]].tobytes()


def test_cases_cover_what_the_helpers_must_keep_out_of(expected):
    """The case list has a memcpyed chunk, a special-zero chunk, a chunk that does not fit, a chunk off a 4-byte boundary and a
    chunk with a leftover block -- read from the oracle's chunks, not from the names."""
    flags = {name: [(c[2] if c else None, c[31] >> 4 if c else None) for c in chunks] for name, chunks in expected.items()}
    assert any(f is not None and f & 0x02 for f, _ in flags["b_random_chunk_memcpyed"])
    assert any(s == 1 for _, s in flags["k_special_zero_between"])
    assert any(f is None for f, _ in flags["l_does_not_fit_between"])
    by_name = {c[0]: c for c in CASES}
    assert by_name["h_odd_comp_off"][7] % 4 != 0
    assert any(n % S.BLOCK for n in by_name["g_leftover_chunk_between"][5])
    assert by_name["f_nofilter_ts2"][2] == S.NOFILTER and by_name["j_three_stored_planes_f32"][1] == 4


def test_helpers_sanitized():
    """The driver under AddressSanitizer / UBSan as a program of its own: every chunk destination an allocation of exactly
    destsize, the LDS of every wave exactly the launch's."""
    if _stale(_EXE, _deps() + [_MAIN]):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0",
                               "-std=c++17", "-fno-strict-aliasing", "-I", E._CSRC, "-I", _EMU, _MAIN, _SRC, "-o", _EXE])
    r = subprocess.run([_EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "helpers asan ok" in r.stdout, r.stdout
