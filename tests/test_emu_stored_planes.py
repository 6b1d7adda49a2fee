"""Stored planes of chunks assembled inside the encode launch (encode_kernel.h: REC_RAW_SRC), on the host emulator: the encoder
leaves a record and nothing in the scratch slot, and the wave that places the plane selects it from the launch's input again.
The chunks must be the oracle's byte for byte, decode to the pixels, and the emulator's counters must say that the path under
test -- not the scratch path, which gives the same bytes -- produced them.

The emulator runs the waves of a launch one after the other and rotates their number (1, 38, 75) from launch to launch; every
case runs often enough to see each, under the three item forms of the split launch (planes, whole blocks, mixed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _emu as E
import _oracle as O
import _stored_cases as S

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "stored_emu.cpp")
_LIB = os.path.join(_HERE, "emu", "libcimg_stored_emu.so")


@pytest.fixture(scope="module")
def L():
    deps = [_SRC, E._SRC] + [os.path.join(E._CSRC, f) for f in os.listdir(E._CSRC) if f.endswith(".h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-I", E._CSRC,
                               "-I", os.path.dirname(_SRC), _SRC, "-o", _LIB])
    lib = C.CDLL(_LIB)
    vp = C.c_void_p
    lib.emu_stored_compress_batch.argtypes = [C.POINTER(E.CParams), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.emu_stored_compress_batch.restype = C.c_int
    lib.emu_set_block_items.argtypes = [C.c_int]
    yield lib
    lib.emu_set_block_items(1)


CASES = S.cases()


@pytest.fixture(scope="module")
def expected():
    """The oracle's chunks of every case, computed once."""
    want = {}
    for name, ts, filters, split, raw, sizes, dest, _, _, _ in CASES:
        po = O.cparams(ts, splitmode=split, filters=filters)
        off, chunks = 0, []
        for n in sizes:
            r, c = O.compress(po, raw[off:off + n], destsize=dest)
            assert r == len(c) and r > 0
            chunks.append(c)
            off += n
        want[name] = chunks
    return want


def _compress(lib, p, raw, sizes, dest, stride):
    n = len(sizes)
    nb = np.asarray(sizes, np.int32)
    ds = np.full(n, dest, np.int32)
    raw_off = np.concatenate([[0], np.cumsum(nb[:-1], dtype=np.int64)]).astype(np.int64)
    stride = dest + 64 if stride is None else stride
    comp_off = np.arange(n, dtype=np.int64) * stride
    comp = np.full(n * stride + 64, 0x5A, np.uint8)
    cbytes = np.zeros(n, np.int32)
    stats = (C.c_long * 2)()
    rc = lib.emu_stored_compress_batch(C.byref(p), n, E._p(raw), E._p(raw_off), E._p(nb), E._p(comp), E._p(comp_off), E._p(ds),
                                       E._p(cbytes), stats)
    chunks = [comp[comp_off[i]:comp_off[i] + max(cbytes[i], 0)].tobytes() for i in range(n)]
    guard = [comp[comp_off[i] + dest:comp_off[i] + stride] for i in range(n)]
    return rc, chunks, guard, (stats[0], stats[1])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stored_planes_are_placed_from_the_source(L, expected, case):
    name, ts, filters, split, raw, sizes, dest, stride, want_left, want_placed = case
    p = E.cparams(ts, splitmode=split, filters=filters)
    for call in range(6):                                    # wave counts 1, 38, 75 (a two-launch batch advances the rotation by two)
        L.emu_set_block_items((1, 2, 0)[call % 3] if call < 3 else (2, 0, 1)[call % 3])
        rc, chunks, guard, stats = _compress(L, p, raw, sizes, dest, stride)
        assert rc == 0, (name, call)
        assert chunks == expected[name], (name, call)
        assert all((g == 0x5A).all() for g in guard), (name, call)      # nothing written past a chunk's capacity
        assert stats == (want_left, want_placed), (name, call, stats)
    rc, status, outs = E.decompress_batch(chunks, sizes, [S.BLOCK] * len(sizes))
    assert rc == 0 and not any(status)
    assert np.concatenate(outs).tobytes() == raw.tobytes()
