"""The pack kernel (csrc/pack_kernel.h: a batched gather copy of variable-sized pieces) on the host lane emulator against numpy.

tests/emu/pack_emu.cpp is compiled here into a library in a pytest temp directory with the flags of tests/emu/Makefile; the size and
misalignment grid runs once more in an AddressSanitizer / UBSan build (host code only) where every piece is an allocation of exactly
its size (tests/emu/pack_asan_main.cpp).  Every call's destination is canary-filled: the bytes between and around the pieces must
come back unchanged.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _pack import CANARY, ERR_INVALID_PARAM, LARGE, SMALL, expected, grid, layout

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
FLAGS = ["-std=c++17", "-fPIC", "-Wall", "-Wextra", "-fno-strict-aliasing", "-I", CSRC]


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack_emu") / "libpack_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, os.path.join(EMU, "pack_emu.cpp"), "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.pkemu_pack.argtypes = [C.c_int, vp, vp, vp, vp]
    L.pkemu_tiles.argtypes = [C.c_int, vp, vp, vp, vp]
    L.pkemu_tiles.restype = C.c_int64
    L.pkemu_write_order.argtypes = [C.c_int]
    return L


def _aligned(size, fill=None):
    """uint8 array of `size` bytes whose first byte is 16-byte aligned"""
    raw = np.empty(size + 16, np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:size]
    if fill is not None:
        a[:] = fill
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(P, cases, rng, fn=None):
    so, do, nb, ssz, dsz = layout(cases)
    src = _aligned(ssz)
    src[:] = rng.integers(0, 256, ssz, dtype=np.uint8)
    dst = _aligned(dsz, CANARY)
    ptrs = (src.ctypes.data + so).astype(np.uint64)
    rc = (fn or P.pkemu_pack)(len(cases), _p(ptrs), _p(nb), _p(dst), _p(do))
    return rc, src, dst, so, do, nb, dsz


def test_every_size_and_misalignment_one_piece_a_call(P):
    rng = np.random.default_rng(11)
    for order in (0, 1, 2):                                   # lanes that store visit in ascending / descending / shuffled order
        P.pkemu_write_order(order)
        for case in grid():
            if order and case[0] in LARGE:
                continue
            rc, src, dst, so, do, nb, dsz = run(P, [case], rng)
            assert rc == 0, case
            assert np.array_equal(dst, expected(src, so, do, nb, dsz)), (case, order)
    P.pkemu_write_order(0)


def test_whole_grid_in_one_call(P):
    rng = np.random.default_rng(12)
    cases = list(grid())
    rc, src, dst, so, do, nb, dsz = run(P, cases, rng)
    assert rc == 0
    assert np.array_equal(dst, expected(src, so, do, nb, dsz))


@pytest.mark.parametrize("npieces", [1, 2, 3, 64, 65, 1000, 3000])
def test_one_to_three_thousand_pieces(P, npieces):
    rng = np.random.default_rng(npieces)
    sizes = rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 100, 4095, 20000, 65537], npieces)
    cases = [(int(n), int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in sizes]
    rc, src, dst, so, do, nb, dsz = run(P, cases, rng)
    assert rc == 0
    assert np.array_equal(dst, expected(src, so, do, nb, dsz))


def test_work_follows_bytes_not_pieces(P):
    """tiles: one per 16 KiB of a piece's middle, at least one per non-empty piece -- a 4 MiB piece is cut like 256 pieces of 16 KiB"""
    rng = np.random.default_rng(13)
    big = run(P, [((4 << 20), 0, 0)], rng, fn=P.pkemu_tiles)[0]
    small = run(P, [(16384, 0, 0)] * 256, rng, fn=P.pkemu_tiles)[0]
    assert big == small == 256
    assert run(P, [(0, 3, 5), (40, 3, 5), (0, 0, 0)], rng, fn=P.pkemu_tiles)[0] == 1          # empty pieces cost nothing
    assert run(P, [(16384 + 32, 0, 1)], rng, fn=P.pkemu_tiles)[0] == 2


def test_overlapping_ranges_are_refused_and_nothing_is_written(P):
    buf = _aligned(4096, CANARY)
    base = buf.ctypes.data

    def call(srcs, sizes, dsts):
        ptrs = np.array([base + s for s in srcs], np.uint64)
        nb = np.array(sizes, np.int32)
        do = np.array(dsts, np.int64)
        return P.pkemu_pack(len(srcs), _p(ptrs), _p(nb), _p(buf), _p(do))

    assert call([0], [100], [50]) == ERR_INVALID_PARAM                    # destination inside its own source
    assert call([0], [100], [99]) == ERR_INVALID_PARAM                    # by one byte
    assert call([0, 1000], [100, 100], [2000, 2050]) == ERR_INVALID_PARAM  # two destinations
    assert call([0, 2000], [100, 100], [2050, 3000]) == ERR_INVALID_PARAM  # piece 0's destination over piece 1's source
    assert call([0, 1000], [-1, 100], [2000, 3000]) == ERR_INVALID_PARAM
    assert (buf == CANARY).all()
    buf[:200] = np.arange(200, dtype=np.uint8)
    assert call([0, 50], [100, 100], [1000, 2000]) == 0                   # sources may overlap each other
    assert call([0], [100], [100]) == 0                                   # touching is not overlapping
    assert np.array_equal(buf[1000:1100], np.arange(100, dtype=np.uint8)) and np.array_equal(buf[2000:2100], np.arange(50, 150, dtype=np.uint8))
    assert np.array_equal(buf[100:200], np.arange(100, dtype=np.uint8))
    assert call([0, 0], [0, 0], [0, 0]) == 0                              # empty pieces are skipped before any check


def test_grid_under_address_sanitizer(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack_asan") / "pack_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                           os.path.join(EMU, "pack_asan_main.cpp"), os.path.join(EMU, "pack_emu.cpp"), "-o", out])
    r = subprocess.run([out] + [str(n) for n in SMALL + LARGE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(256 * len(SMALL) + 4 * len(LARGE))], r.stdout
