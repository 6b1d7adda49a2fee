"""BloscLZ with blocks up to 256 KiB on the host lane emulator: blosclz_wide_encode and the BloscLZ instance of the wide encode wave
(csrc/wide_kernel.h), and the planner flag that admits them (csrc/wide_plan.h).

tests/emu/blosclz_wide_emu.cpp is compiled here with tests/emu/emu.cpp into a library in a pytest temp directory, with the flags of
tests/emu/Makefile.  Checked:
  * every vector of tests/golden/blosclz_wide_kat.npz (BloscLZ 2.3.0 on streams of 65 535 .. 262 144 bytes,
    make_blosclz_wide_golden.py) and of blosclz_kat.npz (128 .. 65 535 bytes) through blosclz_wide_encode, under the three lane
    orders of the emulator,
  * the tight-capacity rule (cap = need: same bytes; cap = need - 1: 0; need = the oracle's),
  * whole chunks -- planner with the flag set, the wave, the emulated layout / emit -- against the oracle's chunks byte for byte,
    and back through the wide decoder,
  * the flag left unset still refuses BloscLZ (what wide_emu.cpp, which has the LZ4 instance alone, relies on),
  * a stand-alone AddressSanitizer / UBSan program (tests/emu/blosclz_wide_asan_main.cpp): no load outside a stream.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from _blosclz_wide import CHUNKS, chunk_case, load_kat, load_stream_inputs
from cimg import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
ERR_CODEC_SUPPORT = -7


class CParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32),
                ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("blosclz_wide_emu") / "libblosclz_wide_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-fno-strict-aliasing",
                           "-I", CSRC, os.path.join(EMU, "emu.cpp"), os.path.join(EMU, "blosclz_wide_emu.cpp"), "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.bwemu_blosclz_encode.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.bwemu_compress_batch.argtypes = [C.POINTER(CParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bwemu_decompress_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    yield L
    L.emu_set_write_order(0)
    L.bwemu_set_blosclz_flag(1)


@pytest.fixture(scope="module")
def kat():
    return load_kat()


@pytest.fixture(scope="module")
def stream_inputs(kat):
    return load_stream_inputs(kat)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def encode(W, src, clevel, cap=None, in_place=1):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    cap = src.size if cap is None else cap
    out = np.zeros(max(cap, 1) + 64, np.uint8)
    need = C.c_int(0)
    r = W.bwemu_blosclz_encode(_p(src), src.size, _p(out), cap, clevel, in_place, C.byref(need))
    return r, out[:max(r, 0)].tobytes(), need.value


def test_golden_covers_the_far_limits(kat):
    """What the file pins, independent of any encoder: the second copy is a match while d < MAX_FARDISTANCE = 73 725 and literals
    from there on; the offset grows from two to four bytes between d = 8191 and 8192."""
    size = {d: int(kat[f"len|far|100000|{d}|9"]) for d in (8190, 8191, 8192, 8193, 65535, 65536, 73722, 73723, 73724, 73725, 73726, 73727, 73728, 90000)}
    assert (size[73724], size[73725]) == (5753, 5959)          # with and without the far match
    assert all(size[d] == size[73724] for d in (65535, 65536, 73722, 73723))
    assert all(size[d] > size[73724] + 100 for d in (73726, 73727, 73728, 90000))
    assert size[8192] - size[8191] == 2 and size[8190] == size[8191] and size[8192] == size[8193]
    assert int(kat["len|far|262144|73724|9"]) < int(kat["len|far|262144|73725|9"])
    assert int(kat["len|random|131072|9"]) == 0 and int(kat["len|constant|131072|9"]) > 0
    for n in (65535, 65536, 65537):
        assert int(kat[f"len|steps|{n}|9"]) > 0


@pytest.mark.parametrize("order", [0, 1, 2])
def test_wide_vectors_match_blosclz(W, kat, stream_inputs, order):
    W.emu_set_write_order(order)
    try:
        coded = 0
        for key in kat["cases"]:
            name, clevel = str(key).rsplit("|", 1)
            n, clevel = int(name.split("|")[1]), int(clevel)
            src = stream_inputs[name]
            assert src.size == n
            r, data, need = encode(W, src, clevel, in_place=order != 1)
            assert r == int(kat["len|" + str(key)]), key
            assert hashlib.sha256(data).hexdigest() == str(kat["sha256|" + str(key)]), key
            assert need == (max(66, r + 1) if r else 0), key
            coded += r > 0
        assert coded >= 100
    finally:
        W.emu_set_write_order(0)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_normal_path_vectors_match_blosclz(W, golden_dir, order):
    """A wide batch sends every stream through the wide kernel, short leftover blocks included: the vectors of the normal-path
    encoder (128 .. 65 535 bytes) hold for this one too."""
    small = np.load(os.path.join(golden_dir, "blosclz_kat.npz"))
    W.emu_set_write_order(order)
    try:
        for key in small["cases"]:
            fname, n, clevel = str(key).split("|")
            src = small[f"in|{fname}|{n}"]
            r, data, _ = encode(W, src, int(clevel))
            assert data == small["out|" + str(key)].tobytes(), key
            assert r == len(data)
    finally:
        W.emu_set_write_order(0)


def test_short_streams_match_the_oracle(W):
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 66, 67, 100, 127):
        for src in (np.zeros(n, np.uint8), rng.integers(0, 3, n, dtype=np.uint8), np.resize(np.arange(7, dtype=np.uint8), n)):
            for clevel in (1, 4, 9):
                for cap in (n, 66, 65, 200):
                    ro, want, need_o = O.blosclz_compress(src, clevel=clevel, cap=cap, want_need=True)
                    r, data, need = encode(W, src, clevel, cap=cap)
                    assert (r, data) == (max(ro, 0), want), (n, clevel, cap)
                    assert need == (need_o if ro > 0 else 0)


def test_tight_capacity(W, kat, stream_inputs):
    done = 0
    for name in ("steps|65536", "tiled_u16_hi|131072", "far|100000|73724", "far|100000|8192", "period|262144", "steps|200001"):
        src = stream_inputs[name]
        for clevel in (5, 9):
            if int(kat[f"len|{name}|{clevel}"]) == 0:              # (BloscLZ gives up on it at this level: no capacity edge)
                continue
            ro, want, need_o = O.blosclz_compress(src, clevel=clevel, want_need=True)
            r, data, need = encode(W, src, clevel)
            assert ro > 0 and (r, data, need) == (ro, want, need_o), (name, clevel)
            r2, data2, _ = encode(W, src, clevel, cap=need)
            assert (r2, data2) == (ro, want), (name, clevel)
            assert encode(W, src, clevel, cap=need - 1)[0] == 0, (name, clevel)
            assert O.blosclz_compress(src, clevel=clevel, cap=need - 1)[0] == 0
            done += 1
    assert done >= 8


# ---- whole chunks ------------------------------------------------------------------------------------------------------------

def cparams(ts, blocksize, compcode=O.BLOSCLZ, clevel=9, splitmode=O.AUTO_SPLIT, filt=O.SHUFFLE):
    p = CParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    return p


def compress(W, p, raw, destsize=None):
    raw = np.ascontiguousarray(raw).view(np.uint8).ravel()
    nbytes = np.array([raw.size], np.int32)
    raw_off = np.zeros(1, np.int64)
    dest = np.array([raw.size + 32 if destsize is None else destsize], np.int32)
    comp_off = np.zeros(1, np.int64)
    comp = np.zeros(int(dest[0]) + 64, np.uint8)
    cb = np.zeros(1, np.int32)
    # the pixels end with their allocation's last byte: an unshuffled stream is read in place
    exact = np.empty(raw.size, np.uint8)
    exact[:] = raw
    rc = W.bwemu_compress_batch(C.byref(p), 1, _p(exact), _p(raw_off), _p(nbytes), _p(comp), _p(comp_off), _p(dest), _p(cb))
    return rc, int(cb[0]), comp[:max(int(cb[0]), 0)].tobytes()


def decompress(W, chunk):
    nb, _, bs = O.cbuffer_sizes(np.frombuffer(chunk[:32], np.uint8))
    comp = np.frombuffer(chunk + bytes(64), np.uint8).copy()
    raw = np.full(nb + 64, 0x5A, np.uint8)
    st = np.zeros(1, np.int32)
    z64, nb32, bs32, cs32 = np.zeros(1, np.int64), np.array([nb], np.int32), np.array([bs], np.int32), np.array([len(chunk)], np.int32)
    rc = W.bwemu_decompress_batch(1, _p(comp), _p(z64), _p(cs32), _p(nb32), _p(bs32), _p(raw), _p(z64), _p(st))
    return rc, int(st[0]), raw[:nb].tobytes()


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_chunks_equal_the_oracle(W, name):
    for clevel in ((9, 5) if name in ("u8_natural_b262144", "f16_tiled_b262144") else (9,)):
        raw, ts, blk, split, filt, want = chunk_case(name, clevel)
        rc, cb, chunk = compress(W, cparams(ts, blk, clevel=clevel, splitmode=split, filt=filt), raw)
        assert rc == 0 and W.bwemu_last_route() == 2, name
        assert cb == len(want) and chunk == want, (name, clevel)
        if name == "u8_noise_b262144":
            assert chunk[2] & 0x2                              # memcpyed
        rc, st, back = decompress(W, chunk)
        assert rc == 0 and st == 0 and back == raw.tobytes(), name


def test_destsizes_around_cbytes(W):
    """The running-destsize rule and the memcpyed fallback: the oracle's answer at four capacities around its own cbytes."""
    raw = synth.natural_channel(np.float16, 1024, 512).view(np.uint8).ravel()
    op = O.cparams(2, blocksize=262144, compcode=O.BLOSCLZ)
    full, _ = O.compress(op, raw)
    assert 0 < full < raw.size
    seen = set()
    for dest in (full + 1, full, full - 1, full - 4096):
        r, want = O.compress(op, raw, destsize=dest)
        rc, cb, chunk = compress(W, cparams(2, 262144), raw, destsize=dest)
        assert rc == 0 and W.bwemu_last_route() == 2
        assert cb == max(r, 0) and chunk == want, dest
        seen.add(r > 0)
    assert seen == {True, False}


def test_flag_unset_still_refuses(W):
    raw = synth.natural_channel(np.uint8, 1024, 512).ravel()
    W.bwemu_set_blosclz_flag(0)
    try:
        rc, _, _ = compress(W, cparams(1, 131072), raw)
        assert rc == ERR_CODEC_SUPPORT
        rc, _, _ = compress(W, cparams(1, 131072, compcode=O.LZ4), raw)     # (the other codecs do not look at the flag)
        assert rc == 0 and W.bwemu_last_route() == 1
    finally:
        W.bwemu_set_blosclz_flag(1)
    # with it: still no bitshuffle on the wide route, no blocks above 256 KiB; and what the normal planner takes stays with it
    assert compress(W, cparams(1, 262144, filt=O.BITSHUFFLE), raw)[0] == ERR_CODEC_SUPPORT
    assert compress(W, cparams(1, 262145), raw)[0] == ERR_CODEC_SUPPORT
    rc, cb, chunk = compress(W, cparams(1, 32768), raw)
    assert rc == 0 and W.bwemu_last_route() == 0
    assert chunk == O.compress(O.cparams(1, blocksize=32768, compcode=O.BLOSCLZ), raw)[1]


def test_streams_under_address_sanitizer(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("blosclz_wide_asan") / "blosclz_wide_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(EMU, "blosclz_wide_asan_main.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 300, r.stdout
