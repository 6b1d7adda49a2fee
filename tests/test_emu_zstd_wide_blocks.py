"""zstd blocks up to 256 KiB on the host lane emulator: the wide zstd encoder (csrc/wide_kernel.h: zstd_wide_encode, frames of
more than one zstd block) and the wide zstd read path (cimg_decode_wide leaves zstd blocks pending; the walk and the replay out of
a device-memory slot, csrc/zstd_walk_kernel.h).

The kernels are compiled here with tests/emu/zstd_wide_emu.cpp (plus emu.cpp and wide_emu.cpp) into a library in a pytest temp
directory, with the flags of tests/emu/Makefile.  Checked:
  * single frames of 65 537 .. 262 144 bytes: libzstd (where there is one) and this repository's decoder read them back, and the
    encoder writes nothing past its budget,
  * round trips at 128 / 192 / 256 KiB blocks for float32 / float16 / uint8 at clevel 5 and 9,
  * chunks libzstd wrote with 160 / 192 / 256 KiB blocks (tests/golden/zstd_wide_kat.npz, make_zstd_wide_golden.py),
  * a corrupt frame and a truncated chunk, and the 256 KiB ceiling,
  * all of it in the three write orders of the emulator (csrc/wave.h, R2): what the encoders write is byte for byte what they write
    in the ascending order, and the read path returns the pixels in every order.
"""
import ctypes as C
import ctypes.util
import hashlib
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import _emu as E
import _oracle as O
from cimg import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "compressed-image_amd", "csrc")
EMU = os.path.join(HERE, "emu")
LZ4, ZSTD = 1, 5
ERR_CODEC_SUPPORT = -7


class CParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32),
                ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


@pytest.fixture(scope="module")
def Z(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("zstd_wide_emu") / "libzstd_wide_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-fno-strict-aliasing",
                           "-I", CSRC, os.path.join(EMU, "emu.cpp"), os.path.join(EMU, "wide_emu.cpp"),
                           os.path.join(EMU, "zstd_wide_emu.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    L = C.CDLL(out)
    vp = C.c_void_p
    L.zwemu_zstd_encode.argtypes = [vp, C.c_int, vp, C.c_int]
    L.zwemu_compress_batch.argtypes = [C.POINTER(CParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.zwemu_decompress_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def libzstd():
    name = ctypes.util.find_library("zstd")
    if not name:
        return None
    z = C.CDLL(name)
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    return z


ORDERS = (0, 1, 2)
_order = 0                 # the write order of the running test (in_every_write_order)


def set_order(Z, order):
    """both libraries keep an order: the wide one (Z) and the one behind _emu.zstd_decode"""
    Z.emu_set_write_order(order)
    E.set_write_order(order)


def use_order(Z, order):
    global _order
    _order = order
    set_order(Z, order)


def in_every_write_order(fn):
    """Run the test once in each order in which the emulator visits the lanes of a FOR_LANES_W body (csrc/wave.h, R2: ascending,
    descending, shuffled) and put the ascending order back.  The test keeps its name and its other arguments; one that names a
    `write_order` argument is told the order (every test here takes the library fixture Z, by name).  A result must not depend on it: positive frames give their input's BYTES in every
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
                use_order(kw["Z"], order)
                try:
                    fn(*args, **kw, **({"write_order": order} if wants else {}))
                except AssertionError as e:
                    raise AssertionError("in write order %d: %s" % (order, e)) from e
        finally:
            use_order(kw["Z"], 0)
    del run.__wrapped__
    run.__signature__ = sig.replace(parameters=[p for name, p in sig.parameters.items() if name != "write_order"])
    return run


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cparams(ts, blocksize, compcode=ZSTD, clevel=9, splitmode=3, filt=1):
    p = CParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = ts, clevel, blocksize, compcode, splitmode
    p.filters[5] = filt
    return p


def compress(Z, p, chunks):
    """chunks: list of uint8 arrays -> (rc, [chunk bytes]), written in the ascending order; in another write order the encoders
    run once more and must return the same code and the same bytes"""
    set_order(Z, 0)
    try:
        rc, out = compress_once(Z, p, chunks)
        if _order:
            set_order(Z, _order)
            assert compress_once(Z, p, chunks) == (rc, out), "chunk bytes depend on the write order %d" % _order
    finally:
        set_order(Z, _order)
    return rc, out


def compress_once(Z, p, chunks):
    n = len(chunks)
    raw = np.concatenate(chunks)
    nbytes = np.array([c.size for c in chunks], np.int32)
    raw_off = np.concatenate([[0], np.cumsum(nbytes[:-1])]).astype(np.int64)
    dest = (nbytes + 96).astype(np.int32)
    comp_off = np.concatenate([[0], np.cumsum(dest[:-1].astype(np.int64))]).astype(np.int64)
    comp = np.zeros(int(dest.sum()) + 64, np.uint8)
    cb = np.zeros(n, np.int32)
    rc = Z.zwemu_compress_batch(C.byref(p), n, _p(raw), _p(raw_off), _p(nbytes), _p(comp), _p(comp_off), _p(dest), _p(cb))
    if rc < 0:
        return rc, None
    return rc, [comp[comp_off[i]:comp_off[i] + cb[i]].tobytes() for i in range(n)]


def decompress(Z, chunks, sizes=None):
    """-> (rc, status array, [pixel bytes])"""
    n = len(chunks)
    hdr = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8)) for c in chunks]
    nbytes = np.array([h[0] for h in hdr], np.int32)
    bsize = np.array([h[2] for h in hdr], np.int32)
    comp_size = np.array([len(c) if sizes is None else sizes[i] for i, c in enumerate(chunks)], np.int32)
    comp = np.frombuffer(b"".join(chunks) + bytes(64), np.uint8).copy()
    comp_off = np.concatenate([[0], np.cumsum([len(c) for c in chunks[:-1]])]).astype(np.int64)
    raw_off = np.concatenate([[0], np.cumsum(nbytes[:-1])]).astype(np.int64)
    raw = np.full(int(nbytes.sum()) + 64, 0x5A, np.uint8)
    st = np.zeros(n, np.int32)
    rc = Z.zwemu_decompress_batch(n, _p(comp), _p(comp_off), _p(comp_size), _p(nbytes), _p(bsize), _p(raw), _p(raw_off), _p(st))
    return rc, st, [raw[raw_off[i]:raw_off[i] + nbytes[i]].tobytes() for i in range(n)]


def _streams():
    rng = np.random.Generator(np.random.PCG64(5))
    nat = np.ascontiguousarray(synth.natural_channel(np.uint8, 1024, 256)).ravel()
    tile = rng.integers(0, 256, 3000, dtype=np.uint8)
    return {
        "long_match_65537": np.concatenate([tile, np.full(65537 - 3000, 7, np.uint8)]),
        "long_literals_131072": np.concatenate([rng.integers(0, 256, 120000, dtype=np.uint8), np.tile(tile[:100], 111)[:11072]]),
        "far_offset_262144": np.concatenate([tile, rng.integers(0, 256, 256000, dtype=np.uint8), tile, tile[:144]]),
        "repeats_200000": np.tile(rng.integers(0, 256, 70001, dtype=np.uint8), 3)[:200000],
        "natural_plane_262144": nat[:262144].copy(),
        "natural_plane_150001": nat[:150001].copy(),
        "noise_100000": rng.integers(0, 256, 100000, dtype=np.uint8),
        "skewed_196608": np.minimum(rng.geometric(0.2, 196608), 255).astype(np.uint8),
        # the second 128 KiB zstd block continues a periodic pattern: one match covers it whole (a 131 072-byte match length)
        "periodic_262144": np.tile(np.arange(256, dtype=np.uint8), 1024),
        "periodic_after_noise_262144": np.concatenate([rng.integers(0, 256, 131072 - 1000, dtype=np.uint8),
                                                       np.tile(tile[:97], 1400)[:131072 + 1000]]),
    }


@in_every_write_order
def test_wide_frames_decode_with_libzstd_and_our_decoder(Z, libzstd, write_order):
    written = 0
    for name, src in _streams().items():
        n = src.size
        for cap in (n, n // 2, 2000):
            out = np.full(n + 4096, 0xEE, np.uint8)
            r = Z.zwemu_zstd_encode(_p(src), n, _p(out), cap)
            assert 0 <= r < n and r <= cap, (name, cap, r)
            assert (out[cap:] == 0xEE).all(), (name, cap)        # nothing past the budget
            if write_order:                                      # the frame is the one the ascending order writes
                set_order(Z, 0)
                out0 = np.full(n + 4096, 0xEE, np.uint8)
                r0 = Z.zwemu_zstd_encode(_p(src), n, _p(out0), cap)
                set_order(Z, write_order)
                assert r0 == r and np.array_equal(out0, out), (name, cap)
            if r == 0:
                continue
            written += 1
            frame = out[:r].copy()
            rr, dec = E.zstd_decode(frame, n + 8)
            assert rr == n and dec == src.tobytes(), (name, cap)
            if libzstd is not None:
                got = np.zeros(n, np.uint8)
                d = libzstd.ZSTD_decompress(_p(got), n, _p(frame), r)
                assert not libzstd.ZSTD_isError(d) and d == n and got.tobytes() == src.tobytes(), (name, cap)
    assert written >= 8


@pytest.mark.parametrize("dt", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("blk", [131072, 196608, 262144])
@pytest.mark.parametrize("clevel", [5, 9])
@in_every_write_order
def test_round_trip_table(Z, dt, blk, clevel):
    it = np.dtype(dt).itemsize
    arr = synth.natural_channel(dt, 1024, 1048576 // 1024 // it)
    raw = arr.view(np.uint8).ravel()
    rc, chunks = compress(Z, cparams(it, blk, clevel=clevel), [raw])
    assert rc == 0
    assert len(chunks[0]) < raw.size
    rc, st, out = decompress(Z, chunks)
    assert rc == 0 and st[0] == 0, st
    assert out[0] == raw.tobytes()


def _periodic_images():
    """images whose 256 KiB streams repeat from one row to the next: a zstd block of them is one match"""
    x = np.arange(1024)
    gradient_u8 = np.tile((x * 255 // 1023).astype(np.uint8), (1024, 1))
    rows_u16 = np.tile((x * 37 % 65536).astype(np.uint16), (512, 1))
    small_u16 = np.tile((x % 256).astype(np.uint16), (512, 1))         # 8-bit values in 16 bits: the high-byte plane is zero
    return [("gradient_u8", gradient_u8, 1), ("rows_u16_none", rows_u16, 0), ("small_u16", small_u16, 1)]


@pytest.mark.parametrize("clevel", [5, 9])
@in_every_write_order
def test_streams_that_are_one_match_per_zstd_block_round_trip(Z, clevel):
    for name, img, filt in _periodic_images():
        raw = np.ascontiguousarray(img).view(np.uint8).ravel()
        rc, chunks = compress(Z, cparams(img.dtype.itemsize, 262144, clevel=clevel, filt=filt), [raw])
        assert rc == 0, name
        assert len(chunks[0]) < raw.size // 8, name
        rc, st, out = decompress(Z, chunks)
        assert rc == 0 and st[0] == 0, (name, st)
        assert out[0] == raw.tobytes(), name


@in_every_write_order
def test_float32_clevel5_256k_is_written_by_the_normal_path_and_read_by_the_wide_one(Z):
    arr = synth.natural_channel(np.float32, 512, 512)
    raw = arr.view(np.uint8).ravel()
    rc, chunks = compress(Z, cparams(4, 262144, clevel=5), [raw])
    assert rc == 0 and Z.zwemu_last_route() == 0             # (byte planes of 64 KiB: the normal encoder)
    rc, st, out = decompress(Z, chunks)
    assert rc == 0 and st[0] == 0 and Z.zwemu_last_route() == 2
    assert out[0] == raw.tobytes()


@in_every_write_order
def test_a_mixed_batch_decodes_in_one_call(Z):
    small = synth.tiled_channel(np.float16, 512, 256).view(np.uint8).ravel()
    big = synth.natural_channel(np.uint16, 1024, 512).view(np.uint8).ravel()
    rc, c1 = compress(Z, cparams(2, 32768), [small])
    assert rc == 0
    rc, c2 = compress(Z, cparams(2, 262144), [big])
    assert rc == 0
    rc, c3 = compress(Z, cparams(2, 262144, compcode=LZ4), [big])
    assert rc == 0
    rc, st, out = decompress(Z, [c1[0], c2[0], c3[0], c2[0]])
    assert rc == 0 and list(st) == [0, 0, 0, 0]
    assert out == [small.tobytes(), big.tobytes(), big.tobytes(), big.tobytes()]


@pytest.fixture(scope="module")
def wkat(golden_dir):
    return np.load(os.path.join(golden_dir, "zstd_wide_kat.npz"))


@pytest.fixture(scope="module")
def golden_inputs(golden_dir, wkat):
    spec = importlib.util.spec_from_file_location("make_zstd_wide_golden", os.path.join(golden_dir, "make_zstd_wide_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs = gen.inputs()
    for name in wkat["chunks"]:
        assert hashlib.sha256(inputs[str(name)][0].tobytes()).hexdigest() == str(wkat["in_sha256|" + str(name)]), name
    return inputs


@in_every_write_order
def test_libzstd_chunks_decode(Z, wkat, golden_inputs):
    names = [str(n) for n in wkat["chunks"]]
    assert len(names) >= 20
    for name in names:
        chunk = wkat["chunk|" + name].tobytes()
        rc, st, out = decompress(Z, [chunk])
        assert rc == 0 and st[0] == 0, (name, st)
        assert out[0] == golden_inputs[name][0].tobytes(), name
    # all of them in one batch
    rc, st, out = decompress(Z, [wkat["chunk|" + n].tobytes() for n in names])
    assert rc == 0 and not st.any()
    assert all(o == golden_inputs[n][0].tobytes() for o, n in zip(out, names))


@in_every_write_order
def test_corrupt_frame_and_truncated_chunk(Z):
    raw = synth.natural_channel(np.uint8, 1024, 512).ravel()
    rc, chunks = compress(Z, cparams(1, 262144), [raw])
    assert rc == 0
    c = bytearray(chunks[0])
    bstart = int(np.frombuffer(bytes(c[32:36]), np.int32)[0])
    cs = int(np.frombuffer(bytes(c[bstart:bstart + 4]), np.int32)[0])
    assert 0 < cs < 262144 and bytes(c[bstart + 4:bstart + 8]) == b"\x28\xb5\x2f\xfd"
    for k in range(bstart + 4 + cs - 40, bstart + 4 + cs):
        c[k] = 0xFF                                            # the end of the first frame's sequence bit stream
    rc, st, _ = decompress(Z, [bytes(c)])
    assert rc == 0 and st[0] < 0
    c = bytearray(chunks[0])
    c[bstart + 4 + 5] ^= 0x40                                  # the content size of the first frame
    rc, st, _ = decompress(Z, [bytes(c)])
    assert rc == 0 and st[0] < 0
    rc, st, _ = decompress(Z, [chunks[0]], sizes=[len(chunks[0]) // 2])
    assert rc == 0 and st[0] < 0


def test_plan_memory_that_cannot_be_had_fails_the_chunk(Z):
    raw = synth.natural_channel(np.uint16, 1024, 256).view(np.uint8).ravel()
    rc, chunks = compress(Z, cparams(2, 262144), [raw])
    assert rc == 0
    Z.zwemu_set_plan_fail(1)
    try:
        rc, st, _ = decompress(Z, chunks)
    finally:
        Z.zwemu_set_plan_fail(0)
    assert rc == 0 and st[0] == -4


def test_blocks_above_256k_stay_refused(Z):
    raw = synth.natural_channel(np.uint8, 1024, 1024).ravel()
    for blk in (262145, 524288):
        rc, _ = compress(Z, cparams(1, blk), [raw])
        assert rc == ERR_CODEC_SUPPORT
    # bitshuffle on the wide write path stays refused, as for LZ4
    rc, _ = compress(Z, cparams(1, 262144, filt=2), [raw])
    assert rc == ERR_CODEC_SUPPORT
