"""Channel.set_region / Image.set_region of the `compressed_image` module (host mirror: channel<T>::set_region, image<T>::set_region over
cimg_update_windows_host), on the "mock" backend (the module linked against the emulator, tests/emu/mock_window_write.cpp) and on the
MI355X.  After every write the channel must decode to the numpy-edited array and hold exactly the bytes of a channel built from that
array with the same parameters."""
import importlib.util
import os
import subprocess
import sysconfig

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = sysconfig.get_config_var("EXT_SUFFIX")
_cache = {}


def _load(backend):
    if backend not in _cache:
        if backend == "mock":
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
            path = os.path.join(ROOT, "tests", "emu", "compressed_image" + EXT)
        else:
            path = os.path.join(ROOT, "compressed-image_amd", "compressed_image" + EXT)
            assert os.path.exists(path), "product module missing: run __graft_entry__.build()"
        spec = importlib.util.spec_from_file_location("compressed_image", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache[backend] = mod
    return _cache[backend]


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def ci(request):
    return _load(request.param)


def pixels(dtype, width, height, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    a = ((x // 7) * 3 + (y // 5) * 11 + rng.integers(0, 3, (height, width))) % 200
    return a.astype(dtype)


def patch(dtype, h, w, seed):
    return np.random.default_rng(seed).integers(0, 250, (h, w)).astype(dtype)


# 1 x 1, a single row, a single column, a full-width band, one across chunk boundaries, the whole channel, width / height 0
REGIONS = [(5, 3, 1, 1), (0, 20, 300, 1), (299, 0, 1, 90), (0, 13, 300, 13), (17, 4, 71, 60), (290, 89, 10, 1), (0, 0, 300, 90),
           (10, 10, 0, 5), (10, 10, 5, 0)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32])
def test_channel_set_region(ci, dtype):
    W, H = 300, 90
    it = np.dtype(dtype).itemsize
    for codec in (ci.Codec.lz4, ci.Codec.blosclz, ci.Codec.zstd):
        kw = dict(compression_codec=codec, block_size=4096, chunk_size=W * it * 13)
        want = pixels(dtype, W, H)
        ch = ci.Channel(want, W, H, **kw)
        for k, (x, y, w, h) in enumerate(REGIONS):
            p = patch(dtype, h, w, k)
            ch.set_region(x, y, p)
            want[y:y + h, x:x + w] = p
            assert np.array_equal(ch.get_decompressed(), want), (codec, x, y, w, h)
            assert ch.compressed_bytes() == ci.Channel(want, W, H, **kw).compressed_bytes(), (codec, x, y, w, h)
        assert np.array_equal(ch.get_region(17, 4, 71, 60), want[4:64, 17:88])


def test_strided_source(ci):
    W, H = 257, 40
    want = pixels(np.float32, W, H)
    ch = ci.Channel(want, W, H, block_size=4096, chunk_size=W * 4 * 6)
    big = patch(np.float32, 60, 90, 3)
    src = big[::2, ::3]                                   # (30, 30), not contiguous
    ch.set_region(100, 5, src)
    want[5:35, 100:130] = src
    assert np.array_equal(ch.get_decompressed(), want)
    assert ch.compressed_bytes() == ci.Channel(want, W, H, block_size=4096, chunk_size=W * 4 * 6).compressed_bytes()


def test_same_state_as_set_chunk(ci):
    W, H = 256, 64
    kw = dict(block_size=4096, chunk_size=W * 2 * 16)
    base = pixels(np.uint16, W, H)
    a, b = ci.Channel(base, W, H, **kw), ci.Channel(base, W, H, **kw)
    p = patch(np.uint16, 8, 40, 7)
    a.set_region(30, 18, p)                                # rows 18 .. 25: all inside chunk 1
    c = b.get_chunk(1).reshape(16, W)
    c[2:10, 30:70] = p
    b.set_chunk(1, c.ravel())
    assert np.array_equal(a.get_decompressed(), b.get_decompressed())
    assert a.compressed_bytes() == b.compressed_bytes()
    for i in range(a.num_chunks()):
        assert np.array_equal(a.get_chunk(i), b.get_chunk(i))


def test_lazy_channels(ci):
    W, H = 257, 40
    full = ci.Channel.full(np.float32, 2.5, W, H, chunk_size=W * 4 * 3)
    want = np.full((H, W), 2.5, np.float32)
    p = patch(np.float32, 20, 100, 1)
    full.set_region(3, 4, p)                               # rows 4 .. 23: chunks 1 .. 7 become real, the others stay lazy
    want[4:24, 3:103] = p
    assert np.array_equal(full.get_decompressed(), want)
    assert np.array_equal(full.get_region(0, 0, W, 6), want[:6])
    full.set_region(0, 5, patch(np.float32, 1, W, 2))      # a real chunk written again
    want[5] = patch(np.float32, 1, W, 2)[0]
    assert np.array_equal(full.get_decompressed(), want)
    zeros = ci.Channel.zeros(np.uint16, W, H)
    z = np.zeros((H, W), np.uint16)
    zeros.set_region(250, 39, patch(np.uint16, 1, 7, 4))
    z[39, 250:] = patch(np.uint16, 1, 7, 4)[0]
    assert np.array_equal(zeros.get_decompressed(), z)
    # partly lazy: one chunk compressed, its neighbours a fill value; the window spans all three
    mixed = ci.Channel.full(np.uint16, 7, W, H, chunk_size=W * 2 * 4)
    mixed.set_chunk(1, np.arange(mixed.chunk_elems(1), dtype=np.uint16))
    m = mixed.get_decompressed()
    q = patch(np.uint16, 9, 50, 5)
    mixed.set_region(100, 2, q)
    m[2:11, 100:150] = q
    assert np.array_equal(mixed.get_decompressed(), m)


def test_image_set_region(ci):
    W, H = 200, 64
    kw = dict(block_size=4096, chunk_size=W * 2 * 9)
    planes = [pixels(np.uint16, W, H, seed=s) for s in range(4)]
    img = ci.Image(np.uint16, planes, W, H, ["r", "g", "b", "a"], **kw)
    ps = [patch(np.uint16, 40, 150, 10 + s) for s in range(4)]
    img.set_region(13, 7, ps)
    for p, q in zip(planes, ps):
        p[7:47, 13:163] = q
    dec = img.get_decompressed()
    assert all(np.array_equal(d, p) for d, p in zip(dec, planes))
    for k, p in enumerate(planes):
        assert img.channel(k).compressed_bytes() == ci.Channel(p, W, H, **kw).compressed_bytes()


def test_errors(ci):
    W, H = 64, 32
    ch = ci.Channel(pixels(np.uint8, W, H), W, H)
    img = ci.Image(np.uint8, [pixels(np.uint8, W, H)] * 2, W, H)
    before = ch.get_decompressed()
    for (x, y, w, h) in [(0, 0, W + 1, 1), (W, 0, 1, 1), (0, H, 1, 1), (10, 10, 60, 1), (0, 20, 1, 13)]:
        with pytest.raises(IndexError):
            ch.set_region(x, y, np.zeros((h, w), np.uint8))
        with pytest.raises(IndexError):
            img.set_region(x, y, [np.zeros((h, w), np.uint8)] * 2)
    for bad in [lambda: ch.set_region(-1, 0, np.zeros((1, 1), np.uint8)),
                lambda: ch.set_region(0, 0, np.zeros((1, 1), np.uint16)),            # wrong dtype
                lambda: ch.set_region(0, 0, np.zeros(4, np.uint8)),                  # not (height, width)
                lambda: img.set_region(0, 0, [np.zeros((2, 2), np.uint8)]),          # one array for two channels
                lambda: img.set_region(0, 0, [np.zeros((2, 2), np.uint8), np.zeros((2, 3), np.uint8)])]:
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(ch.get_decompressed(), before)
    ch.set_region(W - 1, H - 1, np.full((1, 1), 9, np.uint8))
    before[H - 1, W - 1] = 9
    assert np.array_equal(ch.get_decompressed(), before)
