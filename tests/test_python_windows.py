"""Channel.get_region / Image.get_region of the `compressed_image` module (host mirror: channel<T>::get_region, image<T>::get_region
over cimg_decompress_windows_host), on the "mock" backend (the module linked against the emulator, tests/emu/mock_window.cpp) and
on the MI355X.  Results are compared with slices of get_decompressed() and of the source pixels."""
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


REGIONS = [(0, 0, 1, 1), (5, 3, 1, 1), (0, 0, 300, 1), (0, 0, 300, 90), (290, 89, 10, 1), (17, 4, 71, 60), (299, 0, 1, 90),
           (3, 30, 200, 7), (10, 10, 0, 5), (10, 10, 5, 0)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32, np.int32])
def test_channel_region(ci, dtype):
    W, H = 300, 90
    arr = pixels(dtype, W, H)
    it = np.dtype(dtype).itemsize
    for codec in (ci.Codec.lz4, ci.Codec.blosclz, ci.Codec.zstd):
        ch = ci.Channel(arr, W, H, compression_codec=codec, block_size=4096, chunk_size=W * it * 13)
        for (x, y, w, h) in REGIONS:
            r = ch.get_region(x, y, w, h)
            assert r.shape == (h, w) and r.dtype == np.dtype(dtype)
            assert np.array_equal(r, arr[y:y + h, x:x + w]), (codec, x, y, w, h)


def test_lazy_channels(ci):
    W, H = 257, 40
    full = ci.Channel.full(np.float32, 2.5, W, H, chunk_size=W * 4 * 3)
    assert np.array_equal(full.get_region(3, 4, 100, 20), np.full((20, 100), 2.5, np.float32))
    zeros = ci.Channel.zeros(np.uint16, W, H)
    assert np.array_equal(zeros.get_region(250, 39, 7, 1), np.zeros((1, 7), np.uint16))
    # partly lazy: one chunk rewritten, its neighbours still a fill value
    mixed = ci.Channel.full(np.uint16, 7, W, H, chunk_size=W * 2 * 4)
    c1 = np.arange(mixed.chunk_elems(1), dtype=np.uint16)
    mixed.set_chunk(1, c1)
    want = mixed.get_decompressed()
    assert np.array_equal(want.ravel()[W * 4:W * 8], c1)
    for (x, y, w, h) in [(0, 2, W, 9), (100, 3, 50, 3), (5, 7, 1, 1), (250, 0, 7, 40)]:
        assert np.array_equal(mixed.get_region(x, y, w, h), want[y:y + h, x:x + w])


def test_image_region(ci):
    W, H = 200, 64
    planes = [pixels(np.uint16, W, H, seed=s) for s in range(4)]
    img = ci.Image(np.uint16, planes, W, H, ["r", "g", "b", "a"], block_size=4096, chunk_size=W * 2 * 9)
    out = img.get_region(13, 7, 150, 40)
    assert isinstance(out, list) and len(out) == 4
    for o, p in zip(out, planes):
        assert np.array_equal(o, p[7:47, 13:163])
    dec = img.get_decompressed()
    assert all(np.array_equal(o, d[7:47, 13:163]) for o, d in zip(out, dec))


def test_out_of_bounds(ci):
    W, H = 64, 32
    ch = ci.Channel(pixels(np.uint8, W, H), W, H)
    img = ci.Image(np.uint8, [pixels(np.uint8, W, H)], W, H)
    for bad in [(0, 0, W + 1, 1), (W, 0, 1, 1), (0, H, 1, 1), (10, 10, 60, 1), (0, 20, 1, 13), (-1, 0, 1, 1), (0, 0, -1, 1)]:
        with pytest.raises((IndexError, ValueError)):
            ch.get_region(*bad)
        with pytest.raises((IndexError, ValueError)):
            img.get_region(*bad)
    assert ch.get_region(W - 1, H - 1, 1, 1).shape == (1, 1)
