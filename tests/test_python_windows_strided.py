"""get_region(..., step_x, step_y) of Channel, Image, DeviceChannel and DeviceImage and numpy-style keys on Channel and DeviceChannel
(`compressed_image` module over cimg_decompress_windows_strided_host / _device), on the "mock" backend (the module linked against
the emulator, tests/emu/mock_window_strided.cpp) and on the MI355X.  Results are compared with numpy slices of get_decompressed()
and of the source pixels.  The device classes' cases are in tests/_device_cases_strided.py; with the `gpu` parameter they run on
torch tensors in a child process that imports torch first, like tests/test_python_device.py's."""
import importlib.util
import os
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import _device_cases as D
import _device_cases_strided as S
from _device_cases_strided import BAD_KEYS, KEYS, STEPPED, stepped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = sysconfig.get_config_var("EXT_SUFFIX")
W, H = S.W, S.H
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
def backend(request):
    return request.param


@pytest.fixture
def ci(backend):
    return _load(backend)


pixels = D.pixels


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32])
def test_channel_steps(ci, dtype):
    arr = pixels(dtype, W, H)
    it = np.dtype(dtype).itemsize
    for codec in (ci.Codec.lz4, ci.Codec.blosclz, ci.Codec.zstd):
        ch = ci.Channel(arr, W, H, compression_codec=codec, block_size=4096, chunk_size=W * it * 13)
        want = ch.get_decompressed()
        assert np.array_equal(want, arr)
        for (x, y, w, h, sx, sy) in STEPPED:
            r = ch.get_region(x, y, w, h, step_x=sx, step_y=sy)
            exp = stepped(want, x, y, w, h, sx, sy)
            assert r.shape == exp.shape and r.dtype == np.dtype(dtype), (r.shape, exp.shape)
            assert np.array_equal(r, exp), (codec, x, y, w, h, sx, sy)
        assert np.array_equal(ch.get_region(5, 3, 200, 80, 16, 8), want[3:83:8, 5:205:16])            # positional steps
        assert np.array_equal(ch.get_region(5, 3, 200, 80), want[3:83, 5:205])                        # the defaults are the old call


def test_blocks_smaller_than_the_step(ci):
    """col_pitch * typesize >= blocksize: most blocks of a sampled row hold no sample"""
    Wb, Hb = 8192, 24
    arr = pixels(np.uint16, Wb, Hb)
    ch = ci.Channel(arr, Wb, Hb, block_size=4096, chunk_size=Wb * 2 * 5)
    for sx, sy in ((2048, 1), (4096, 5), (3000, 7), (8191, 23)):
        assert np.array_equal(ch.get_region(0, 0, Wb, Hb, step_x=sx, step_y=sy), arr[::sy, ::sx]), (sx, sy)
    assert np.array_equal(ch[3::4, 100::2500], arr[3::4, 100::2500])


def test_lazy_channels(ci):
    Wl, Hl = 257, 40
    full = ci.Channel.full(np.float32, 2.5, Wl, Hl, chunk_size=Wl * 4 * 3)
    assert np.array_equal(full.get_region(3, 4, 100, 20, step_x=3, step_y=4), np.full((5, 34), 2.5, np.float32))
    zeros = ci.Channel.zeros(np.uint16, Wl, Hl)
    assert np.array_equal(zeros.get_region(0, 0, Wl, Hl, step_x=16, step_y=16), np.zeros((3, 17), np.uint16))
    assert np.array_equal(zeros[::9, 1::50], np.zeros((5, 6), np.uint16))
    # partly lazy: chunks rewritten, their neighbours still a fill value; runs of real chunks between lazy ones
    mixed = ci.Channel.full(np.uint16, 7, Wl, Hl, chunk_size=Wl * 2 * 4)
    for k in (1, 2, 5, 9):
        mixed.set_chunk(k, (np.arange(mixed.chunk_elems(k)) * (k + 1) % 65521).astype(np.uint16))
    want = mixed.get_decompressed()
    for (x, y, w, h, sx, sy) in [(0, 0, Wl, Hl, 2, 2), (0, 0, Wl, Hl, 1, 3), (0, 0, Wl, Hl, 5, 1), (0, 2, Wl, 37, 100, 3), (100, 3, 50, 30, 7, 5),
                                 (5, 7, 1, 1, 4, 4), (250, 0, 7, 40, 3, 11), (0, 0, Wl, Hl, 256, 4), (1, 3, 255, 36, 254, 7)]:
        assert np.array_equal(mixed.get_region(x, y, w, h, step_x=sx, step_y=sy), want[y:y + h:sy, x:x + w:sx]), (x, y, w, h, sx, sy)
    for key in (slice(None, None, 3), (slice(2, None, 5), slice(None, None, 9)), 17, (slice(None), 100), (slice(6, 30, 4), slice(3, 250, 61))):
        assert np.array_equal(mixed[key], want[key]), key


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32])
def test_image_steps(ci, dtype):
    planes = [pixels(dtype, W, H, seed=s) for s in range(4)]
    img = ci.Image(dtype, planes, W, H, ["r", "g", "b", "a"], block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 9)
    dec = img.get_decompressed()
    for (x, y, w, h, sx, sy) in STEPPED:
        out = img.get_region(x, y, w, h, step_x=sx, step_y=sy)
        assert isinstance(out, list) and len(out) == 4
        for o, d, p in zip(out, dec, planes):
            assert o.shape == stepped(d, x, y, w, h, sx, sy).shape
            assert np.array_equal(o, stepped(d, x, y, w, h, sx, sy)) and np.array_equal(o, stepped(p, x, y, w, h, sx, sy))
    assert isinstance(img["g"], ci.Channel) and isinstance(img[1], ci.Channel)        # Image.__getitem__ stays the channel lookup
    assert np.array_equal(img["g"][::4, ::6], dec[1][::4, ::6])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_channel_getitem(ci, dtype):
    arr = pixels(dtype, W, H)
    ch = ci.Channel(arr, W, H, block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 13)
    want = ch.get_decompressed()
    for key in KEYS:
        r, exp = ch[key], want[key]
        assert isinstance(r, np.ndarray) and r.shape == exp.shape and r.dtype == exp.dtype, (key, r.shape, exp.shape)
        assert np.array_equal(r, exp), key
    for key, exc in BAD_KEYS:
        with pytest.raises(exc):
            ch[key]


def test_bad_steps_and_bounds(ci):
    ch = ci.Channel(pixels(np.uint8, 64, 32), 64, 32)
    img = ci.Image(np.uint8, [pixels(np.uint8, 64, 32)], 64, 32)
    for o in (ch, img):
        for bad in (dict(step_x=0), dict(step_y=0), dict(step_x=-1), dict(step_x=2, step_y=-3)):
            with pytest.raises(ValueError):
                o.get_region(0, 0, 10, 10, **bad)
        for bad in [(0, 0, 65, 1), (64, 0, 1, 1), (0, 32, 1, 1), (10, 10, 60, 1), (0, 20, 1, 13), (-1, 0, 1, 1), (0, 0, -1, 1)]:
            with pytest.raises((IndexError, ValueError)):
                o.get_region(*bad, step_x=2, step_y=2)
    assert ch.get_region(63, 31, 1, 1, step_x=5, step_y=5).shape == (1, 1)


def _run(backend, case):
    if backend == "mock":
        S.CASES[case](_load("mock"), D.MockAdapter())
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_strided.py"), case], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_channel_steps(backend):
    _run(backend, "channel_steps")


def test_device_channel_getitem(backend):
    _run(backend, "channel_getitem")


def test_device_image_steps(backend):
    _run(backend, "image_steps")
