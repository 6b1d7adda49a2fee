"""Strided and batched region writes of the `compressed_image` module on all four classes: set_region(..., step_x, step_y),
set_regions, set_pixels on Channel / Image / DeviceChannel / DeviceImage and __setitem__ on Channel / DeviceChannel (compressed/channel.h,
image.h over cimg_update_windows_strided_host; device_channel.h, device_image.h over cimg_update_windows_strided_device), against numpy
assignment on a copy of the pixels.  The host classes' tests are at the end of the file and run in this process.

The cases are in tests/_device_cases_strided_writes.py.  On the "mock" backend (the module linked against the emulator, with
tests/emu/mock_window_write_strided.cpp) device memory is host memory; with the `gpu` parameter every case runs on torch tensors on
the MI355X, in a child process that imports torch first."""
import os
import subprocess
import sys

import pytest

import _device_cases as D
import _device_cases_strided_writes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_mock = {}


def _run(backend, case):
    if backend == "mock":
        if not _mock:
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
            _mock["ci"] = D.load_module("mock")
        S.CASES[case](_mock["ci"], D.MockAdapter())
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_strided_writes.py"), case], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.param


def test_channel_set_region_with_steps(backend):
    _run(backend, "channel_set_region_steps")


def test_channel_set_regions_and_set_pixels(backend):
    _run(backend, "channel_set_regions_and_pixels")


def test_channel_setitem(backend):
    _run(backend, "channel_setitem")


def test_image_set_region_set_regions_set_pixels(backend):
    _run(backend, "image")


def test_errors_raise_before_anything_runs(backend):
    _run(backend, "errors")


# ---- the host classes: Channel / Image (channel<T> / image<T> over cimg_update_windows_strided_host), in this process -----------
import importlib.util  # noqa: E402
import sysconfig  # noqa: E402

import numpy as np  # noqa: E402

_mods = {}


def _load(which):
    if which not in _mods:
        if which == "mock":
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
        _mods[which] = D.load_module(which)
    return _mods[which]


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def ci(request):
    return _load(request.param)


W, H = 300, 90


def _kw(dtype):
    return dict(block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 13)


@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
def test_host_channel_set_region_steps_regions_pixels(ci, dtype):
    rng = np.random.default_rng(3)
    for codec in (ci.Codec.lz4, ci.Codec.blosclz, ci.Codec.zstd):
        kw = dict(compression_codec=codec, **_kw(dtype))
        want = D.pixels(dtype, W, H)
        ch = ci.Channel(want, W, H, **kw)
        for k, (x, y, w, h, sx, sy) in enumerate([(17, 4, 71, 60, 3, 2), (0, 0, 300, 90, 16, 16), (1, 1, 299, 1, 2, 1), (299, 0, 1, 90, 1, 7),
                                                  (0, 0, 300, 90, 299, 89), (3, 3, 1, 1, 4, 4), (5, 11, 290, 40, 7, 13)]):
            v = S.values(dtype, ((h + sy - 1) // sy, (w + sx - 1) // sx), 40 + k)
            ch.set_region(x, y, v, step_x=sx, step_y=sy)
            want[y:y + h:sy, x:x + w:sx] = v
            assert np.array_equal(ch.get_decompressed(), want), (codec, x, y, w, h, sx, sy)
            assert np.array_equal(ch.get_region(x, y, w, h, step_x=sx, step_y=sy), v)
        for (w, h, sx, sy, n) in [(32, 16, 1, 1, 9), (40, 30, 4, 3, 6)]:
            xs, ys = rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)
            xs[-1], ys[-1] = xs[0], ys[0]                       # the last region lies on the first: it wins
            v = S.values(dtype, (n, (h + sy - 1) // sy, (w + sx - 1) // sx), n)
            ch.set_regions(xs, ys, v, step_x=sx, step_y=sy)
            for k in range(n):
                want[ys[k]:ys[k] + h:sy, xs[k]:xs[k] + w:sx] = v[k]
            assert np.array_equal(ch.get_decompressed(), want), (codec, w, h, sx, sy)
        n = 300
        xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
        xs[-20:], ys[-20:] = xs[:20], ys[:20]                   # duplicated pixels: the last value wins
        v = S.values(dtype, (n,), 5)
        ch.set_pixels(xs, ys, v)
        for k in range(n):
            want[ys[k], xs[k]] = v[k]
        assert np.array_equal(ch.get_decompressed(), want)
        before = ch.compressed_bytes()
        ch.set_regions([], [], np.zeros((0, 4, 4), dtype))
        ch.set_pixels([], [], np.zeros(0, dtype))
        assert ch.compressed_bytes() == before
        if codec != ci.Codec.zstd:                              # the chunks of a channel built from the edited pixels
            assert before == ci.Channel(want, W, H, **kw).compressed_bytes(), codec


def test_host_channel_setitem(ci):
    for dtype in (np.uint16, np.float32):
        want = D.pixels(dtype, W, H)
        ch = ci.Channel(want, W, H, **_kw(dtype))
        for k, key in enumerate(S.KEYS):
            shape = want[key].shape
            full = S.values(dtype, shape, 70 + k)
            row = S.values(dtype, shape[-1:], 90 + k) if len(shape) else full
            for v in (full, 7, 3.0, row, row.tolist(), np.float64(5).astype(dtype)):
                ch[key] = v
                want[key] = v
                assert (ch[key] == np.broadcast_to(np.asarray(v, dtype), shape)).all(), (key, type(v))
                assert np.array_equal(ch.get_decompressed(), want), (key, type(v))
        assert ch.compressed_bytes() == ci.Channel(want, W, H, **_kw(dtype)).compressed_bytes()


def test_host_lazy_channels(ci):
    w, h = 257, 40
    full = ci.Channel.full(np.float32, 2.5, w, h, chunk_size=w * 4 * 3)
    want = np.full((h, w), 2.5, np.float32)
    v = S.values(np.float32, (7, 34), 1)
    full.set_region(3, 4, v, step_x=3, step_y=3)            # rows 4, 7, .. 22: the chunks that hold one become real
    want[4:23:3, 3:103:3] = v
    assert np.array_equal(full.get_decompressed(), want)
    full[5::4, ::50] = 9                                     # real and lazy chunks in one call
    want[5::4, ::50] = 9
    assert np.array_equal(full.get_decompressed(), want)
    xs, ys = np.array([0, 250, 0]), np.array([0, 39, 0])
    v = S.values(np.float32, (3,), 2)
    full.set_pixels(xs, ys, v)                               # the same lazy chunk twice: region order
    want[0, 0], want[39, 250] = v[2], v[1]
    assert np.array_equal(full.get_decompressed(), want)
    # partly lazy: one chunk compressed, its neighbours a fill value; the regions span all three
    mixed = ci.Channel.full(np.uint16, 7, w, h, chunk_size=w * 2 * 4)
    mixed.set_chunk(1, np.arange(mixed.chunk_elems(1), dtype=np.uint16))
    m = mixed.get_decompressed()
    q = S.values(np.uint16, (2, 5, 25), 5)
    mixed.set_regions([100, 110], [2, 3], q, step_x=2, step_y=2)
    for k, (x, y) in enumerate([(100, 2), (110, 3)]):
        m[y:y + 9:2, x:x + 49:2] = q[k]
    assert np.array_equal(mixed.get_decompressed(), m)


def test_host_image(ci):
    C = 3
    for dtype in (np.uint8, np.float32):
        planes = np.stack([D.pixels(dtype, W, H, seed=c) for c in range(C)])
        img = ci.Image(dtype, list(planes), W, H, ["r", "g", "b"], **_kw(dtype))
        want = planes.copy()
        v = S.values(dtype, (C, 15, 18), 1)
        img.set_region(10, 7, list(v), step_x=4, step_y=3)
        want[:, 7:7 + 43:3, 10:10 + 69:4] = v
        assert np.array_equal(np.stack(img.get_decompressed()), want)
        xs, ys = np.array([0, 100, 250, 100]), np.array([0, 40, 60, 40])
        v = S.values(dtype, (4, C, 10, 12), 2)
        img.set_regions(xs, ys, v, step_x=2, step_y=3)
        for k in range(4):
            want[:, ys[k]:ys[k] + 28:3, xs[k]:xs[k] + 23:2] = v[k]
        assert np.array_equal(np.stack(img.get_decompressed()), want)
        assert np.array_equal(img.get_regions(xs[:3], ys[:3], 23, 28, step_x=2, step_y=3), v[[0, 3, 2]])
        xs, ys = np.array([5, 6, 299, 5]), np.array([5, 5, 89, 5])
        v = S.values(dtype, (4, C), 3)
        img.set_pixels(xs, ys, v)
        for k in range(4):
            want[:, ys[k], xs[k]] = v[k]
        assert np.array_equal(np.stack(img.get_decompressed()), want)
        img.set_regions([], [], np.zeros((0, C, 2, 2), dtype))
        for c in range(C):
            assert img.channel(c).compressed_bytes() == ci.Channel(want[c], W, H, **_kw(dtype)).compressed_bytes()
        assert not hasattr(img, "__setitem__")
        assert img[0] is not None                            # __getitem__ stays the channel lookup


def test_host_errors(ci):
    dtype = np.float32
    arr = D.pixels(dtype, W, H)
    ch = ci.Channel(arr, W, H, **_kw(dtype))
    img = ci.Image(dtype, [arr, arr], W, H, **_kw(dtype))
    v = S.values(dtype, (10, 10), 0)
    vs = S.values(dtype, (3, 4, 4), 0)
    R = D.raises
    R(ValueError, ch.set_region, 0, 0, v, step_x=0)
    R(ValueError, ch.set_region, 0, 0, v, step_y=-1)
    R(IndexError, ch.set_region, 0, 0, v, step_x=40)
    R(IndexError, ch.set_region, 295, 0, v)
    R(IndexError, ch.set_region, 0, 0, v, step_y=10)
    R(ValueError, ch.set_region, 0, 0, v.astype(np.uint8), step_x=2)
    R(IndexError, img.set_region, 0, 0, [v, v], step_x=40)
    R(ValueError, img.set_region, 0, 0, [v], step_x=2)
    R(ValueError, img.set_region, 0, 0, [v, v], step_x=0)
    R(ValueError, ch.set_regions, [0, 1], [0, 1], vs)
    R(ValueError, ch.set_regions, [0.5, 1, 2], [0, 1, 2], vs)
    R(IndexError, ch.set_regions, [0, 1, 298], [0, 1, 2], vs)        # one bad region: nothing runs
    R(IndexError, ch.set_regions, [0, -1, 2], [0, 1, 2], vs)
    R(ValueError, ch.set_regions, [0, 1, 2], [0, 1, 2], vs, step_x=0)
    R(ValueError, ch.set_regions, [0, 1, 2], [0, 1, 2], vs[:, 0])
    R(ValueError, ch.set_regions, [0, 1, 2], [0, 1, 2], vs.astype(np.float64))
    R(ValueError, ch.set_pixels, [0, 1], [0, 1], vs[:2, 0, :1])
    R(IndexError, ch.set_pixels, [0, 300], [0, 1], vs[0, 0, :2])
    R(ValueError, img.set_regions, [0, 1, 2], [0, 1, 2], vs)
    R(ValueError, img.set_regions, [0, 1, 2], [0, 1, 2], np.zeros((3, 3, 4, 4), dtype))     # three channels for two
    R(IndexError, img.set_pixels, [0, 300], [0, 1], np.zeros((2, 2), dtype))
    for key, exc in [(np.s_[::-1], ValueError), (np.s_[90], IndexError), (np.s_[0, 0, 0], IndexError), (None, TypeError), (np.s_[..., 0], TypeError),
                     ([1, 2], TypeError)]:
        R(exc, ch.__getitem__, key)
        R(exc, ch.__setitem__, key, v)
    R(ValueError, ch.__setitem__, np.s_[0:10, 0:11], v)                  # not broadcastable
    R(ValueError, ch.__setitem__, np.s_[0:10, 0:10], v.astype(np.float16))   # an array of another dtype
    ch[10:10, :] = 5                                                       # an empty selection: nothing happens
    assert np.array_equal(ch.get_decompressed(), arr), "a refused call changed the channel"
    assert np.array_equal(np.stack(img.get_decompressed()), np.stack([arr, arr]))
