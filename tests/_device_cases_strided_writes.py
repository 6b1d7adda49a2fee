"""The cases of tests/test_python_window_writes_strided.py: DeviceChannel / DeviceImage set_region with steps, set_regions, set_pixels
and DeviceChannel.__setitem__ of the `compressed_image` module, against numpy assignment on a copy of the pixels.

Every case takes the module `ci` and an adapter `A` (tests/_device_cases.py: numpy memory behind __cuda_array_interface__ on the
mock backend, torch tensors on the GPU).  Run as a script -- `python _device_cases_strided_writes.py CASE` -- the file imports torch
FIRST, loads the product module and runs CASE on torch tensors, in a process of its own."""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

from _device_cases import H, ROOT, W, HostCuda, MockAdapter, TorchAdapter, codecs, kw, load_module, pixels, raises  # noqa: F401

DTYPES = [np.uint8, np.float16, np.float32]
# the keys tests/test_python_windows_strided.py reads with __getitem__
KEYS = [np.s_[::16, ::16], np.s_[3::7, 5::3], np.s_[10:50:4, 20:200:9], np.s_[::1, ::1], np.s_[5], np.s_[-1], np.s_[2:40:5], np.s_[:, 7],
        np.s_[4, 9], np.s_[::89, ::299], np.s_[::200, ::400], np.s_[10:10, :], np.s_[:, 5:5:3], np.s_[-30:-2:3, -100::11], np.s_[7, ::2]]


def values(dtype, shape, seed):
    return np.random.default_rng(seed).integers(0, 250, shape).astype(dtype)


def case_channel_set_region_steps(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        for codec in codecs(ci):
            ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=codec, **kw(dtype))
            edited = arr.copy()
            for k, (x, y, w, h, sx, sy) in enumerate([(17, 4, 71, 60, 3, 2), (0, 0, 300, 90, 16, 16), (1, 1, 299, 1, 2, 1), (299, 0, 1, 90, 1, 7),
                                                      (0, 0, 300, 90, 299, 89), (5, 5, 40, 30, 1, 1), (3, 3, 1, 1, 4, 4)]):
                v = values(dtype, ((h + sy - 1) // sy, (w + sx - 1) // sx), 40 + k)
                ch.set_region(x, y, A.dev(v), step_x=sx, step_y=sy)
                edited[y:y + h:sy, x:x + w:sx] = v
                assert np.array_equal(A.host(ch.get_decompressed()), edited), (dtype, codec, x, y, w, h, sx, sy)
                assert np.array_equal(A.host(ch.get_region(x, y, w, h, step_x=sx, step_y=sy)), v)
            assert ch.device_bytes() == sum((ch.compressed_bytes(i) + 63) // 64 * 64 for i in range(ch.num_chunks()))
            if codec != ci.Codec.zstd:                     # the chunks are those of a channel built from the edited pixels
                want = ci.Channel(edited, W, H, compression_codec=codec, **kw(dtype))
                assert ch.to_channel().compressed_bytes() == want.compressed_bytes() == ch.compressed_bytes(), (dtype, codec)


def case_channel_set_regions_and_pixels(ci, A):
    rng = np.random.default_rng(11)
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        edited = arr.copy()
        for (w, h, sx, sy, n) in [(32, 16, 1, 1, 9), (40, 30, 4, 3, 6), (1, 1, 1, 1, 50)]:
            xs, ys = rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)
            xs[-1], ys[-1] = xs[0], ys[0]                   # the last region lies on the first: it wins
            v = values(dtype, (n, (h + sy - 1) // sy, (w + sx - 1) // sx), n)
            ch.set_regions(xs, ys, A.dev(v), step_x=sx, step_y=sy)
            for k in range(n):
                edited[ys[k]:ys[k] + h:sy, xs[k]:xs[k] + w:sx] = v[k]
            assert np.array_equal(A.host(ch.get_decompressed()), edited), (dtype, w, h, sx, sy)
        n = 300
        xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
        xs[-20:], ys[-20:] = xs[:20], ys[:20]               # duplicated pixels: the last value wins
        v = values(dtype, (n,), 5)
        ch.set_pixels(xs, ys, A.dev(v))
        for k in range(n):
            edited[ys[k], xs[k]] = v[k]
        assert np.array_equal(A.host(ch.get_decompressed()), edited), dtype
        assert np.array_equal(A.host(ch.get_pixels(xs, ys)), edited[ys, xs])
        before = ch.compressed_bytes()
        ch.set_regions([], [], A.dev(np.zeros((0, 4, 4), dtype)))                       # N = 0: nothing happens
        ch.set_pixels(np.zeros(0, np.int64), np.zeros(0, np.int64), A.dev(np.zeros(0, dtype)))
        assert ch.compressed_bytes() == before and np.array_equal(A.host(ch.get_decompressed()), edited)


def dev(A, v):
    """A.dev for any shape: an integer key on both axes selects a 0-d array, which numpy.ascontiguousarray would make 1-d"""
    if v.ndim:
        return A.dev(v)
    return HostCuda(v.copy()) if A.name == "mock" else A.dev(v.reshape(1)).reshape(())


def case_channel_setitem(ci, A):
    for dtype in (np.uint16, np.float32):
        arr = pixels(dtype, W, H)
        ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        edited = arr.copy()
        for k, key in enumerate(KEYS):
            v = values(dtype, edited[key].shape, 70 + k)
            ch[key] = dev(A, v)
            edited[key] = v
            assert np.array_equal(A.host(ch[key]), v), key
            assert np.array_equal(A.host(ch.get_decompressed()), edited), key


def case_image(ci, A):
    C = 3
    for dtype in (np.uint8, np.float32):
        planes = np.stack([pixels(dtype, W, H, seed=c) for c in range(C)])
        img = ci.DeviceImage(dtype, [A.dev(p) for p in planes], W, H, **kw(dtype))
        edited = planes.copy()
        v = values(dtype, (C, 15, 18), 1)
        img.set_region(10, 7, A.dev(v), step_x=4, step_y=3)
        edited[:, 7:7 + 43:3, 10:10 + 69:4] = v
        assert np.array_equal(A.host(img.get_decompressed()), edited)
        assert np.array_equal(A.host(img.get_region(10, 7, 69, 43, step_x=4, step_y=3)), v)
        xs, ys = np.array([0, 100, 250, 100]), np.array([0, 40, 60, 40])
        v = values(dtype, (4, C, 10, 12), 2)
        img.set_regions(xs, ys, A.dev(v), step_x=2, step_y=3)
        for k in range(4):
            edited[:, ys[k]:ys[k] + 28:3, xs[k]:xs[k] + 23:2] = v[k]
        assert np.array_equal(A.host(img.get_decompressed()), edited)
        assert np.array_equal(A.host(img.get_regions(xs[:3], ys[:3], 23, 28, step_x=2, step_y=3)), v[[0, 3, 2]])
        xs, ys = np.array([5, 6, 299, 5]), np.array([5, 5, 89, 5])
        v = values(dtype, (4, C), 3)
        img.set_pixels(xs, ys, A.dev(v))
        for k in range(4):
            edited[:, ys[k], xs[k]] = v[k]
        assert np.array_equal(A.host(img.get_decompressed()), edited)
        img.set_regions([], [], A.dev(np.zeros((0, C, 2, 2), dtype)))
        assert np.array_equal(A.host(img.get_decompressed()), edited)
        raises((AttributeError, TypeError), lambda: img.__setitem__(0, 1))                   # Image gets no __setitem__


def case_errors(ci, A):
    dtype = np.float32
    arr = pixels(dtype, W, H)
    ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
    v = A.dev(values(dtype, (10, 10), 0))
    raises(ValueError, ch.set_region, 0, 0, v, step_x=0)
    raises(ValueError, ch.set_region, 0, 0, v, step_y=-1)
    raises(IndexError, ch.set_region, 0, 0, v, step_x=40)                  # covers (9 * 40 + 1) columns
    raises(IndexError, ch.set_region, 295, 0, v)
    raises(IndexError, ch.set_region, 0, 0, v, step_y=10)                  # 91 rows
    raises(ValueError, ch.set_region, 0, 0, A.dev(values(np.uint8, (4, 4), 0)), step_x=2)
    raises(TypeError, ch.set_region, 0, 0, values(dtype, (4, 4), 0), step_x=2)          # host memory
    vs = A.dev(values(dtype, (3, 4, 4), 0))
    raises(ValueError, ch.set_regions, [0, 1], [0, 1], vs)                  # 3 arrays, 2 coordinates
    raises(ValueError, ch.set_regions, [0, 1, 2], [0, 1], vs)
    raises(ValueError, ch.set_regions, [0.5, 1, 2], [0, 1, 2], vs)
    raises(IndexError, ch.set_regions, [0, 1, 298], [0, 1, 2], vs)          # one bad region: nothing runs
    raises(IndexError, ch.set_regions, [0, -1, 2], [0, 1, 2], vs)
    raises(ValueError, ch.set_regions, [0, 1, 2], [0, 1, 2], vs, step_x=0)
    raises(ValueError, ch.set_regions, [0, 1, 2], [0, 1, 2], A.dev(values(dtype, (3, 4), 0)))
    raises(ValueError, ch.set_pixels, [0, 1], [0, 1], A.dev(values(dtype, (2, 1), 0)))
    raises(IndexError, ch.set_pixels, [0, 300], [0, 1], A.dev(values(dtype, (2,), 0)))
    # __setitem__: the errors of __getitem__ for the same bad keys, exact shape and dtype
    for key, exc in [(np.s_[::-1], ValueError), (np.s_[90], IndexError), (np.s_[0, 0, 0], IndexError), (None, TypeError), (np.s_[..., 0], TypeError),
                     ([1, 2], TypeError)]:
        raises(exc, ch.__getitem__, key)
        raises(exc, ch.__setitem__, key, v)
    raises(ValueError, ch.__setitem__, np.s_[0:10, 0:11], v)
    raises(ValueError, ch.__setitem__, np.s_[0:10, 0:10], A.dev(values(np.float16, (10, 10), 0)))
    raises(TypeError, ch.__setitem__, np.s_[0:10, 0:10], 1.0)
    assert np.array_equal(A.host(ch.get_decompressed()), arr), "a refused call changed the channel"


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
    CASES[sys.argv[1]](load_module("gpu"), TorchAdapter())
    print("case %s ok" % sys.argv[1])
