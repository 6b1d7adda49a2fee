"""The device-class cases of tests/test_python_windows_grouped.py: DeviceChannel / DeviceImage get_regions and get_pixels, in the
pattern of tests/_device_cases.py (whose adapters they use).  Run as a script -- `python _device_cases_grouped.py CASE` -- the file
imports torch FIRST and runs CASE on torch tensors with the product module, in a process of its own; on the mock backend the test
calls the cases directly.  The plane is 512 x 130 in chunks of 30 rows: four full chunks and a leftover chunk of 10 rows.
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import pixels, raises

W, H = 512, 130
DTYPES = [np.uint8, np.uint16, np.float16, np.float32]
# (xs, ys, width, height, step_x, step_y): a row of tiles; crops over every chunk boundary, the leftover chunk and the last row and
# column, one of them twice; subsampled; one region; the whole plane twice
BATCHES = [
    ([0, 128, 256, 384], [10, 10, 10, 10], 128, 40, 1, 1),
    ([3, 200, 200, 412, 0, 77], [0, 25, 25, 55, 119, 90], 100, 11, 1, 1),
    ([0, 5, 11, 212], [0, 58, 100, 1], 300, 29, 7, 3),
    ([17], [4], 71, 60, 3, 5),
    ([0, 0], [0, 0], W, H, 1, 1),
    ([1, 2, 3], [4, 5, 6], 0, 3, 1, 1),
    ([1, 2, 3], [4, 5, 6], 3, 0, 2, 2),
]


def kw(dtype):
    return dict(block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 30)


def crops(a, xs, ys, w, h, sx=1, sy=1):
    """numpy's answer: (N, [C,] h', w') from a (H, W) or (C, H, W) array"""
    shape = (0,) + a.shape[:-2] + (-(-h // sy), -(-w // sx))
    if len(xs) == 0:
        return np.zeros(shape, a.dtype)
    return np.stack([a[..., y:y + h:sy, x:x + w:sx] for x, y in zip(xs, ys)])


def probe_points(n, seed=5):
    rng = np.random.default_rng(seed)
    xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
    xs[:4], ys[:4] = [0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1]
    return xs, ys


def bad_calls(o, extra=()):
    """every error of get_regions / get_pixels, as callables with the exception they must raise"""
    return [
        (ValueError, lambda: o.get_regions([0, 1], [0], 4, 4, *extra)),                                  # unequal lengths
        (ValueError, lambda: o.get_pixels([0, 1, 2], [0, 1], *extra)),
        (ValueError, lambda: o.get_regions(np.array([0.0, 1.0]), [0, 1], 4, 4, *extra)),                # non-integer arrays
        (ValueError, lambda: o.get_pixels([0, 1], np.array([0.5, 1.0]), *extra)),
        (ValueError, lambda: o.get_pixels(np.array([True, False]), [0, 1], *extra)),
        (ValueError, lambda: o.get_regions(np.zeros((2, 2), np.int64), [0, 1], 4, 4, *extra)),
        (ValueError, lambda: o.get_regions([0], [0], 4, 4, *extra, step_x=0)),
        (ValueError, lambda: o.get_regions([0], [0], 4, 4, *extra, step_y=-1)),
        (ValueError, lambda: o.get_regions([0], [0], -1, 4, *extra)),
        (IndexError, lambda: o.get_regions([0, W - 3], [0, 0], 4, 4, *extra)),                           # the second leaves the plane
        (IndexError, lambda: o.get_regions([0, 0], [0, H - 3], 4, 4, *extra)),
        (IndexError, lambda: o.get_regions([0, -1], [0, 0], 4, 4, *extra)),
        (IndexError, lambda: o.get_pixels([0, W], [0, 0], *extra)),
        (IndexError, lambda: o.get_pixels([0, 0], [0, H], *extra)),
        (IndexError, lambda: o.get_pixels([5], [-2], *extra)),
    ]


def case_channel_regions(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        for codec in D.codecs(ci):
            ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=codec, **kw(dtype))
            assert ch.num_chunks() == 5
            for i, (xs, ys, w, h, sx, sy) in enumerate(BATCHES):
                exp = crops(arr, xs, ys, w, h, sx, sy)
                if i % 2 and exp.size:
                    out = A.empty(exp.shape, dtype)
                    r = ch.get_regions(np.asarray(xs), np.asarray(ys, np.int32), w, h, out=out, step_x=sx, step_y=sy)
                    assert r is out
                else:
                    r = ch.get_regions(xs, ys, w, h, step_x=sx, step_y=sy)
                    assert isinstance(r, ci.DeviceArray) and tuple(r.shape) == exp.shape and r.dtype == exp.dtype, (r.shape, exp.shape)
                got = r.copy_to_host() if exp.size == 0 else A.host(r)
                assert np.array_equal(got, exp), (dtype, codec, i)
            xs, ys = probe_points(300)
            r = ch.get_pixels(xs, ys)
            assert tuple(r.shape) == (300,) and np.array_equal(A.host(r), arr[ys, xs])
            out = A.empty((300,), dtype)
            assert ch.get_pixels(list(map(int, xs)), tuple(map(int, ys)), out=out) is out and np.array_equal(A.host(out), arr[ys, xs])
    ch = ci.DeviceChannel(A.dev(pixels(np.uint16, W, H)), W, H, **kw(np.uint16))
    r = ch.get_regions([], [], 7, 5, step_x=2)
    assert tuple(r.shape) == (0, 5, 4) and r.copy_to_host().shape == (0, 5, 4)
    assert tuple(ch.get_pixels(np.zeros(0, np.int64), []).shape) == (0,)
    for exc, fn in bad_calls(ch):
        raises(exc, fn)
    # nothing is written when a region is out of bounds, and out must have the result's shape and dtype
    out = A.empty((2, 4, 4), np.uint16)
    raises(IndexError, ch.get_regions, [0, W - 3], [0, 0], 4, 4, out=out)
    assert np.array_equal(A.host(out), A.host(A.empty((2, 4, 4), np.uint16)))
    raises(ValueError, ch.get_regions, [0, 1], [0, 0], 4, 4, out=A.empty((2, 4, 5), np.uint16))
    raises(ValueError, ch.get_pixels, [0, 1], [0, 0], out=A.empty((2, 1, 1), np.uint16))
    raises(TypeError, ch.get_pixels, [0, 1], [0, 0], out=A.empty((2,), np.uint8))


def case_image_regions(ci, A):
    for dtype in DTYPES:
        planes = np.stack([pixels(dtype, W, H, seed=s) for s in range(3)])
        img = ci.DeviceImage(dtype, A.dev(planes), W, H, ["r", "g", "b"], **kw(dtype))
        for i, (xs, ys, w, h, sx, sy) in enumerate(BATCHES):
            exp = crops(planes, xs, ys, w, h, sx, sy)
            assert exp.shape[:2] == (len(xs), 3)
            if i % 2 and exp.size:
                out = A.empty(exp.shape, dtype)
                r = img.get_regions(xs, ys, w, h, out=out, step_x=sx, step_y=sy)
                assert r is out
            else:
                r = img.get_regions(np.asarray(xs, np.uint32), ys, w, h, step_x=sx, step_y=sy)
                assert tuple(r.shape) == exp.shape, (r.shape, exp.shape)
            got = r.copy_to_host() if exp.size == 0 else A.host(r)
            assert np.array_equal(got, exp), (dtype, i)
        xs, ys = probe_points(257, seed=9)
        r = img.get_pixels(xs, ys)
        assert tuple(r.shape) == (257, 3) and np.array_equal(A.host(r), planes[:, ys, xs].T)
        # a channel of the image reads the same
        assert np.array_equal(A.host(img.channel("g").get_pixels(xs, ys)), planes[1][ys, xs])
    r = img.get_regions([], [], 6, 6)
    assert tuple(r.shape) == (0, 3, 6, 6)
    assert tuple(img.get_pixels([], []).shape) == (0, 3)
    for exc, fn in bad_calls(img):
        raises(exc, fn)
    out = A.empty((2, 3), DTYPES[-1])
    raises(IndexError, img.get_pixels, [0, W], [0, 0], out=out)
    assert np.array_equal(A.host(out), A.host(A.empty((2, 3), DTYPES[-1])))


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
