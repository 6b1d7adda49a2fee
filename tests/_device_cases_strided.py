"""The device-class cases of tests/test_python_windows_strided.py: DeviceChannel / DeviceImage get_region with steps and
DeviceChannel.__getitem__, in the pattern of tests/_device_cases.py (whose adapters they use).  Run as a script --
`python _device_cases_strided.py CASE` -- the file imports torch FIRST and runs CASE on torch tensors with the product module, in a
process of its own; on the mock backend the test calls the cases directly.
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import H, W, kw, pixels, raises

DTYPES = [np.uint8, np.uint16, np.float16, np.float32]
# (x, y, width, height, step_x, step_y)
STEPPED = [(0, 0, W, H, 2, 2), (0, 0, W, H, 1, 3), (0, 0, W, H, 7, 1), (5, 3, 200, 80, 16, 8), (17, 4, 71, 60, 3, 5), (0, 0, W, H, W + 5, H + 5),
           (290, 89, 10, 1, 4, 4), (3, 30, 200, 7, 199, 6), (0, 0, W, H, W - 1, H - 1), (10, 10, 0, 5, 2, 2), (10, 10, 5, 0, 3, 1)]
KEYS = [
    0, 5, -1, -H, H - 1, (3, 7), (-2, -3), (0, slice(None)), (slice(None), 0), (slice(None), -1),
    slice(None), slice(None, None, 2), slice(3, None), slice(None, 11), slice(-20, -3, 4), slice(5, 5), slice(50, 10), slice(H, None),
    slice(-1000, 1000, 9), slice(None, None, H + 7), slice(2, 3, 1000),
    (slice(None), slice(None)), (slice(None, None, 3), slice(None, None, 5)), (slice(1, None, 8), slice(2, None, 16)),
    (slice(10, 80, 7), slice(-250, -5, 13)), (slice(None), slice(None, None, W + 3)), (slice(None, None, H), slice(None, None, W)),
    (slice(4, 4), slice(None)), (slice(None), slice(9, 2)), (slice(4, 4), 3), (7, slice(W, None)), (slice(0, 1000), slice(0, 1000, 299)),
    (np.int64(4), slice(None, None, 2)), (slice(np.int32(2), np.int64(30), np.int16(3)), 5), (),
]
BAD_KEYS = [(H, IndexError), (-H - 1, IndexError), ((0, W), IndexError), ((0, -W - 1), IndexError), ((0, 0, 0), IndexError),
            (slice(None, None, -1), ValueError), ((slice(None), slice(10, 2, -2)), ValueError), (slice(None, None, 0), ValueError),
            (Ellipsis, (TypeError, ValueError)), ((Ellipsis, 0), (TypeError, ValueError)), (None, (TypeError, ValueError)),
            ((None, 0), (TypeError, ValueError)), ([0, 1], (TypeError, ValueError)), (np.array([0, 2]), (TypeError, ValueError)),
            ((slice(None), np.array([True] * W)), (TypeError, ValueError)), (1.5, (TypeError, ValueError)), ("r", (TypeError, ValueError)),
            (True, (TypeError, ValueError))]


def stepped(a, x, y, w, h, sx, sy):
    return a[..., y:y + h:sy, x:x + w:sx]


def case_channel_steps(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        for codec in D.codecs(ci):
            ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=codec, **kw(dtype))
            want = A.host(ch.get_decompressed())
            assert np.array_equal(want, arr)
            for i, (x, y, w, h, sx, sy) in enumerate(STEPPED):
                exp = stepped(want, x, y, w, h, sx, sy)
                if i % 2:
                    out = A.empty(exp.shape, dtype)
                    r = ch.get_region(x, y, w, h, out=out, step_x=sx, step_y=sy)
                    assert r is out
                else:
                    r = ch.get_region(x, y, w, h, step_x=sx, step_y=sy)
                    assert r.shape == exp.shape, (r.shape, exp.shape)
                assert np.array_equal(A.host(r), exp), (dtype, codec, x, y, w, h, sx, sy)
    ch = ci.DeviceChannel(A.dev(pixels(np.uint16, W, H)), W, H, **kw(np.uint16))
    raises(ValueError, ch.get_region, 0, 0, 10, 10, step_x=0)
    raises(ValueError, ch.get_region, 0, 0, 10, 10, step_y=-2)
    raises(ValueError, ch.get_region, 0, 0, 10, 10, out=A.empty((10, 10), np.uint16), step_x=2)       # out takes the subsampled shape
    raises((IndexError, ValueError), ch.get_region, 0, 0, W + 1, 10, step_x=2)
    assert np.array_equal(A.host(ch.get_region(2, 3, 50, 40)), pixels(np.uint16, W, H)[3:43, 2:52])    # the defaults are the old call


def case_channel_getitem(ci, A):
    for dtype in (np.uint8, np.float32):
        arr = pixels(dtype, W, H)
        ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        want = A.host(ch.get_decompressed())
        for key in KEYS:
            r = ch[key]
            assert isinstance(r, ci.DeviceArray)
            exp = want[key]
            assert tuple(r.shape) == exp.shape and r.dtype == exp.dtype, (key, r.shape, exp.shape)
            got = r.copy_to_host() if exp.size == 0 else A.host(r)                  # (an empty selection: nothing for torch to wrap)
            assert got.shape == exp.shape and np.array_equal(got, exp), key
        for key, exc in BAD_KEYS:
            raises(exc, ch.__getitem__, key)


def case_image_steps(ci, A):
    for dtype in DTYPES:
        planes = np.stack([pixels(dtype, W, H, seed=s) for s in range(3)])
        img = ci.DeviceImage(dtype, A.dev(planes), W, H, ["r", "g", "b"], **kw(dtype))
        want = A.host(img.get_decompressed())
        assert np.array_equal(want, planes)
        for i, (x, y, w, h, sx, sy) in enumerate(STEPPED):
            exp = stepped(want, x, y, w, h, sx, sy)
            r = img.get_region(x, y, w, h, step_x=sx, step_y=sy)
            assert tuple(r.shape) == exp.shape and np.array_equal(A.host(r), exp), (dtype, x, y, w, h, sx, sy)
            if exp.size == 0:
                continue
            expi = np.ascontiguousarray(exp.transpose(1, 2, 0))
            if i % 2:
                out = A.empty(expi.shape, dtype)
                r = img.get_region(x, y, w, h, out=out, interleaved=True, step_x=sx, step_y=sy)
                assert r is out
            else:
                r = img.get_region(x, y, w, h, interleaved=True, step_x=sx, step_y=sy)
            assert A.host(r).shape == expi.shape and np.array_equal(A.host(r), expi), (dtype, x, y, w, h, sx, sy)
        # a channel of the image, its steps and its keys
        g = img.channel("g")
        assert np.array_equal(A.host(g.get_region(4, 4, 100, 50, step_x=9, step_y=2)), want[1][4:54:2, 4:104:9])
        assert np.array_equal(A.host(g[::7, 3::11]), want[1][::7, 3::11])
    raises(ValueError, img.get_region, 0, 0, 10, 10, step_x=0)
    raises(ValueError, img.get_region, 0, 0, 10, 10, out=A.empty((3, 10, 10), DTYPES[-1]), step_y=3)


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
