"""The device-class cases of tests/test_python_windows_typed.py: DeviceChannel / DeviceImage get_region, get_regions and get_pixels
with dtype=, scale= and offset= (and DeviceImage.get_regions(interleaved=True)), in the pattern of tests/_device_cases.py (whose
adapters they use).  Run as a script -- `python _device_cases_typed.py CASE` -- the file imports torch FIRST and runs CASE on torch
tensors with the product module, in a process of its own; on the mock backend the test calls the cases directly.  The plane is
512 x 130 in chunks of 30 rows.  The expectation is numpy's, two ufunc calls: (v.astype(float32) * float32(scale) +
float32(offset)).astype(dtype), compared bit for bit.
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import raises
from _device_cases_grouped import BATCHES, H, W, crops, kw, probe_points

STORED = [np.uint8, np.uint16, np.int16, np.float16, np.float32]
SCALES, OFFSETS = [1 / 255, 1 / 58.395, -0.4851], [-0.485, 0.406, 3.0e-41]


def pixels(dtype, seed=0):
    """the tiled pixels of _device_cases stretched over the dtype's range (float: fractions and negative values too)"""
    a = D.pixels(np.int64, W, H, seed)
    d = np.dtype(dtype)
    if d.kind == "f":
        return ((a - 90) * 0.37).astype(dtype)
    info = np.iinfo(d)
    return (a * 331 % (int(info.max) - int(info.min) + 1) + int(info.min)).astype(dtype)


def convert(v, dtype, scale, offset):
    """numpy's answer; scale / offset: numbers, or one per channel over axis -3 of v"""
    if np.dtype(dtype) == v.dtype and np.all(np.float32(scale) == 1) and np.all(np.float32(offset) == 0):
        return v
    s, o = np.asarray(scale, np.float32), np.asarray(offset, np.float32)
    if s.ndim:
        s = s.reshape(-1, 1, 1)
    if o.ndim:
        o = o.reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        y = v.astype(np.float32) * s
        y = y + o
        return y.astype(dtype)


def same(got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(bits), np.ascontiguousarray(exp).view(bits))


def host(A, r, exp):
    return r.copy_to_host() if exp.size == 0 else A.host(r)


def case_channel_typed(ci, A):
    for dtype in STORED:
        arr = pixels(dtype)
        ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        for out_dtype, sc, of in ((np.float32, 1 / 255, -0.4851), (np.float16, -0.4851, 1 / 255), (dtype, 1.0, 0.0)):
            for i, (xs, ys, w, h, sx, sy) in enumerate(BATCHES):
                exp = convert(crops(arr, xs, ys, w, h, sx, sy), out_dtype, sc, of)
                if i % 2 and exp.size:
                    out = A.empty(exp.shape, out_dtype)
                    r = ch.get_regions(xs, ys, w, h, out=out, step_x=sx, step_y=sy, dtype=out_dtype, scale=sc, offset=of)
                    assert r is out
                else:
                    r = ch.get_regions(np.asarray(xs), ys, w, h, step_x=sx, step_y=sy, dtype=out_dtype, scale=sc, offset=of)
                    assert isinstance(r, ci.DeviceArray) and r.dtype == np.dtype(out_dtype)
                assert same(host(A, r, exp), exp), (dtype, out_dtype, i)
            # one region, subsampled; out= given and omitted
            exp = convert(arr[4:64:5, 17:88:3], out_dtype, sc, of)
            assert same(A.host(ch.get_region(17, 4, 71, 60, step_x=3, step_y=5, dtype=out_dtype, scale=sc, offset=of)), exp)
            out = A.empty(exp.shape, out_dtype)
            assert ch.get_region(17, 4, 71, 60, out=out, step_x=3, step_y=5, dtype=np.dtype(out_dtype).name, scale=sc, offset=of) is out
            assert same(A.host(out), exp)
            xs, ys = probe_points(300)
            exp = convert(arr[ys, xs], out_dtype, sc, of)
            assert same(A.host(ch.get_pixels(xs, ys, dtype=out_dtype, scale=sc, offset=of)), exp)
            out = A.empty((300,), out_dtype)
            assert ch.get_pixels(xs, ys, out=out, dtype=out_dtype, scale=sc, offset=of) is out and same(A.host(out), exp)
        # empty batches keep their shape and take the new dtype
        r = ch.get_regions([], [], 7, 5, step_x=2, dtype=np.float16, scale=2.0)
        assert tuple(r.shape) == (0, 5, 4) and r.dtype == np.float16
        assert ch.get_pixels([], [], dtype=np.float32).dtype == np.float32
    ch = ci.DeviceChannel(A.dev(pixels(np.uint16)), W, H, **kw(np.uint16))
    # without dtype= nothing changes: out of another dtype is a TypeError, scale / offset a ValueError
    raises(TypeError, ch.get_region, 0, 0, 4, 4, out=A.empty((4, 4), np.float32))
    raises(ValueError, ch.get_region, 0, 0, 4, 4, scale=2.0)
    raises(ValueError, ch.get_regions, [0], [0], 4, 4, offset=1.0)
    raises(ValueError, ch.get_pixels, [0], [0], scale=0.5)
    # with dtype=: out must have it (TypeError) and the result's shape (ValueError); only float32, float16 or the stored dtype
    raises(TypeError, ch.get_region, 0, 0, 4, 4, out=A.empty((4, 4), np.uint16), dtype=np.float32)
    raises(TypeError, ch.get_regions, [0, 1], [0, 0], 4, 4, out=A.empty((2, 4, 4), np.float32), dtype=np.float16)
    raises(ValueError, ch.get_region, 0, 0, 4, 4, out=A.empty((4, 5), np.float32), dtype=np.float32)
    raises(ValueError, ch.get_pixels, [0, 1], [0, 0], out=A.empty((3,), np.float32), dtype=np.float32)
    raises(ValueError, ch.get_region, 0, 0, 4, 4, dtype=np.float64)
    raises(ValueError, ch.get_region, 0, 0, 4, 4, dtype=np.uint8)
    raises(ValueError, ch.get_region, 0, 0, 4, 4, dtype=np.uint16, scale=2.0)              # an integer result is the identity only
    raises(ValueError, ch.get_region, 0, 0, 4, 4, dtype=np.float32, scale=[1.0, 2.0])      # a channel has one scale
    raises(IndexError, ch.get_regions, [0, W - 3], [0, 0], 4, 4, dtype=np.float32)
    raises(ValueError, ch.get_region, 0, 0, 4, 4, dtype=np.float32, step_x=0)
    out = A.empty((2, 4, 4), np.float32)
    raises(IndexError, ch.get_regions, [0, W - 3], [0, 0], 4, 4, out=out, dtype=np.float32)
    assert np.array_equal(A.host(out), A.host(A.empty((2, 4, 4), np.float32)))             # nothing written


def nhwc(a):
    """(N, C, h, w) -> (N, h, w, C)"""
    return np.ascontiguousarray(np.moveaxis(a, -3, -1))


def case_image_typed(ci, A):
    for dtype in STORED:
        planes = np.stack([pixels(dtype, seed=s) for s in range(3)])
        img = ci.DeviceImage(dtype, A.dev(planes), W, H, ["r", "g", "b"], **kw(dtype))
        for out_dtype, sc, of in ((np.float32, SCALES, OFFSETS), (np.float16, SCALES, 0.5), (np.float32, 2.0, OFFSETS), (dtype, 1.0, [0.0] * 3)):
            for interleaved in (False, True):
                for i, (xs, ys, w, h, sx, sy) in enumerate(BATCHES):
                    exp = convert(crops(planes, xs, ys, w, h, sx, sy), out_dtype, sc, of)
                    exp = nhwc(exp) if interleaved else exp
                    if i % 2 and exp.size:
                        out = A.empty(exp.shape, out_dtype)
                        r = img.get_regions(xs, ys, w, h, out=out, step_x=sx, step_y=sy, dtype=out_dtype, scale=sc, offset=of, interleaved=interleaved)
                        assert r is out
                    else:
                        r = img.get_regions(xs, ys, w, h, step_x=sx, step_y=sy, dtype=out_dtype, scale=sc, offset=of, interleaved=interleaved)
                        assert tuple(r.shape) == exp.shape and r.dtype == np.dtype(out_dtype), (r.shape, exp.shape)
                    assert same(host(A, r, exp), exp), (dtype, out_dtype, interleaved, i)
                exp = convert(planes[:, 4:64:5, 17:88:3], out_dtype, sc, of)
                exp = nhwc(exp) if interleaved else exp
                r = img.get_region(17, 4, 71, 60, interleaved=interleaved, step_x=3, step_y=5, dtype=out_dtype, scale=sc, offset=of)
                assert tuple(r.shape) == exp.shape and same(A.host(r), exp)
                out = A.empty(exp.shape, out_dtype)
                assert img.get_region(17, 4, 71, 60, out=out, interleaved=interleaved, step_x=3, step_y=5, dtype=out_dtype, scale=sc, offset=of) is out
                assert same(A.host(out), exp)
            xs, ys = probe_points(257, seed=9)
            exp = np.ascontiguousarray(convert(planes[:, ys, xs][:, None, :], out_dtype, sc, of)[:, 0, :].T)
            assert same(A.host(img.get_pixels(xs, ys, dtype=out_dtype, scale=sc, offset=of)), exp)
        # interleaved=True without dtype: the stored type, pixel-major, in the one call
        xs, ys, w, h, sx, sy = BATCHES[1]
        exp = nhwc(crops(planes, xs, ys, w, h, sx, sy))
        r = img.get_regions(xs, ys, w, h, interleaved=True)
        assert r.dtype == np.dtype(dtype) and same(A.host(r), exp)
        # the same pixels as the existing pixel-major get_region
        assert same(A.host(img.get_region(96, 20, 224, 64, interleaved=True)), A.host(img.get_regions([96], [20], 224, 64, interleaved=True))[0])
        r = img.get_regions([], [], 6, 6, dtype=np.float16, interleaved=True)
        assert tuple(r.shape) == (0, 6, 6, 3) and r.dtype == np.float16
        assert tuple(img.get_regions([], [], 6, 6, dtype=np.float32).shape) == (0, 3, 6, 6)
        assert tuple(img.get_pixels([], [], dtype=np.float32).shape) == (0, 3)
    img = ci.DeviceImage(np.uint8, A.dev(np.stack([pixels(np.uint8, seed=s) for s in range(3)])), W, H, **kw(np.uint8))
    raises(TypeError, img.get_region, 0, 0, 4, 4, out=A.empty((3, 4, 4), np.float32))
    raises(ValueError, img.get_region, 0, 0, 4, 4, scale=[1.0, 2.0, 1.0])
    raises(ValueError, img.get_regions, [0], [0], 4, 4, offset=0.5)
    raises(ValueError, img.get_pixels, [0], [0], scale=2.0)
    raises(TypeError, img.get_regions, [0], [0], 4, 4, out=A.empty((1, 3, 4, 4), np.uint8), dtype=np.float32)
    raises(ValueError, img.get_regions, [0], [0], 4, 4, out=A.empty((1, 3, 4, 4), np.float32), dtype=np.float32, interleaved=True)
    raises(ValueError, img.get_regions, [0], [0], 4, 4, out=A.empty((1, 4, 4, 3), np.float32), dtype=np.float32)
    raises(ValueError, img.get_region, 0, 0, 4, 4, dtype=np.float32, scale=[1.0, 2.0])      # neither one nor one per channel
    raises(ValueError, img.get_region, 0, 0, 4, 4, dtype=np.float32, offset=[0.0] * 4)
    raises(ValueError, img.get_region, 0, 0, 4, 4, dtype=np.int16)
    raises(ValueError, img.get_region, 0, 0, 4, 4, dtype=np.uint8, scale=[1.0, 1.0, 2.0])
    raises(IndexError, img.get_regions, [0, 0], [0, H - 3], 4, 4, dtype=np.float16, interleaved=True)
    out = A.empty((4, 4, 3), np.float32)
    assert img.get_region(0, 0, 4, 4, out=out, interleaved=True, dtype=np.float32, scale=SCALES, offset=OFFSETS) is out


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
