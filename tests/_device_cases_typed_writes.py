"""The device-class cases of tests/test_python_window_writes_typed.py: DeviceChannel / DeviceImage set_region, set_regions and
set_pixels with dtype=, scale= and offset= (and DeviceImage's interleaved=True), in the pattern of tests/_device_cases.py (whose
adapters they use).  Run as a script -- `python _device_cases_typed_writes.py CASE` -- the file imports torch FIRST and runs CASE on
torch tensors with the product module, in a process of its own; on the mock backend the test calls the cases directly.  The plane is
512 x 130 in chunks of 30 rows.  The expectation is numpy's, separate ufunc calls: t = (y.astype(float32) - float32(offset)) /
float32(scale), then clip(rint(where(isnan(t), 0, t)), min, max) for integer pixels, astype for float ones -- assigned into a copy of
the pixels and compared bit for bit (NaN where numpy has NaN).
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import raises
from _device_cases_grouped import H, W, kw
from _device_cases_typed import nhwc, pixels

STORED = [np.uint8, np.uint16, np.int16, np.float16, np.float32]
SCALES, OFFSETS = [1 / 255, 1 / (255 * 0.229), -0.5], [0.0, -0.485 / 0.229, 3.0]
# pairs under which every 8 / 16-bit value returns to itself through a float32 read and write (checked with numpy for all four types)
ROUND_TRIP = [(1 / 255, 0.0), (1 / 65535, 0.0), (1 / (255 * 0.229), -0.485 / 0.229), (1 / 255, -0.4851), (2 / 65535, -1.0), (1 / 128, -1.0)]


def unconvert(y, stored, scale, offset):
    """numpy's answer; scale / offset: numbers, or one per channel over axis -3 of y"""
    d = np.dtype(stored)
    if y.dtype == d and np.all(np.float32(scale) == 1) and np.all(np.float32(offset) == 0):
        return y
    s, o = np.asarray(scale, np.float32), np.asarray(offset, np.float32)
    if s.ndim:
        s = s.reshape(-1, 1, 1)
    if o.ndim:
        o = o.reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        x = y.astype(np.float32)
        t = np.subtract(x, o)
        t = np.divide(t, s)
        if d.kind in "iu":
            info = np.iinfo(d)
            return np.clip(np.rint(np.where(np.isnan(t), np.float32(0), t).astype(np.float64)), info.min, info.max).astype(d)
        return t.astype(d)


def memory(mem, stored, shape, scale, offset, seed):
    """values of dtype `mem` around the stored type's range under (scale, offset): ties, both saturation edges, NaN, +-inf, -0"""
    rng = np.random.default_rng(seed)
    d = np.dtype(stored)
    lo, hi = (np.iinfo(d).min, np.iinfo(d).max) if d.kind in "iu" else (-300, 300)
    n = int(np.prod(shape))
    v = rng.integers(max(lo, -40000) - 3, min(hi, 40000) + 4, n).astype(np.float64) + rng.choice([0.0, 0.5, -0.5, 0.25, 0.49], n)
    s = np.broadcast_to(np.asarray(scale, np.float64).reshape(-1, 1, 1) if np.ndim(scale) else np.float64(scale), shape).ravel()
    o = np.broadcast_to(np.asarray(offset, np.float64).reshape(-1, 1, 1) if np.ndim(offset) else np.float64(offset), shape).ravel()
    with np.errstate(all="ignore"):
        y = (v.astype(np.float32) * s.astype(np.float32) + o.astype(np.float32)).astype(mem)
    y[::53] = np.nan
    y[7::101] = np.inf
    y[11::103] = -np.inf
    y[13::107] = -0.0
    return y.reshape(shape)


def same(got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
    eq = np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(exp).view(bits)
    if exp.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(exp)
    return bool(eq.all())


def case_channel_typed_writes(ci, A):
    rng = np.random.default_rng(3)
    for dtype in STORED:
        arr = pixels(dtype)
        for mem, sc, of in ((np.float32, 1 / 255, -0.4851), (np.float16, -0.5, 3.0), (np.float32, 2 / 65535, -1.0), (dtype, 1.0, 0.0)):
            ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
            edited = arr.copy()
            mk = (lambda shape, seed: memory(mem, dtype, shape, sc, of, seed)) if mem is not dtype else (lambda shape, seed: pixels(dtype, seed).ravel()[:int(np.prod(shape))].reshape(shape))
            # one region with steps
            for k, (x, y, w, h, sx, sy) in enumerate([(17, 4, 71, 60, 3, 5), (0, 0, W, H, 16, 16), (5, 29, 300, 3, 1, 1), (W - 1, H - 1, 1, 1, 4, 4)]):
                v = mk((-(-h // sy), -(-w // sx)), 10 + k)
                ch.set_region(x, y, A.dev(v), step_x=sx, step_y=sy, dtype=mem, scale=sc, offset=of)
                edited[y:y + h:sy, x:x + w:sx] = unconvert(v, dtype, sc, of)
                assert same(A.host(ch.get_decompressed()), edited), (dtype, mem, k)
            # batches; the last region lies on the first and wins
            for (w, h, sx, sy, n) in [(32, 16, 1, 1, 9), (40, 30, 4, 3, 6)]:
                xs, ys = rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)
                xs[-1], ys[-1] = xs[0], ys[0]
                v = mk((n, -(-h // sy), -(-w // sx)), n)
                ch.set_regions(xs, ys, A.dev(v), step_x=sx, step_y=sy, dtype=np.dtype(mem).name, scale=sc, offset=of)
                for k in range(n):
                    edited[ys[k]:ys[k] + h:sy, xs[k]:xs[k] + w:sx] = unconvert(v[k], dtype, sc, of)
                assert same(A.host(ch.get_decompressed()), edited), (dtype, mem, w, h)
            n = 300
            xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
            xs[-1], ys[-1] = xs[0], ys[0]
            v = mk((n,), 77)
            ch.set_pixels(xs, ys, A.dev(v), dtype=mem, scale=sc, offset=of)
            c = unconvert(v, dtype, sc, of)
            for k in range(n):
                edited[ys[k], xs[k]] = c[k]
            assert same(A.host(ch.get_decompressed()), edited), (dtype, mem)
            ch.set_regions([], [], A.dev(np.zeros((0, 4, 4), mem)), dtype=mem, scale=sc, offset=of)          # nothing to do
            assert same(A.host(ch.get_decompressed()), edited)
            if np.dtype(dtype).kind != "f":              # the chunks are those of a channel built from the edited pixels
                want = ci.Channel(edited, W, H, **kw(dtype))
                assert ch.compressed_bytes() == want.compressed_bytes(), (dtype, mem)


def case_image_typed_writes(ci, A):
    rng = np.random.default_rng(4)
    for dtype in STORED:
        planes = np.stack([pixels(dtype, seed=s) for s in range(3)])
        for mem, sc, of in ((np.float32, SCALES, OFFSETS), (np.float16, SCALES, 0.5), (np.float32, 2.0, OFFSETS), (dtype, 1.0, [0.0] * 3)):
            for interleaved in (False, True):
                img = ci.DeviceImage(dtype, A.dev(planes), W, H, ["r", "g", "b"], **kw(dtype))
                edited = planes.copy()
                mk = (lambda shape, seed: memory(mem, dtype, shape, sc, of, seed)) if mem is not dtype else (lambda shape, seed: np.resize(pixels(dtype, seed), shape))
                lay = (lambda a: nhwc(a)) if interleaved else (lambda a: a)
                x, y, w, h, sx, sy = 17, 4, 71, 60, 3, 5
                v = mk((3, -(-h // sy), -(-w // sx)), 21)
                img.set_region(x, y, A.dev(lay(v)), step_x=sx, step_y=sy, dtype=mem, scale=sc, offset=of, interleaved=interleaved)
                edited[:, y:y + h:sy, x:x + w:sx] = unconvert(v, dtype, sc, of)
                assert same(A.host(img.get_decompressed()), edited), (dtype, mem, interleaved)
                for (w, h, sx, sy, n) in [(224, 64, 1, 1, 4), (40, 30, 4, 3, 6)]:
                    xs, ys = rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)
                    xs[-1], ys[-1] = xs[0], ys[0]
                    v = mk((n, 3, -(-h // sy), -(-w // sx)), n)
                    img.set_regions(xs, ys, A.dev(lay(v)), step_x=sx, step_y=sy, dtype=mem, scale=sc, offset=of, interleaved=interleaved)
                    for k in range(n):
                        edited[:, ys[k]:ys[k] + h:sy, xs[k]:xs[k] + w:sx] = unconvert(v[k], dtype, sc, of)
                    assert same(A.host(img.get_decompressed()), edited), (dtype, mem, interleaved, w, h)
                n = 257
                xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
                xs[-1], ys[-1] = xs[0], ys[0]
                v = mk((3, 1, n), 31)                                           # (C, 1, N): one scale per channel over axis -3
                img.set_pixels(xs, ys, A.dev(np.ascontiguousarray(v[:, 0, :].T)), dtype=mem, scale=sc, offset=of, interleaved=interleaved)
                c = unconvert(v, dtype, sc, of)[:, 0, :]
                for k in range(n):
                    edited[:, ys[k], xs[k]] = c[:, k]
                assert same(A.host(img.get_decompressed()), edited), (dtype, mem, interleaved)


def case_round_trip(ci, A):
    """x = get_regions(dtype=float32, scale, offset); set_regions(x, dtype=float32, scale, offset): every pixel and every chunk's
    size as before (the chunk bytes are a function of the pixels; the C-ABI tests compare them byte for byte)"""
    for dtype in (np.uint8, np.int16, np.uint16):
        planes = np.stack([pixels(dtype, seed=s) for s in range(3)])
        for k, (sc, of) in enumerate(ROUND_TRIP):
            img = ci.DeviceImage(dtype, A.dev(planes), W, H, **kw(dtype))
            before = [img.channel(c).compressed_bytes(i) for c in range(3) for i in range(img.channel(c).num_chunks())]
            xs, ys = [0, 100, 288], [0, 33, 66]
            for interleaved in (False, True):
                x = img.get_regions(xs, ys, 224, 64, dtype=np.float32, scale=sc, offset=of, interleaved=interleaved)
                img.set_regions(xs, ys, x, dtype=np.float32, scale=sc, offset=of, interleaved=interleaved)
            x = img.get_region(0, 0, W, H, dtype=np.float32, scale=sc, offset=of)
            img.set_region(0, 0, x, dtype=np.float32, scale=sc, offset=of)
            assert np.array_equal(A.host(img.get_decompressed()), planes), (dtype, sc, of)
            assert before == [img.channel(c).compressed_bytes(i) for c in range(3) for i in range(img.channel(c).num_chunks())]
    # float16 memory holds every uint8 under (1 / 255, 0)
    arr = pixels(np.uint8)
    ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(np.uint8))
    x = ch.get_region(0, 0, W, H, dtype=np.float16, scale=1 / 255)
    ch.set_region(0, 0, x, dtype=np.float16, scale=1 / 255)
    assert np.array_equal(A.host(ch.get_decompressed()), arr)


def case_typed_write_errors(ci, A):
    arr = pixels(np.uint16)
    ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(np.uint16))
    f = A.dev(np.zeros((4, 4), np.float32))
    u = A.dev(np.zeros((4, 4), np.uint16))
    # without dtype= nothing changes: an array of another dtype is a ValueError, scale / offset need dtype=
    raises(ValueError, ch.set_region, 0, 0, f)
    raises(ValueError, ch.set_region, 0, 0, u, scale=2.0)
    raises(ValueError, ch.set_region, 0, 0, u, offset=1.0)
    raises(ValueError, ch.set_regions, [0], [0], A.dev(np.zeros((1, 4, 4), np.uint16)), scale=0.5)
    raises(ValueError, ch.set_pixels, [0], [0], A.dev(np.zeros((1,), np.uint16)), offset=0.5)
    # with dtype=: float32, float16 or the stored dtype; the array must have exactly it
    raises(ValueError, ch.set_region, 0, 0, A.dev(np.zeros((4, 4), np.float64)), dtype=np.float64)
    raises(ValueError, ch.set_region, 0, 0, A.dev(np.zeros((4, 4), np.uint8)), dtype=np.uint8)
    raises(TypeError, ch.set_region, 0, 0, u, dtype=np.float32)
    raises(TypeError, ch.set_region, 0, 0, f, dtype=np.float16)
    raises(TypeError, ch.set_regions, [0], [0], A.dev(np.zeros((1, 4, 4), np.float16)), dtype=np.float32)
    raises(TypeError, ch.set_pixels, [0], [0], A.dev(np.zeros((1,), np.float32)), dtype=np.uint16)
    raises(TypeError, ch.set_region, 0, 0, np.zeros((4, 4), np.float32), dtype=np.float32)          # host memory
    raises(ValueError, ch.set_region, 0, 0, u, dtype=np.uint16, scale=2.0)                           # an integer dtype is the identity only
    raises(ValueError, ch.set_region, 0, 0, u, dtype=np.uint16, offset=1.0)
    raises(ValueError, ch.set_region, 0, 0, f, dtype=np.float32, scale=[1.0, 2.0])                   # a channel has one scale
    for bad in (0.0, float("nan"), float("inf"), -float("inf"), 1e-50):
        raises(ValueError, ch.set_region, 0, 0, f, dtype=np.float32, scale=bad)
    raises(ValueError, ch.set_region, 0, 0, f, dtype=np.float32, offset=float("nan"))
    raises(ValueError, ch.set_region, 0, 0, f, dtype=np.float32, offset=float("inf"))
    # the errors of the plain calls, with dtype=
    raises(ValueError, ch.set_region, 0, 0, f, dtype=np.float32, step_x=0)
    raises(IndexError, ch.set_region, W - 3, 0, f, dtype=np.float32)
    raises(IndexError, ch.set_region, 0, 0, f, dtype=np.float32, step_y=50)
    raises(ValueError, ch.set_region, 0, 0, A.dev(np.zeros((4,), np.float32)), dtype=np.float32)
    vs = A.dev(np.zeros((3, 4, 4), np.float32))
    raises(ValueError, ch.set_regions, [0, 1], [0, 1], vs, dtype=np.float32)
    raises(IndexError, ch.set_regions, [0, 1, W - 3], [0, 1, 2], vs, dtype=np.float32)
    raises(IndexError, ch.set_pixels, [0, W], [0, 1], A.dev(np.zeros((2,), np.float32)), dtype=np.float32)
    assert np.array_equal(A.host(ch.get_decompressed()), arr), "a refused call changed the channel"
    ch64 = ci.DeviceChannel(A.dev(arr.astype(np.float64)), W, H, **kw(np.float64))
    raises(ValueError, ch64.set_region, 0, 0, f, dtype=np.float32)                                   # float64 pixels: the identity only
    ch64.set_region(0, 0, A.dev(np.ones((4, 4), np.float64)), dtype=np.float64)
    assert (A.host(ch64.get_region(0, 0, 4, 4)) == 1).all()

    planes = np.stack([pixels(np.uint8, seed=s) for s in range(3)])
    img = ci.DeviceImage(np.uint8, A.dev(planes), W, H, **kw(np.uint8))
    p = A.dev(np.zeros((3, 4, 4), np.float32))
    q = A.dev(np.zeros((4, 4, 3), np.float32))
    raises(ValueError, img.set_region, 0, 0, p)                                                      # another dtype, no dtype=
    raises(ValueError, img.set_region, 0, 0, A.dev(np.zeros((3, 4, 4), np.uint8)), scale=[1.0, 2.0, 1.0])
    raises(ValueError, img.set_region, 0, 0, A.dev(np.zeros((4, 4, 3), np.uint8)), interleaved=True)
    raises(ValueError, img.set_regions, [0], [0], A.dev(np.zeros((1, 4, 4, 3), np.uint8)), interleaved=True)
    raises(ValueError, img.set_pixels, [0], [0], A.dev(np.zeros((1, 3), np.uint8)), offset=0.5)
    raises(ValueError, img.set_region, 0, 0, p, dtype=np.float32, scale=[1.0, 2.0])                  # neither one nor one per channel
    raises(ValueError, img.set_region, 0, 0, p, dtype=np.float32, offset=[0.0] * 4)
    raises(ValueError, img.set_region, 0, 0, p, dtype=np.float32, scale=[1.0, 0.0, 1.0])
    raises(ValueError, img.set_region, 0, 0, p, dtype=np.int16)
    raises(TypeError, img.set_region, 0, 0, p, dtype=np.float16)
    raises(ValueError, img.set_region, 0, 0, A.dev(np.zeros((3, 4, 4), np.uint8)), dtype=np.uint8, scale=[1.0, 1.0, 2.0])
    raises(ValueError, img.set_region, 0, 0, p, dtype=np.float32, interleaved=True)                  # (3, 4, 4) is not (h, w, 3)
    raises(ValueError, img.set_region, 0, 0, q, dtype=np.float32)
    raises(ValueError, img.set_regions, [0], [0], A.dev(np.zeros((1, 3, 4, 4), np.float32)), dtype=np.float32, interleaved=True)
    raises(ValueError, img.set_regions, [0], [0], A.dev(np.zeros((1, 4, 4, 3), np.float32)), dtype=np.float32)
    raises(IndexError, img.set_regions, [0, 0], [0, H - 3], A.dev(np.zeros((2, 4, 4, 3), np.float16)), dtype=np.float16, interleaved=True)
    raises(ValueError, img.set_pixels, [0], [0], A.dev(np.zeros((1, 2), np.float32)), dtype=np.float32)
    assert np.array_equal(A.host(img.get_decompressed()), planes), "a refused call changed the image"
    img.set_region(0, 0, q, dtype=np.float32, scale=SCALES, offset=OFFSETS, interleaved=True)
    assert same(A.host(img.get_region(0, 0, 4, 4)), unconvert(np.zeros((3, 4, 4), np.float32), np.uint8, SCALES, OFFSETS))


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
