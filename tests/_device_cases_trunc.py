"""The device-class cases of tests/test_python_trunc_prec.py: `mantissa_bits` on DeviceChannel / DeviceImage of the `compressed_image`
module, in the pattern of tests/_device_cases.py (whose adapters they use).  Run as a script -- `python _device_cases_trunc.py CASE` --
the file imports torch FIRST, loads the product module and runs CASE on torch tensors in a process of its own.  Expectations are the
source pixels truncated in numpy."""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import raises

W, H = 300, 90
FLOATS = [(np.float16, 5), (np.float32, 12), (np.float32, 23), (np.float64, 30)]
MANTISSA = {2: 10, 4: 23, 8: 52}


def fpixels(dtype, width, height, seed=0):
    """a smooth ramp with noise in every mantissa bit"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    return ((x // 7) * 0.25 + (y // 5) * 1.5 + rng.standard_normal((height, width))).astype(dtype)


def trunc(a, bits):
    a = np.ascontiguousarray(a)
    it = a.dtype.itemsize
    u = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[it])
    mask = ~((1 << (MANTISSA[it] - bits)) - 1) & ((1 << (8 * it)) - 1)
    return (u & u.dtype.type(mask)).view(a.dtype)


def same(a, b):
    """bit for bit (NaN-safe, -0.0 != 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def kw(dtype):
    return dict(block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 13)


def case_channel(ci, A):
    for dtype, m in FLOATS:
        arr = fpixels(dtype, W, H)
        want = trunc(arr, m)
        assert m == MANTISSA[np.dtype(dtype).itemsize] or not same(want, arr)
        for codec in D.codecs(ci):
            src = A.dev(arr)
            ch = ci.DeviceChannel(src, W, H, compression_codec=codec, mantissa_bits=m, **kw(dtype))
            assert ch.mantissa_bits() == m
            assert same(A.host(src), arr), "the caller's pixels were modified"
            assert same(A.host(ch.get_decompressed()), want), (dtype, codec)
            assert same(A.host(ch.get_region(17, 4, 71, 60)), want[4:64, 17:88])
            # what is written later is truncated too
            patch = fpixels(dtype, 120, 33, seed=7)
            ch.set_region(40, 20, A.dev(patch))
            edited = want.copy()
            edited[20:53, 40:160] = trunc(patch, m)
            assert same(A.host(ch.get_decompressed()), edited), (dtype, codec)
            # the parameter travels with the chunks
            down = ch.to_channel()
            assert down.mantissa_bits() == m and same(down.get_decompressed(), edited)
            down.set_region(0, 0, patch)                                    # ... and the host channel goes on truncating
            edited[0:33, 0:120] = trunc(patch, m)
            assert same(down.get_decompressed(), edited)
            up = ci.DeviceChannel.from_channel(down)
            assert up.mantissa_bits() == m and same(A.host(up.get_decompressed()), edited)
        plain = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        assert plain.mantissa_bits() is None and same(A.host(plain.get_decompressed()), arr)
        assert plain.to_channel().mantissa_bits() is None


def case_image(ci, A):
    for dtype, m in FLOATS[:2]:
        stack = np.stack([fpixels(dtype, W, H, seed=c) for c in range(3)])
        want = trunc(stack, m)
        img = ci.DeviceImage(dtype, A.dev(stack), W, H, channel_names=["R", "G", "B"], mantissa_bits=m, **kw(dtype))
        assert img.mantissa_bits() == m and img.channel("G").mantissa_bits() == m
        assert same(A.host(img.get_decompressed()), want)
        assert same(A.host(img.get_region(17, 4, 71, 60)), want[:, 4:64, 17:88])
        patch = np.stack([fpixels(dtype, 120, 33, seed=50 + c) for c in range(3)])
        img.set_region(40, 20, A.dev(patch))
        edited = want.copy()
        edited[:, 20:53, 40:160] = trunc(patch, m)
        assert same(A.host(img.get_decompressed()), edited)
        down = img.to_image()
        assert down.mantissa_bits() == m and same(down.get_decompressed(), edited)
        up = ci.DeviceImage.from_image(down)
        assert up.mantissa_bits() == m and same(A.host(up.get_decompressed()), edited)
        # interleaved pixels: split on the device, the planes truncated there
        hwc = np.ascontiguousarray(np.moveaxis(stack, 0, -1))
        src = A.dev(hwc)
        fi = ci.DeviceImage.from_interleaved(src, mantissa_bits=m, **kw(dtype))
        assert fi.mantissa_bits() == m and same(A.host(fi.get_decompressed()), want)
        assert same(A.host(src), hwc), "the caller's pixels were modified"
        assert ci.DeviceImage(dtype, A.dev(stack), W, H, **kw(dtype)).mantissa_bits() is None


def case_errors(ci, A):
    """ValueError before anything is compressed: integer dtypes, values outside 1 .. M"""
    ints = D.pixels(np.uint16, W, H)
    raises(ValueError, ci.DeviceChannel, A.dev(ints), W, H, mantissa_bits=5)
    raises(ValueError, ci.DeviceImage, np.uint16, A.dev(np.stack([ints, ints])), W, H, mantissa_bits=5)
    raises(ValueError, ci.DeviceImage.from_interleaved, A.dev(np.zeros((H, W, 2), np.int32)), mantissa_bits=5)
    f32, f16 = fpixels(np.float32, W, H), fpixels(np.float16, W, H)
    for bad in (0, 24, -3, 255):
        raises(ValueError, ci.DeviceChannel, A.dev(f32), W, H, mantissa_bits=bad)
        raises(ValueError, ci.DeviceImage, np.float32, A.dev(np.stack([f32, f32])), W, H, mantissa_bits=bad)
        raises(ValueError, ci.DeviceImage.from_interleaved, A.dev(np.zeros((H, W, 2), np.float32)), mantissa_bits=bad)
    raises(ValueError, ci.DeviceChannel, A.dev(f16), W, H, mantissa_bits=11)


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
