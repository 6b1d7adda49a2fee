"""The cases of tests/test_python_special.py and tests/test_gpu_special_chunks.py: DeviceChannel.full / zeros / full_like / zeros_like --
blank channels made of blosc2 special-value chunks -- in the pattern of tests/_device_cases.py (whose adapters they use).  Run as a
script -- `python _device_cases_special.py CASE` -- the file imports torch FIRST, loads the product module and runs CASE on torch
tensors in a process of its own.  Expectations are np.full and numpy edits of it."""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import raises

W, H = 300, 90
ROWS = 13                                                     # scanlines a chunk: 7 chunks, the last one short
FILLS = [(np.uint8, 7), (np.uint16, 0x1234), (np.float16, 1.5), (np.float32, -2.75), (np.int32, -123456), (np.float64, 3.0e-7)]


def kw(dtype):
    return dict(block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * ROWS)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def chunk_sizes(ch):
    return [ch.compressed_bytes(i) for i in range(ch.num_chunks())]


def case_full_reads(ci, A):
    for dtype, fill in FILLS:
        it = np.dtype(dtype).itemsize
        want = np.full((H, W), fill, dtype)
        for codec in D.codecs(ci):
            ch = ci.DeviceChannel.full(dtype, fill, W, H, compression_codec=codec, **kw(dtype))
            assert ch.shape == (H, W) and ch.dtype == np.dtype(dtype) and ch.num_chunks() == (H + ROWS - 1) // ROWS
            assert ch.compression() == codec and ch.compression_level() == 9 and ch.block_size() == 4096
            assert chunk_sizes(ch) == [32 + it] * ch.num_chunks()
            assert ch.device_bytes() == 64 * ch.num_chunks()
            assert same(A.host(ch.get_decompressed()), want), (dtype, codec)
            out = A.empty((H, W), dtype)
            assert ch.get_decompressed(out=out) is out and same(A.host(out), want)
            for (x, y, w, h) in D.REGIONS:
                assert same(A.host(ch.get_region(x, y, w, h)), want[y:y + h, x:x + w]), (dtype, x, y, w, h)
            assert same(A.host(ch[10:80:7, 5:290:11]), want[10:80:7, 5:290:11])
            assert same(A.host(ch.get_regions([0, 100, 250], [0, 40, 77], 50, 13)), np.stack([want[y:y + 13, x:x + 50] for x, y in ((0, 0), (100, 40), (250, 77))]))
            xs, ys = np.array([0, 299, 17, 150]), np.array([0, 89, 45, 13])
            assert same(A.host(ch.get_pixels(xs, ys)), want[ys, xs])
    # zeros: special-zero chunks, 32 bytes each; so is a fill whose bytes are all zero
    for make in (lambda: ci.DeviceChannel.zeros(np.float32, W, H, **kw(np.float32)), lambda: ci.DeviceChannel.full(np.float32, 0.0, W, H, **kw(np.float32))):
        z = make()
        assert chunk_sizes(z) == [32] * z.num_chunks() and z.device_bytes() == 64 * z.num_chunks()
        assert same(A.host(z.get_decompressed()), np.zeros((H, W), np.float32))
    # -0.0 is a value, not zero bytes
    m = ci.DeviceChannel.full(np.float32, -0.0, W, H, **kw(np.float32))
    assert chunk_sizes(m) == [36] * m.num_chunks() and same(A.host(m.get_decompressed()), np.full((H, W), -0.0, np.float32))
    # *_like: geometry and codec parameters of the other channel
    src = ci.DeviceChannel(A.dev(D.pixels(np.uint16, W, H)), W, H, compression_codec=ci.Codec.blosclz, compression_level=5, **kw(np.uint16))
    for like, fill in ((ci.DeviceChannel.full_like(src, 999), 999), (ci.DeviceChannel.zeros_like(src), 0)):
        assert (like.shape, like.dtype, like.num_chunks(), like.chunk_size(), like.block_size()) == (src.shape, src.dtype, src.num_chunks(), src.chunk_size(), src.block_size())
        assert like.compression() == ci.Codec.blosclz and like.compression_level() == 5
        assert like.device_bytes() == 64 * like.num_chunks()
        assert same(A.host(like.get_decompressed()), np.full((H, W), fill, np.uint16))
    raises(ValueError, ci.DeviceChannel.full, np.float32, 1.0, 0, 5)
    raises(ValueError, ci.DeviceChannel.full, np.int32, 1, W, H, mantissa_bits=5)


def case_full_set_region(ci, A):
    for dtype, fill in FILLS[:5]:
        it = np.dtype(dtype).itemsize
        for codec in D.codecs(ci):
            ch = ci.DeviceChannel.full(dtype, fill, W, H, compression_codec=codec, **kw(dtype))
            want = np.full((H, W), fill, dtype)
            # rows 20 .. 32 lie in chunks 1 and 2 (13 scanlines a chunk)
            patch = D.pixels(dtype, 71, 13, seed=5)
            ch.set_region(17, 20, A.dev(patch))
            want[20:33, 17:88] = patch
            sizes = chunk_sizes(ch)
            assert [i for i, s in enumerate(sizes) if s != 32 + it] == [1, 2], sizes
            assert same(A.host(ch.get_decompressed()), want), (dtype, codec)
            assert same(A.host(ch.get_region(0, 15, 300, 30)), want[15:45])
            # the touched chunks are what a channel compressed from the edited pixels holds
            ref = ci.DeviceChannel(A.dev(want), W, H, compression_codec=codec, **kw(dtype))
            if codec != ci.Codec.zstd:
                assert sizes[1] == ref.compressed_bytes(1) and sizes[2] == ref.compressed_bytes(2)
            # writing the fill value back over an edited chunk does not bring the special chunk back, and the pixels are right
            ch.set_region(0, 13, A.dev(np.full((13, W), fill, dtype)))
            want[13:26] = fill
            assert same(A.host(ch.get_decompressed()), want)


def case_full_host_round_trip(ci, A):
    dtype, fill = np.float32, 6.25
    want = np.full((H, W), fill, dtype)
    ch = ci.DeviceChannel.full(dtype, fill, W, H, **kw(dtype))
    host = ch.to_channel()
    assert isinstance(host, ci.Channel) and host.shape == (H, W) and host.num_chunks() == ch.num_chunks()
    assert host.compressed_bytes() == 36 * ch.num_chunks()                      # the special chunks, handed over as they are
    assert same(host.get_decompressed(), want)
    assert same(host.get_region(17, 4, 71, 60), want[4:64, 17:88])
    back = ci.DeviceChannel.from_channel(host)
    assert back.device_bytes() == 64 * back.num_chunks() and same(A.host(back.get_decompressed()), want)
    # (inside a DeviceImage: tests/cpp/special_channel_test.cpp -- the Python Image has no constructor over finished channels)


def case_full_mantissa(ci, A):
    from _device_cases_trunc import trunc
    for dtype, fill, m in ((np.float32, np.pi, 8), (np.float16, 1.2345, 3), (np.float64, np.e, 20)):
        want = trunc(np.full((H, W), fill, dtype), m)
        assert not same(want, np.full((H, W), fill, dtype))
        ch = ci.DeviceChannel.full(dtype, fill, W, H, mantissa_bits=m, **kw(dtype))
        assert ch.mantissa_bits() == m and ch.device_bytes() == 64 * ch.num_chunks()
        assert same(A.host(ch.get_decompressed()), want), dtype
        assert same(A.host(ch.get_region(3, 30, 200, 7)), want[30:37, 3:203])
        like = ci.DeviceChannel.full_like(ch, fill)
        assert like.mantissa_bits() == m and same(A.host(like.get_decompressed()), want)


def case_gpu_full_set_region(ci, A):
    """one DeviceChannel.full -> set_region -> get_decompressed on the GPU"""
    dtype, fill = np.float32, -2.75
    ch = ci.DeviceChannel.full(dtype, fill, W, H, **kw(dtype))
    assert ch.device_bytes() == 64 * ch.num_chunks()
    want = np.full((H, W), fill, dtype)
    assert same(A.host(ch.get_decompressed()), want)
    patch = D.pixels(dtype, 71, 13, seed=5)
    ch.set_region(17, 20, A.dev(patch))
    want[20:33, 17:88] = patch
    assert [i for i, s in enumerate(chunk_sizes(ch)) if s != 36] == [1, 2]
    assert same(A.host(ch.get_decompressed()), want)
    assert same(A.host(ch.get_region(10, 10, 100, 40)), want[10:50, 10:110])
    assert same(A.host(ch[0:90:3, 0:300:5]), want[0:90:3, 0:300:5])
    assert same(ch.to_channel().get_decompressed(), want)


CASES = {n[5:]: f for n, f in list(globals().items()) if n.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
