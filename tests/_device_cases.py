"""The cases of tests/test_python_device.py: DeviceChannel / DeviceImage / DeviceArray of the `compressed_image` module.

Every case takes the module `ci` and an adapter `A` that makes device arrays: `A.dev(numpy array)` -> an object with
__cuda_array_interface__, `A.host(obj)` -> numpy, `A.empty(shape, dtype)`.  On the mock backend device memory is host memory and
the adapter wraps numpy (HostCuda); on the GPU it is torch.  Run as a script -- `python _device_cases.py CASE` -- the file imports
torch FIRST (one HIP runtime in the process: torch's), loads the product module and runs CASE on torch tensors; that is how the
`gpu` parameter of the tests runs, in a process of its own.
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.uint8, np.uint16, np.float16, np.float32, np.int32]
REGIONS = [(0, 0, 1, 1), (5, 3, 1, 1), (0, 0, 300, 1), (0, 0, 300, 90), (290, 89, 10, 1), (17, 4, 71, 60), (299, 0, 1, 90),
           (3, 30, 200, 7), (10, 10, 0, 5), (10, 10, 5, 0)]          # tests/test_python_windows.py's
W, H = 300, 90


class HostCuda:
    """__cuda_array_interface__ over numpy memory: what a device array is on the mock backend"""

    def __init__(self, a, strides=False, readonly=False):
        self.a, self.strides, self.readonly = a, strides, readonly

    @property
    def __cuda_array_interface__(self):
        return {"version": 2, "shape": self.a.shape, "typestr": self.a.dtype.str, "data": (self.a.ctypes.data, self.readonly),
                "strides": self.a.strides if self.strides else None}


class MockAdapter:
    name = "mock"

    def dev(self, a):
        return HostCuda(np.ascontiguousarray(a).copy())

    def empty(self, shape, dtype):
        return HostCuda(np.full(shape, 0x5A, dtype))

    def host(self, o):
        return o.a.copy() if isinstance(o, HostCuda) else o.copy_to_host()

    def noncontiguous(self, a):
        return HostCuda(np.ascontiguousarray(a)[:, ::2], strides=True)


class TorchAdapter:
    name = "gpu"

    def dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    def empty(self, shape, dtype):
        import torch
        return torch.from_numpy(np.full(shape, 0x5A, dtype)).cuda()

    def host(self, o):
        import torch
        t = o if isinstance(o, torch.Tensor) else torch.as_tensor(o, device="cuda")
        return t.cpu().numpy()

    def noncontiguous(self, a):
        return self.dev(a)[:, ::2]


def pixels(dtype, width, height, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    a = ((x // 7) * 3 + (y // 5) * 11 + rng.integers(0, 3, (height, width))) % 200
    return a.astype(dtype)


def kw(dtype):
    return dict(block_size=4096, chunk_size=W * np.dtype(dtype).itemsize * 13)


def raises(exc, fn, *a, **k):
    try:
        fn(*a, **k)
    except exc:
        return
    except Exception as e:                                    # noqa: BLE001
        raise AssertionError("%s raised %r, expected %s" % (fn, e, exc)) from e
    raise AssertionError("%s did not raise %s" % (fn, exc))


def codecs(ci):
    return (ci.Codec.lz4, ci.Codec.blosclz, ci.Codec.zstd)


def case_channel_pixels_and_regions(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        for codec in codecs(ci):
            ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=codec, **kw(dtype))
            assert ch.shape == (H, W) and ch.dtype == np.dtype(dtype) and ch.width == W and ch.height == H
            got = ch.get_decompressed()
            assert isinstance(got, ci.DeviceArray) and got.shape == (H, W) and got.dtype == np.dtype(dtype)
            assert got.__cuda_array_interface__["version"] == 2 and got.__cuda_array_interface__["typestr"] == np.dtype(dtype).str
            assert np.array_equal(A.host(got), arr), (dtype, codec)
            out = A.empty((H, W), dtype)
            assert ch.get_decompressed(out=out) is out and np.array_equal(A.host(out), arr)
            for i, (x, y, w, h) in enumerate(REGIONS):
                if i % 2:
                    out = A.empty((h, w), dtype)
                    r = ch.get_region(x, y, w, h, out=out)
                    assert r is out
                else:
                    r = ch.get_region(x, y, w, h)
                    assert r.shape == (h, w)
                assert np.array_equal(A.host(r), arr[y:y + h, x:x + w]), (dtype, codec, x, y, w, h)
            # same chunking and, for the codecs whose bytes are the CPU codec's, the same chunks as the host class
            host = ci.Channel(arr, W, H, compression_codec=codec, **kw(dtype))
            assert (ch.num_chunks(), ch.chunk_size(), ch.chunk_elems(), ch.block_size()) == (host.num_chunks(), host.chunk_size(), host.chunk_elems(), host.block_size())
            assert ch.chunk_size(ch.num_chunks() - 1) == host.chunk_size(host.num_chunks() - 1)
            assert ch.compressed_bytes() == host.compressed_bytes() and ch.uncompressed_size() == host.uncompressed_size()
            assert ch.compression() == codec and ch.compression_level() == 9
            # packed: 64-byte slots of exactly the chunks' sizes, and less than the pixels
            assert ch.device_bytes() == sum((ch.compressed_bytes(i) + 63) // 64 * 64 for i in range(ch.num_chunks()))
            assert sum(ch.compressed_bytes(i) for i in range(ch.num_chunks())) == ch.compressed_bytes()
            # ... and less than the pixels where they compress (the same picture without its noise)
            y, x = np.mgrid[0:H, 0:W]
            smooth = ci.DeviceChannel(A.dev((((x // 7) * 3 + (y // 5) * 11) % 200).astype(dtype)), W, H, compression_codec=codec, **kw(dtype))
            assert smooth.device_bytes() < smooth.uncompressed_size() * np.dtype(dtype).itemsize, (dtype, codec)


def case_channel_set_region(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H)
        for codec in codecs(ci):
            ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=codec, **kw(dtype))
            edited = arr.copy()
            for k, (x, y, w, h) in enumerate([(17, 4, 71, 60), (0, 0, 300, 1), (299, 0, 1, 90), (10, 10, 0, 5)]):
                patch = pixels(dtype, w, h, seed=30 + k) if w and h else np.zeros((h, w), dtype)
                ch.set_region(x, y, A.dev(patch))
                edited[y:y + h, x:x + w] = patch
                assert np.array_equal(A.host(ch.get_decompressed()), edited), (dtype, codec, x, y, w, h)
            back = ch.to_channel()
            assert np.array_equal(back.get_decompressed(), edited)
            assert ch.device_bytes() == sum((ch.compressed_bytes(i) + 63) // 64 * 64 for i in range(ch.num_chunks()))
            if codec != ci.Codec.zstd:
                want = ci.Channel(edited, W, H, compression_codec=codec, **kw(dtype))
                assert back.compressed_bytes() == want.compressed_bytes() == ch.compressed_bytes(), (dtype, codec)


def case_channel_host_round_trip(ci, A):
    for dtype in DTYPES:
        arr = pixels(dtype, W, H, seed=2)
        for codec in codecs(ci):
            host = ci.Channel(arr, W, H, compression_codec=codec, **kw(dtype))
            dev = ci.DeviceChannel.from_channel(host)
            assert dev.compressed_bytes() == host.compressed_bytes() and dev.num_chunks() == host.num_chunks()
            assert np.array_equal(A.host(dev.get_decompressed()), arr)
            down = dev.to_channel()
            assert down.compressed_bytes() == host.compressed_bytes() and np.array_equal(down.get_decompressed(), arr)
            assert down.compression() == codec and down.chunk_size() == host.chunk_size()
        lazy = ci.Channel.full(dtype, 7, W, H, **kw(dtype))
        dev = ci.DeviceChannel.from_channel(lazy)
        assert np.array_equal(A.host(dev.get_decompressed()), np.full((H, W), 7, dtype))
        assert np.array_equal(A.host(dev.get_region(290, 85, 10, 5)), np.full((5, 10), 7, dtype))


def case_image(ci, A):
    for dtype in (np.uint8, np.float16, np.float32):
        planes = [pixels(dtype, W, H, seed=10 + c) for c in range(3)]
        stack = np.stack(planes)
        for codec in codecs(ci):
            for channels in ([A.dev(p) for p in planes], A.dev(stack)):
                img = ci.DeviceImage(dtype, channels, W, H, channel_names=["R", "G", "B"], compression_codec=codec, **kw(dtype))
                assert len(img) == 3 and img.shape == (3, H, W) and img.dtype == np.dtype(dtype) and img.num_channels == 3
                assert img.get_channel_names() == ["R", "G", "B"] and img.get_channel_index("B") == 2
                assert np.array_equal(A.host(img.get_decompressed()), stack)
            out = A.empty((3, H, W), dtype)
            assert img.get_decompressed(out=out) is out and np.array_equal(A.host(out), stack)
            host = ci.Image(dtype, planes, W, H, compression_codec=codec, **kw(dtype))
            assert img.compressed_bytes() == sum(c.compressed_bytes() for c in host.channels())
            for (x, y, w, h) in REGIONS:
                r = A.host(img.get_region(x, y, w, h))
                assert r.shape == (3, h, w) and np.array_equal(r, stack[:, y:y + h, x:x + w]), (dtype, codec, x, y, w, h)
                q = A.host(img.get_region(x, y, w, h, interleaved=True))
                assert q.shape == (h, w, 3) and np.array_equal(q, np.moveaxis(stack[:, y:y + h, x:x + w], 0, -1)), (dtype, codec, x, y, w, h)
            out = A.empty((60, 71, 3), dtype)
            assert img.get_region(17, 4, 71, 60, out=out, interleaved=True) is out
            assert np.array_equal(A.host(out), np.moveaxis(stack[:, 4:64, 17:88], 0, -1))
            # channel handles share the store and are read-only
            g = img["G"]
            assert g.read_only() and g.device_bytes() == img.device_bytes() and np.array_equal(A.host(g.get_decompressed()), planes[1])
            assert np.array_equal(A.host(img.channel(2).get_region(3, 30, 200, 7)), planes[2][30:37, 3:203])
            raises(RuntimeError, g.set_region, 0, 0, A.dev(planes[0][:4, :4]))
            raises(IndexError, img.channel, 3)
            raises(ValueError, img.channel, "Z")
            # edits go through the image
            patch = np.stack([pixels(dtype, 120, 33, seed=50 + c) for c in range(3)])
            img.set_region(40, 20, A.dev(patch))
            edited = stack.copy()
            edited[:, 20:53, 40:160] = patch
            assert np.array_equal(A.host(img.get_decompressed()), edited)
            assert np.array_equal(A.host(g.get_decompressed()), planes[1])          # the earlier handle keeps its store
            down = img.to_image()
            assert np.array_equal(down.get_decompressed(), edited) and down.get_channel_names() == ["R", "G", "B"]
            up = ci.DeviceImage.from_image(down)
            assert up.compressed_bytes() == img.compressed_bytes() and up.device_bytes() == img.device_bytes()
            assert np.array_equal(A.host(up.get_decompressed()), edited)
            if codec != ci.Codec.zstd:
                want = ci.Image(dtype, list(edited), W, H, compression_codec=codec, **kw(dtype))
                assert img.compressed_bytes() == sum(c.compressed_bytes() for c in want.channels())
            hwc = np.ascontiguousarray(np.moveaxis(stack, 0, -1))
            fi = ci.DeviceImage.from_interleaved(A.dev(hwc), compression_codec=codec, **kw(dtype))
            assert fi.shape == (3, H, W) and np.array_equal(A.host(fi.get_decompressed()), stack)
            assert np.array_equal(A.host(fi.get_region(0, 0, W, H, interleaved=True)), hwc)


def case_bad_arguments(ci, A):
    arr = pixels(np.uint16, W, H)
    raises(TypeError, ci.DeviceChannel, arr, W, H)                                   # numpy is host memory
    raises(TypeError, ci.DeviceChannel, [1, 2, 3], W, H)
    raises(ValueError, ci.DeviceChannel, A.noncontiguous(arr), W // 2, H)
    raises(ValueError, ci.DeviceChannel, A.dev(arr), W + 1, H)
    raises(ValueError, ci.DeviceChannel, A.dev(arr.astype(np.complex64)), W, H)       # no such element type
    ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(np.uint16))
    raises(TypeError, ch.get_decompressed, out=np.empty((H, W), np.uint16))
    raises(TypeError, ch.get_decompressed, out=A.empty((H, W), np.int16))
    raises(ValueError, ch.get_decompressed, out=A.empty((H, W + 1), np.uint16))
    raises(ValueError, ch.get_decompressed, out=A.noncontiguous(np.zeros((H, 2 * W), np.uint16)))
    raises(ValueError, ch.get_region, 0, 0, 10, 10, out=A.empty((10, 11), np.uint16))
    raises(TypeError, ch.get_region, 0, 0, 10, 10, out=A.empty((10, 10), np.float16))
    raises(TypeError, ch.set_region, 0, 0, arr[:4, :4])
    raises(ValueError, ch.set_region, 0, 0, A.dev(arr[:4, :4].astype(np.int16)))
    raises(ValueError, ch.set_region, 0, 0, A.dev(arr.ravel()[:16]))
    # bad regions: what Channel.get_region raises
    host = ci.Channel(arr, W, H, **kw(np.uint16))
    for region in [(W, 0, 1, 1), (0, H, 1, 1), (W - 5, 0, 6, 1), (0, 0, W, H + 1), (-1, 0, 1, 1), (0, 0, -1, 1)]:
        try:
            host.get_region(*region)
            raise AssertionError("the host class accepts %r" % (region,))
        except (IndexError, ValueError) as e:
            raises(type(e), ch.get_region, *region)
    raises(IndexError, ch.set_region, W - 2, 0, A.dev(arr[:4, :4]))
    planes = [A.dev(arr), A.dev(arr)]
    raises(ValueError, ci.DeviceImage, np.float32, planes, W, H)                      # dtype of the channels
    raises(TypeError, ci.DeviceImage, np.uint16, [arr, arr], W, H)
    raises(ValueError, ci.DeviceImage, np.uint16, planes, W, H + 1)
    img = ci.DeviceImage(np.uint16, planes, W, H, **kw(np.uint16))
    raises(ValueError, img.get_region, 0, 0, 10, 10, out=A.empty((10, 10, 2), np.uint16))         # planar asked, pixel-shaped out
    raises(ValueError, img.get_region, 0, 0, 10, 10, out=A.empty((2, 10, 10), np.uint16), interleaved=True)
    raises(IndexError, img.get_region, W - 5, 0, 6, 1)
    raises(ValueError, img.set_region, 0, 0, A.dev(arr[:4, :4]))
    raises(ValueError, img.set_channel_names, ["one"])
    assert np.array_equal(A.host(ch.get_decompressed()), arr)                         # nothing above changed or broke anything


# ---- GPU only: torch streams, zero-copy results, the headline geometry ----------------------------------------------------
def case_gpu_stream_and_zero_copy(ci, A):
    import torch
    side = torch.cuda.Stream()
    n = 4096
    with torch.cuda.stream(side):
        t = torch.zeros((n, n), dtype=torch.int16, device="cuda")
        for _ in range(20):                                  # queued work: an unordered read would see an earlier value
            t += 3
    ch = ci.DeviceChannel(t, n, n, stream=side.cuda_stream)
    side.synchronize()
    r = ch.get_decompressed()
    wrapped = torch.as_tensor(r, device="cuda")
    assert wrapped.data_ptr() == r.__cuda_array_interface__["data"][0], "torch copied the result"
    assert wrapped.shape == (n, n) and wrapped.dtype == torch.int16 and bool((wrapped == 60).all())
    with torch.cuda.stream(side):
        patch = torch.full((100, 200), 7, dtype=torch.int16, device="cuda") + 1
    ch.set_region(50, 60, patch, stream=side.cuda_stream)
    out = torch.empty((100, 200), dtype=torch.int16, device="cuda")
    ch.get_region(50, 60, 200, 100, out=out, stream=torch.cuda.current_stream().cuda_stream)
    assert bool((out == 8).all())
    del r
    assert bool((wrapped == 60).all())                       # the tensor keeps the DeviceArray's memory alive
    raises(TypeError, ci.DeviceChannel, torch.zeros((4, 4)), 4, 4)                     # a CPU tensor is host memory


def case_gpu_headline_geometry(ci, A):
    import torch
    from cimg import synth
    n = 4096
    planes = np.stack([synth.tiled_channel(np.float16, n, n) for _ in range(4)])
    planes[1] = planes[1][::-1]
    t = torch.from_numpy(planes.view(np.int16)).cuda().view(torch.float16)
    img = ci.DeviceImage(np.float16, t, n, n)
    assert img.device_bytes() < img.uncompressed_size() * 2 and img.num_chunks() == 4 * 8
    out = torch.empty_like(t)
    img.get_decompressed(out=out)
    assert torch.equal(out.view(torch.int16), t.view(torch.int16))
    crop = torch.as_tensor(img.get_region(1000, 2000, 512, 256, interleaved=True), device="cuda")
    assert torch.equal(crop.view(torch.int16), t[:, 2000:2256, 1000:1512].permute(1, 2, 0).contiguous().view(torch.int16))


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}


def load_module(backend):
    import importlib.util
    import sysconfig
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    path = os.path.join(ROOT, "tests", "emu" if backend == "mock" else os.path.join("..", "compressed-image_amd"), "compressed_image" + ext)
    path = os.path.normpath(path)
    assert os.path.exists(path), path + " is missing: run __graft_entry__.build()"
    spec = importlib.util.spec_from_file_location("compressed_image", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]
    CASES[sys.argv[1]](load_module("gpu"), TorchAdapter())
    print("case %s ok" % sys.argv[1])
