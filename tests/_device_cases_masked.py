"""The device-class cases of tests/test_python_window_writes_masked.py: DeviceChannel.fill_region / fill_regions and mask= / masks= of
set_region / set_regions, in the pattern of tests/_device_cases.py (whose adapters they use).  Run as a script -- `python
_device_cases_masked.py CASE` -- the file imports torch FIRST and runs CASE on torch tensors with the product module, in a process
of its own; on the mock backend the test calls the cases directly.  The plane is 512 x 130 in chunks of 30 rows.  The expectation is
numpy's: np.copyto(view, src_or_value, where=mask) into a copy of the pixels, compared bit for bit; and the compressed size of the
edited channel equals that of a channel constructed from the edited pixels.
"""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first)

import numpy as np

import _device_cases as D
from _device_cases import raises
from _device_cases_grouped import H, W, kw
from _device_cases_typed import pixels

STORED = [np.uint8, np.uint16, np.float16, np.float32]
# (x, y, width, height, step_x, step_y): over chunk boundaries, subsampled, whole rows (whole blocks for a fill), the last element
REGIONS = [(17, 4, 71, 60, 1, 1), (3, 25, 301, 40, 3, 5), (0, 40, W, 50, 1, 1), (W - 1, H - 1, 1, 1, 4, 4), (0, 0, W, H, 16, 16)]


def masks_of(shape, seed):
    """bool and uint8 masks in turn: random 50 %, with the values 2 and 255 among the set bytes of the uint8 ones"""
    rng = np.random.default_rng(seed)
    m = rng.random(shape) < 0.5
    if seed & 1:
        return m
    return (m * rng.choice(np.array([1, 2, 255], np.uint8), shape)).astype(np.uint8)


def same(got, exp):
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
    return got.shape == exp.shape and got.dtype == exp.dtype and bool((np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(exp).view(bits)).all())


def fresh_size(ci, A, dtype, arr):
    return ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype)).compressed_bytes()


def case_channel_fill_and_masked_writes(ci, A):
    for dtype in STORED:
        arr = pixels(dtype)
        ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(dtype))
        edited = arr.copy()
        for k, (x, y, w, h, sx, sy) in enumerate(REGIONS):
            shape = (-(-h // sy), -(-w // sx))
            view = edited[y:y + h:sy, x:x + w:sx]
            value = np.dtype(dtype).type(3 + k)
            ch.fill_region(x, y, w, h, 3 + k, step_x=sx, step_y=sy)
            np.copyto(view, value)
            assert same(A.host(ch.get_decompressed()), edited), (dtype, "fill", k)
            m = masks_of(shape, 20 + k)
            ch.fill_region(x, y, w, h, 100 + k, step_x=sx, step_y=sy, mask=A.dev(m))
            np.copyto(view, np.dtype(dtype).type(100 + k), where=m != 0)
            assert same(A.host(ch.get_decompressed()), edited), (dtype, "masked fill", k)
            v = pixels(dtype, 30 + k).ravel()[:shape[0] * shape[1]].reshape(shape)
            m = masks_of(shape, 41 + k)
            ch.set_region(x, y, A.dev(v), step_x=sx, step_y=sy, mask=A.dev(m))
            np.copyto(view, v, where=m != 0)
            assert same(A.host(ch.get_decompressed()), edited), (dtype, "masked set", k)
        # batches: the last region lies on the first and wins where its mask is set
        xs, ys, w, h, sx, sy = [5, 140, 300, 5], [10, 60, 100, 10], 90, 28, 2, 1
        shape = (4, -(-h // sy), -(-w // sx))
        vals = [7, 8, 9, 10]
        ch.fill_regions(xs, ys, w, h, vals, step_x=sx, step_y=sy)
        for x, y, c in zip(xs, ys, vals):
            np.copyto(edited[y:y + h:sy, x:x + w:sx], np.dtype(dtype).type(c))
        assert same(A.host(ch.get_decompressed()), edited), (dtype, "fill_regions")
        m = masks_of(shape, 50)
        ch.fill_regions(xs, ys, w, h, 55, step_x=sx, step_y=sy, masks=A.dev(m))
        for k, (x, y) in enumerate(zip(xs, ys)):
            np.copyto(edited[y:y + h:sy, x:x + w:sx], np.dtype(dtype).type(55), where=m[k] != 0)
        assert same(A.host(ch.get_decompressed()), edited), (dtype, "masked fill_regions")
        v = pixels(dtype, 60).ravel()[:int(np.prod(shape))].reshape(shape)
        m = masks_of(shape, 61)
        ch.set_regions(xs, ys, A.dev(v), step_x=sx, step_y=sy, masks=A.dev(m))
        for k, (x, y) in enumerate(zip(xs, ys)):
            np.copyto(edited[y:y + h:sy, x:x + w:sx], v[k], where=m[k] != 0)
        assert same(A.host(ch.get_decompressed()), edited), (dtype, "masked set_regions")
        assert ch.compressed_bytes() == fresh_size(ci, A, dtype, edited), dtype
        # an all-zero mask changes nothing, not even the size
        before = ch.compressed_bytes()
        ch.fill_region(0, 0, W, H, 1, mask=A.dev(np.zeros((H, W), np.uint8)))
        assert same(A.host(ch.get_decompressed()), edited) and ch.compressed_bytes() == before
        # a whole-plane fill
        ch.fill_region(0, 0, W, H, 42)
        assert same(A.host(ch.get_decompressed()), np.full((H, W), 42, dtype))
        assert ch.compressed_bytes() == fresh_size(ci, A, dtype, np.full((H, W), 42, dtype))


def case_blank_channel(ci, A):
    """full / zeros channels (special-value chunks): a fill and a masked write make the chunks they meet real"""
    for dtype in (np.uint8, np.float32):
        ch = ci.DeviceChannel.full(dtype, 5, W, H, **kw(dtype))
        edited = np.full((H, W), 5, dtype)
        ch.fill_region(10, 20, 100, 50, 9, step_x=3)
        edited[20:70, 10:110:3] = 9
        m = masks_of((30, 200), 3)
        v = pixels(dtype, 4)[:30, :200]
        ch.set_region(300, 95, A.dev(v), mask=A.dev(m))
        np.copyto(edited[95:125, 300:500], v, where=m != 0)
        assert same(A.host(ch.get_decompressed()), edited), dtype


def case_masked_errors(ci, A):
    arr = pixels(np.uint8)
    ch = ci.DeviceChannel(A.dev(arr), W, H, **kw(np.uint8))
    v, m = A.dev(np.zeros((4, 6), np.uint8)), A.dev(np.ones((4, 6), np.uint8))
    raises(ValueError, ch.set_region, 0, 0, v, mask=A.dev(np.ones((4, 6), np.float32)))           # dtype
    raises(ValueError, ch.set_region, 0, 0, v, mask=A.dev(np.ones((4, 6), np.int8)))
    raises(ValueError, ch.set_region, 0, 0, v, mask=A.dev(np.ones((4, 5), np.uint8)))             # shape
    raises(ValueError, ch.set_region, 0, 0, v, mask=A.dev(np.ones((24,), np.uint8)))
    raises(ValueError, ch.set_region, 0, 0, A.dev(np.zeros((4, 6), np.float32)), dtype=np.float32, mask=m)   # masked typed writes: out of scope
    raises(ValueError, ch.set_regions, [0], [0], A.dev(np.zeros((1, 4, 6), np.float32)), dtype=np.float32, masks=A.dev(np.ones((1, 4, 6), np.uint8)))
    raises(ValueError, ch.set_regions, [0, 9], [0, 9], A.dev(np.zeros((2, 4, 6), np.uint8)), masks=A.dev(np.ones((1, 4, 6), np.uint8)))
    raises(IndexError, ch.set_region, W - 5, 0, v, mask=m)
    raises(IndexError, ch.fill_region, 0, H - 3, 4, 4, 1)
    raises(IndexError, ch.fill_regions, [0, W - 3], [0, 0], 4, 4, 1)
    raises(ValueError, ch.fill_region, 0, 0, 4, 6, 1, mask=A.dev(np.ones((4, 6), np.uint8)))                   # (height, width) is (6, 4)
    raises(ValueError, ch.fill_region, 0, 0, 8, 6, 1, step_x=2, mask=A.dev(np.ones((6, 8), np.uint8)))        # the subsampled shape is (6, 4)
    raises(ValueError, ch.fill_regions, [0, 9], [0, 9], 4, 4, [1, 2, 3])
    raises(ValueError, ch.fill_regions, [0, 9], [0, 9], 4, 4, 1, masks=A.dev(np.ones((4, 4), np.uint8)))
    raises(ValueError, ch.fill_region, 0, 0, 4, 4, 1, step_x=0)
    raises(TypeError, ch.fill_region, 0, 0, 4, 6, 1, mask=np.ones((6, 4), np.uint8))               # host memory
    assert np.array_equal(A.host(ch.get_decompressed()), arr), "a refused call changed the channel"
    raises(TypeError, ch.__setitem__, (slice(0, 4), slice(0, 4)), 3)                               # __setitem__ is untouched: no scalars
    ch.fill_region(0, 0, 0, 0, 1)                                                                  # nothing to do
    ch.fill_regions([], [], 4, 4, 1)
    assert np.array_equal(A.host(ch.get_decompressed()), arr)


def _host_writes(dtype, k):
    """the writes every class runs: (kind, x, y, w, h, sx, sy) -- over chunk boundaries, subsampled, whole rows"""
    return [(17, 4, 71, 60, 1, 1), (3, 25, 301, 40, 3, 5), (0, 40, W, 50, 1, 1), (W - 1, H - 1, 1, 1, 4, 4)]


def case_host_channel(ci, A):
    """Channel: numpy arrays and numpy masks; full / zeros chunks a region meets become real"""
    for dtype in STORED:
        for lazy in (False, True):
            arr = np.full((H, W), 5, dtype) if lazy else pixels(dtype)
            ch = ci.Channel.full(dtype, 5, W, H, **kw(dtype)) if lazy else ci.Channel(arr, W, H, **kw(dtype))
            edited = arr.copy()
            for k, (x, y, w, h, sx, sy) in enumerate(_host_writes(dtype, 0)):
                shape = (-(-h // sy), -(-w // sx))
                view = edited[y:y + h:sy, x:x + w:sx]
                ch.fill_region(x, y, w, h, 3 + k, step_x=sx, step_y=sy)
                np.copyto(view, np.dtype(dtype).type(3 + k))
                m = masks_of(shape, 20 + k)
                ch.fill_region(x, y, w, h, np.int64(100 + k), step_x=sx, step_y=sy, mask=m)         # (a numpy scalar is a number)
                np.copyto(view, np.dtype(dtype).type(100 + k), where=m != 0)
                v = pixels(dtype, 30 + k).ravel()[:shape[0] * shape[1]].reshape(shape)
                m = masks_of(shape, 41 + k)
                ch.set_region(x, y, v, step_x=sx, step_y=sy, mask=m)
                np.copyto(view, v, where=m != 0)
                assert same(ch.get_decompressed(), edited), (dtype, lazy, k)
            xs, ys, w, h, sx, sy = [5, 140, 300, 5], [10, 60, 100, 10], 90, 28, 2, 1
            shape = (4, -(-h // sy), -(-w // sx))
            ch.fill_regions(xs, ys, w, h, [7, 8, 9, 10], step_x=sx, step_y=sy)
            for x, y, c in zip(xs, ys, [7, 8, 9, 10]):
                np.copyto(edited[y:y + h:sy, x:x + w:sx], np.dtype(dtype).type(c))
            m = masks_of(shape, 50)
            ch.fill_regions(xs, ys, w, h, np.array(55), step_x=sx, step_y=sy, masks=m)             # (a 0-d array is a number)
            v = pixels(dtype, 60).ravel()[:int(np.prod(shape))].reshape(shape)
            m2 = masks_of(shape, 61)
            ch.set_regions(xs, ys, v, step_x=sx, step_y=sy, masks=m2)
            for k, (x, y) in enumerate(zip(xs, ys)):
                np.copyto(edited[y:y + h:sy, x:x + w:sx], np.dtype(dtype).type(55), where=m[k] != 0)
            for k, (x, y) in enumerate(zip(xs, ys)):
                np.copyto(edited[y:y + h:sy, x:x + w:sx], v[k], where=m2[k] != 0)
            assert same(ch.get_decompressed(), edited), (dtype, lazy, "batches")
            if not lazy:
                assert ch.compressed_bytes() == ci.Channel(edited, W, H, **kw(dtype)).compressed_bytes(), dtype


def _image_case(ci, A, device):
    C = 3
    for dtype in (np.uint8, np.float32):
        planes = np.stack([pixels(dtype, seed=s) for s in range(C)])
        if device:
            img = ci.DeviceImage(dtype, A.dev(planes), W, H, **kw(dtype))
            dev = A.dev
            decoded = lambda: A.host(img.get_decompressed())                                       # noqa: E731
        else:
            img = ci.Image(dtype, list(planes), W, H, ["r", "g", "b"], **kw(dtype))
            dev = lambda a: a                                                                      # noqa: E731
            decoded = lambda: np.asarray(img.get_decompressed())                                   # noqa: E731
        edited = planes.copy()
        for k, (x, y, w, h, sx, sy) in enumerate(_host_writes(dtype, 0)):
            shape = (-(-h // sy), -(-w // sx))
            view = edited[:, y:y + h:sy, x:x + w:sx]
            img.fill_region(x, y, w, h, 9 + k, step_x=sx, step_y=sy)                               # one value for all channels
            np.copyto(view, np.dtype(dtype).type(9 + k))
            vals = [20 + k, 30 + k, 40 + k]
            m = masks_of(shape, 70 + k)
            img.fill_region(x, y, w, h, vals, step_x=sx, step_y=sy, mask=dev(m))                   # one value a channel, ONE mask
            np.copyto(view, np.array(vals, dtype).reshape(C, 1, 1), where=(m != 0)[None])
            v = np.stack([pixels(dtype, 80 + k + c).ravel()[:shape[0] * shape[1]].reshape(shape) for c in range(C)])
            m = masks_of(shape, 91 + k)
            img.set_region(x, y, dev(v) if device else list(v), step_x=sx, step_y=sy, mask=dev(m))
            np.copyto(view, v, where=(m != 0)[None])
            assert same(decoded(), edited), (dtype, device, k)
        xs, ys, w, h, sx, sy = [5, 140, 300, 5], [10, 60, 100, 10], 90, 28, 2, 1
        shape = (4, -(-h // sy), -(-w // sx))
        m = masks_of(shape, 50)
        img.fill_regions(xs, ys, w, h, [1, 2, 3], step_x=sx, step_y=sy, masks=dev(m))
        for k, (x, y) in enumerate(zip(xs, ys)):
            np.copyto(edited[:, y:y + h:sy, x:x + w:sx], np.array([1, 2, 3], dtype).reshape(C, 1, 1), where=(m[k] != 0)[None])
        v = pixels(dtype, 60).ravel()[:4 * C * shape[1] * shape[2]].reshape(4, C, shape[1], shape[2])
        m2 = masks_of(shape, 61)
        img.set_regions(xs, ys, dev(v), step_x=sx, step_y=sy, masks=dev(m2))
        for k, (x, y) in enumerate(zip(xs, ys)):
            np.copyto(edited[:, y:y + h:sy, x:x + w:sx], v[k], where=(m2[k] != 0)[None])
        assert same(decoded(), edited), (dtype, device, "batches")
        # refusals leave the image as it was
        raises(ValueError, img.fill_region, 0, 0, 4, 4, [1, 2])                                    # two values for three channels
        raises(ValueError, img.fill_region, 0, 0, 4, 6, 1, mask=dev(np.ones((4, 6), np.uint8)))
        raises(ValueError, img.fill_region, 0, 0, 4, 6, 1, mask=dev(np.ones((6, 4), np.float32)))
        raises(ValueError, img.set_regions, [0], [0], dev(np.zeros((1, C, 4, 6), dtype)), masks=dev(np.ones((1, C, 4, 6), np.uint8)))   # the mask has no channel axis
        raises(IndexError, img.fill_region, W - 2, 0, 4, 4, 1)
        raises(IndexError, img.set_regions, [0, W - 2], [0, 0], dev(np.zeros((2, C, 4, 6), dtype)), masks=dev(np.ones((2, 4, 6), np.uint8)))
        if device:
            raises(ValueError, img.set_region, 0, 0, dev(np.zeros((C, 4, 6), np.float32)), dtype=np.float32, mask=dev(np.ones((4, 6), np.uint8)))
        assert same(decoded(), edited), (dtype, device, "after refusals")


def case_host_image(ci, A):
    _image_case(ci, A, False)


def case_device_image(ci, A):
    _image_case(ci, A, True)


def case_host_errors(ci, A):
    arr = pixels(np.uint8)
    ch = ci.Channel(arr, W, H, **kw(np.uint8))
    v, m = np.zeros((4, 6), np.uint8), np.ones((4, 6), np.uint8)
    raises(ValueError, ch.set_region, 0, 0, v, mask=np.ones((4, 6), np.float32))
    raises(ValueError, ch.set_region, 0, 0, v, mask=np.ones((4, 5), np.uint8))
    raises(ValueError, ch.set_region, 0, 0, v, mask=[[1] * 6] * 4)                                 # not an array
    raises(ValueError, ch.set_regions, [0, 9], [0, 9], np.zeros((2, 4, 6), np.uint8), masks=np.ones((1, 4, 6), np.uint8))
    raises(IndexError, ch.set_region, W - 5, 0, v, mask=m)
    raises(IndexError, ch.fill_region, 0, H - 3, 4, 4, 1)
    raises(IndexError, ch.fill_regions, [0, W - 3], [0, 0], 4, 4, 1)
    raises(ValueError, ch.fill_region, 0, 0, 4, 6, 1, mask=m)                                      # (height, width) is (6, 4)
    raises(ValueError, ch.fill_region, 0, 0, 4, 6, [1])                                            # fill_region takes one number
    raises(ValueError, ch.fill_regions, [0, 9], [0, 9], 4, 4, [1, 2, 3])
    raises(ValueError, ch.fill_region, 0, 0, 4, 4, 1, step_x=0)
    raises(ValueError, ch.fill_region, -1, 0, 4, 4, 1)
    assert np.array_equal(ch.get_decompressed(), arr), "a refused call changed the channel"
    ch.fill_region(0, 0, 0, 0, 1)
    ch.fill_regions([], [], 4, 4, 1)
    assert np.array_equal(ch.get_decompressed(), arr)


CASES = {f[len("case_"):]: g for f, g in list(globals().items()) if f.startswith("case_")}

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(D.ROOT, "compressed-image_amd"), os.path.join(D.ROOT, "tests")]
    CASES[sys.argv[1]](D.load_module("gpu"), D.TorchAdapter())
    print("case %s ok" % sys.argv[1])
