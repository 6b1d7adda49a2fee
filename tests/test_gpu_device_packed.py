"""Packed device storage on the MI355X through cimg/hip.py: cimg_compress_batch_device_packed_begin / _fetch,
cimg_pack_chunks_device (csrc/pack_kernel.h), cimg_interleave_device (csrc/interleave_kernel.h), cimg_engine_wait_stream and
cimg_device_range_check.

Device memory comes from Engine.alloc; the only host address handed to the library as a device address is the one the
range-check test passes to cimg_device_range_check, which launches nothing.
"""
import numpy as np
import pytest

import _oracle as O
from _pack import CANARY, ERR_INVALID_PARAM, INTERLEAVE_CASES, expected, grid, interleaved, layout
from cimg import hip, synth

pytestmark = pytest.mark.gpu
BLOSCLZ, LZ4, LZ4HC, ZSTD = 0, 1, 2, 5


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def plane(ts):
    """pixels that compress to very different chunk sizes: tiled, noisy and constant stretches; a short last chunk"""
    rng = np.random.default_rng(ts)
    a = synth.tiled_channel(np.float16, 512, 300).view(np.uint8).ravel().copy()
    a[100000:180000] = rng.integers(0, 256, 80000, dtype=np.uint8)
    a[200000:260000] = 7
    return a[:(a.size - 1234) // ts * ts]


def chunking(raw, chunk):
    nb = np.array([min(chunk, raw.size - o) for o in range(0, raw.size, chunk)], np.int32)
    off = np.concatenate([[0], np.cumsum(nb[:-1], dtype=np.int64)]).astype(np.int64)
    return nb, off


@pytest.mark.parametrize("codec", [LZ4, BLOSCLZ, LZ4HC, ZSTD])
@pytest.mark.parametrize("ts", [2, 4])
def test_packed_chunks_equal_the_unpacked_batch_and_the_oracle(eng, codec, ts):
    raw = plane(ts)
    chunk = 65536
    nb, roff = chunking(raw, chunk)
    dest = nb + hip.MAX_OVERHEAD
    p = hip.cparams(ts, compcode=codec, blocksize=16384)
    d_raw = eng.alloc(raw.size)
    d_raw.upload(raw)
    # the unpacked layout: chunk i at i * (chunk + overhead)
    coff = np.arange(nb.size, dtype=np.int64) * (chunk + hip.MAX_OVERHEAD)
    d_comp = eng.alloc(int(coff[-1]) + chunk + hip.MAX_OVERHEAD)
    cb_ref = eng.compress_device(p, d_raw.ptr, roff, nb, d_comp.ptr, coff, dest)
    comp = d_comp.download()
    ref = [comp[o:o + c].tobytes() for o, c in zip(coff, cb_ref)]
    # the packed one: sizes first, then an exact-size store with canaries between the chunks (64-byte slots + 16 canary bytes,
    # odd offsets so that the destinations are misaligned)
    cb = eng.compress_device_packed_begin(p, d_raw.ptr, roff, nb, dest)
    assert np.array_equal(cb, cb_ref)
    assert (cb > 0).all()
    doff = np.zeros(nb.size, np.int64)
    at = 16
    for i, c in enumerate(cb):
        doff[i] = at + (i % 3)
        at = doff[i] + int(c) + 16
    d_store = eng.alloc(at + 16)
    d_store.upload(np.full(at + 16, CANARY, np.uint8))
    eng.compress_device_packed_fetch(nb.size, d_store.ptr, doff)
    store = d_store.download()
    want = np.full(at + 16, CANARY, np.uint8)
    for o, c in zip(doff, ref):
        want[o:o + len(c)] = np.frombuffer(c, np.uint8)
    assert np.array_equal(store, want), "packed chunks differ from cimg_compress_batch_device's, or a canary was overwritten"
    assert int(cb.sum()) < raw.size                                       # packed: the store is smaller than the pixels
    if codec in (LZ4, BLOSCLZ):
        po = O.cparams(ts, compcode=codec, blocksize=16384)
        for i, (o, n) in enumerate(zip(roff, nb)):
            r, chunk_bytes = O.compress(po, raw[o:o + n], destsize=int(dest[i]))
            assert r == len(ref[i]) and chunk_bytes == ref[i], (codec, ts, i)
    # and they decode from where they were packed
    d_out = eng.alloc(raw.size)
    eng.decompress_device(d_store.ptr, doff, nb, np.minimum(nb, 16384), d_out.ptr, roff, comp_size=cb)
    assert np.array_equal(d_out.download(), raw)
    for b in (d_raw, d_comp, d_store, d_out):
        b.free()


def test_a_voided_fetch_is_an_error(eng):
    raw = plane(2)[:200000]
    nb, roff = chunking(raw, 65536)
    p = hip.cparams(2)
    d_raw = eng.alloc(raw.size)
    d_raw.upload(raw)
    d_store = eng.alloc(raw.size + 4096)
    doff = np.arange(nb.size, dtype=np.int64) * 66000
    with pytest.raises(hip.CodecError):                                   # nothing begun
        eng.compress_device_packed_fetch(nb.size, d_store.ptr, doff)
    eng.compress_device_packed_begin(p, d_raw.ptr, roff, nb, nb + 32)
    eng.compress_host(p, raw[:65536], [65536], [65536 + 32])              # reuses the staging area
    with pytest.raises(hip.CodecError) as ei:
        eng.compress_device_packed_fetch(nb.size, d_store.ptr, doff)
    assert ei.value.code == ERR_INVALID_PARAM
    cb = eng.compress_device_packed_begin(p, d_raw.ptr, roff, nb, nb + 32)
    with pytest.raises(hip.CodecError):                                   # another chunk count than was begun
        eng.compress_device_packed_fetch(nb.size + 1, d_store.ptr, np.arange(nb.size + 1, dtype=np.int64) * 66000)
    eng.compress_device_packed_fetch(nb.size, d_store.ptr, doff)          # the engine stays usable
    with pytest.raises(hip.CodecError):                                   # fetched once
        eng.compress_device_packed_fetch(nb.size, d_store.ptr, doff)
    d_out = eng.alloc(raw.size)
    eng.decompress_device(d_store.ptr, doff, nb, np.minimum(nb, 32768), d_out.ptr, roff, comp_size=cb)
    assert np.array_equal(d_out.download(), raw)
    for b in (d_raw, d_store, d_out):
        b.free()


def _pack_call(eng, cases, rng):
    so, do, nb, ssz, dsz = layout(cases)
    src = rng.integers(0, 256, ssz, dtype=np.uint8)
    d_src, d_dst = eng.alloc(ssz), eng.alloc(dsz)
    assert d_src.ptr % 16 == 0 and d_dst.ptr % 16 == 0
    d_src.upload(src)
    d_dst.upload(np.full(dsz, CANARY, np.uint8))
    eng.pack_chunks_device(d_src.ptr + so, nb, d_dst.ptr, do)
    got = d_dst.download()
    d_src.free(); d_dst.free()
    assert np.array_equal(got, expected(src, so, do, nb, dsz))


def test_pack_kernel_over_the_size_and_misalignment_grid(eng):
    rng = np.random.default_rng(21)
    cases = list(grid())
    _pack_call(eng, cases, rng)                                           # the whole grid in one launch
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 4095, 65536, 65537, (4 << 20) + 32):   # and every size as a launch of its own
        _pack_call(eng, [(n, 5, 11)], rng)
        _pack_call(eng, [(n, 0, 0)], rng)
    sizes = rng.choice([0, 1, 33, 100, 4095, 20000, 65537], 3000)
    _pack_call(eng, [(int(n), int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in sizes], rng)


def test_pack_refuses_overlapping_ranges(eng):
    d = eng.alloc(8192)
    d.upload(np.full(8192, CANARY, np.uint8))
    for srcs, sizes, dsts in (([0], [100], [50]), ([0, 1000], [100, 100], [2000, 2050]), ([0, 2000], [100, 100], [2050, 3000])):
        with pytest.raises(hip.CodecError) as ei:
            eng.pack_chunks_device(d.ptr + np.array(srcs, np.int64), sizes, d.ptr, dsts)
        assert ei.value.code == ERR_INVALID_PARAM
    assert (d.download() == CANARY).all()
    d.free()


def test_interleave_against_numpy(eng):
    rng = np.random.default_rng(22)
    for nch, ts, npix in INTERLEAVE_CASES + [(4, 2, 1 << 20), (3, 4, 333333)]:
        if npix == 0:
            continue
        planes = rng.integers(0, 256, (nch, npix * ts), dtype=np.uint8)
        stride = (npix * ts + 15) & ~15
        buf = np.full(stride * nch, CANARY, np.uint8)
        for c in range(nch):
            buf[c * stride:c * stride + npix * ts] = planes[c]
        d_in, d_out = eng.alloc(buf.size), eng.alloc(npix * nch * ts + 64)
        d_in.upload(buf)
        d_out.upload(np.full(npix * nch * ts + 64, CANARY, np.uint8))
        eng.interleave_device(d_in.ptr, stride, nch, ts, npix, d_out.ptr)
        out = d_out.download()
        assert np.array_equal(out[:npix * nch * ts], interleaved(planes, nch, ts)), (nch, ts, npix)
        assert (out[npix * nch * ts:] == CANARY).all(), (nch, ts, npix)
        # and back through the deinterleave kernel
        d_back = eng.alloc(buf.size)
        d_back.upload(np.full(buf.size, CANARY, np.uint8))
        eng.deinterleave_device(d_out.ptr, nch, ts, npix, d_back.ptr, stride)
        eng.synchronize()
        assert np.array_equal(d_back.download(), buf), (nch, ts, npix)
        for b in (d_in, d_out, d_back):
            b.free()
    d = eng.alloc(4096)
    with pytest.raises(hip.CodecError):
        eng.interleave_device(d.ptr, 1600, 2, 3, 100, d.ptr + 2048)        # element size 3
    with pytest.raises(hip.CodecError):
        eng.interleave_device(d.ptr, 1608, 2, 4, 100, d.ptr + 2048)        # stride no multiple of 16
    d.free()


def test_range_check_refuses_what_is_not_device_memory(eng):
    d = eng.alloc(1 << 20)
    assert eng.device_range_check(d.ptr, 1 << 20) == 0
    assert eng.device_range_check(d.ptr + 4096, (1 << 20) - 4096) == 0       # a sub-range
    assert eng.device_range_check(d.ptr + 4096, 1 << 20) == ERR_INVALID_PARAM  # runs past the allocation
    assert "allocation" in eng.last_error()
    assert eng.device_range_check(None, 16) == ERR_INVALID_PARAM
    host = np.zeros(4096, np.uint8)
    assert eng.device_range_check(host.ctypes.data, host.size) == ERR_INVALID_PARAM   # nothing is launched: the check only asks the runtime
    assert "not device memory" in eng.last_error()
    d.free()
    # the engine is as usable as before
    raw = plane(2)[:65536]
    chunks = eng.compress_host(hip.cparams(2), raw, [65536], [65536 + 32])
    outs, st = eng.decompress_host(chunks)
    assert not st.any() and np.array_equal(outs[0], raw)


def test_wait_stream_accepts_the_null_stream_and_its_own(eng):
    """(ordering behind a torch stream: tests/test_python_device.py, in a process where torch owns the HIP runtime)"""
    eng.wait_stream(None)
    eng.wait_stream(eng.stream_handle())
    raw = plane(2)[:65536]
    chunks = eng.compress_host(hip.cparams(2), raw, [65536], [65536 + 32])
    outs, st = eng.decompress_host(chunks)
    assert not st.any() and np.array_equal(outs[0], raw)
