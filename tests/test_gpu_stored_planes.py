"""Stored planes of chunks assembled inside the encode launch, on the GPU: never written to the scratch slot, placed from the
launch's input (encode_kernel.h: REC_RAW_SRC).  Every batch must be the oracle's bytes and decode to the pixels.  The shapes are
the emulator's (tests/_stored_cases.py) -- every kind of chunk the placing phase meets -- plus one batch with fewer resident
waves than work items, where waves place their streams while others still encode."""
import numpy as np
import pytest

import _oracle as O
import _stored_cases as S
from cimg import hip, synth

pytestmark = pytest.mark.gpu

GPU_CASES = [c for c in S.cases() if c[0][0] in "abegh"]


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def _check_batch(eng, ts, filters, split, raw, sizes, dest, stride):
    n = len(sizes)
    stride = dest + 64 if stride is None else stride
    raw_off = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64)
    comp_off = np.arange(n, dtype=np.int64) * stride
    d_raw, d_out, d_comp = eng.alloc(raw.size), eng.alloc(raw.size), eng.alloc(n * stride + 64)
    try:
        d_raw.upload(raw)
        d_comp.upload(np.full(n * stride + 64, 0x5A, np.uint8))
        p = hip.cparams(ts, splitmode=split, filters=filters)
        po = O.cparams(ts, splitmode=split, filters=filters)
        want = [O.compress(po, raw[o:o + s], destsize=dest) for o, s in zip(raw_off, sizes)]
        for rep in range(2):                                  # the second batch meets the records and flags the first one left behind
            cbytes = eng.compress_device(p, d_raw.ptr, raw_off, sizes, d_comp.ptr, comp_off, [dest] * n)
            comp = d_comp.download()
            for i, (r, c) in enumerate(want):
                assert cbytes[i] == r, (rep, i, cbytes[i], r)
                assert comp[comp_off[i]:comp_off[i] + r].tobytes() == c, (rep, i)
                assert (comp[comp_off[i] + dest:comp_off[i] + stride] == 0x5A).all(), (rep, i)     # nothing past a chunk's capacity
        eng.decompress_device(d_comp.ptr, comp_off, sizes, [S.BLOCK] * n, d_out.ptr, raw_off)
        assert d_out.download().tobytes() == raw.tobytes()
    finally:
        for b in (d_raw, d_out, d_comp):
            b.free()


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_stored_planes_on_the_gpu(eng, case):
    _, ts, filters, split, raw, sizes, dest, stride, _, _ = case
    _check_batch(eng, ts, filters, split, raw, sizes, dest, stride)


def test_fewer_resident_waves_than_items(monkeypatch):
    """20 MiB of tiled float16 in 5 chunks of 4 MiB: 640 blocks, 1280 plane items.  One workgroup per CU leaves far fewer resident
    waves than items, so the first waves to find the queue dry place their streams -- stored planes from the source -- while
    others still encode.  The launch completing is the liveness check; nothing is made to time out."""
    monkeypatch.setenv("CIMG_ENC_WGS_PER_CU", "1")
    e = hip.Engine(0)
    try:
        raw = np.ascontiguousarray(synth.tiled_channel(np.float16, 4096, 2560)).view(np.uint8).ravel()
        chunk = 4 * 1024 * 1024
        _check_batch(e, 2, S.SHUFFLE, S.AUTO, raw, [chunk] * 5, chunk + 32, None)
    finally:
        e.close()
