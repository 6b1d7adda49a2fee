"""The head-path planes of tests/_head_planes.py through the real encode launch: each plane is the upper byte plane of a
typesize-2 block (the lower plane is noise), 1 - 3 blocks per chunk, through compress_device / decompress_device.  Chunk bytes
must be the oracle's and the pixels must come back.

A batch has ONE blocksize and a block is split into planes only when it is a full block, so planes of one length share a batch
(blocksize = twice the plane) and every length gets a batch of its own; lengths below blosc2's split threshold travel as the
unsplit stream the oracle makes of them."""
import numpy as np
import pytest

import _head_planes as H
import _oracle as O
from cimg import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(0)
    yield e
    e.close()


def _batches():
    by_len = {}
    for name, p, _ in H.planes():
        by_len.setdefault(p.size, []).append((name, p))
    return sorted(by_len.items())


BATCHES = _batches()


@pytest.mark.parametrize("m,group", BATCHES, ids=["plane%d" % m for m, _ in BATCHES])
def test_head_planes_as_upper_planes_on_the_gpu(eng, m, group):
    rng = np.random.default_rng(m)
    blocks = []
    for k in range(max(6, len(group))):                   # 6 blocks at least: chunks of 1, 2 and 3 blocks
        _, upper = group[k % len(group)]
        b = np.empty(2 * m, np.uint8)
        b[0::2] = rng.integers(0, 256, m, dtype=np.uint8)
        b[1::2] = upper
        blocks.append(b)
    sizes, k = [], 0
    while k < len(blocks):
        nb = min(1 + len(sizes) % 3, len(blocks) - k)
        sizes.append(nb * 2 * m)
        k += nb
    raw = np.concatenate(blocks)
    n = len(sizes)
    dest = max(sizes) + 32
    stride = dest + 64
    raw_off = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64)
    comp_off = np.arange(n, dtype=np.int64) * stride
    p = hip.cparams(2, blocksize=2 * m)
    po = O.cparams(2, blocksize=2 * m)
    want = [O.compress(po, raw[o:o + s], destsize=dest) for o, s in zip(raw_off, sizes)]
    d_raw, d_out, d_comp = eng.alloc(raw.size), eng.alloc(raw.size), eng.alloc(n * stride + 64)
    try:
        d_raw.upload(raw)
        d_comp.upload(np.full(n * stride + 64, 0x5A, np.uint8))
        cbytes = eng.compress_device(p, d_raw.ptr, raw_off, sizes, d_comp.ptr, comp_off, [dest] * n)
        comp = d_comp.download()
        for i, (r, c) in enumerate(want):
            assert cbytes[i] == r, (m, i, cbytes[i], r)
            assert comp[comp_off[i]:comp_off[i] + r].tobytes() == c, (m, i)
        bsizes = [O.cbuffer_sizes(c)[2] for _, c in want]         # (blosc2 raises a blocksize below 32 bytes to 32: the header says which)
        eng.decompress_device(d_comp.ptr, comp_off, sizes, bsizes, d_out.ptr, raw_off)
        assert d_out.download().tobytes() == raw.tobytes()
    finally:
        for b in (d_raw, d_out, d_comp):
            b.free()
