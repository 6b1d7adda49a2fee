"""Batches for the stored-plane tests (emulator and GPU): 3 chunks of 4 blocks of 32 KiB unless a case says otherwise.

A case is (name, typesize, filters, splitmode, pixels as uint8, chunk sizes, destsize per chunk, comp stride or None, expected
number of streams left for placing from the source, expected number placed).  The expected counts follow from the data: a byte
plane of uniform noise has no 4-byte repeat within LZ4's reach and is stored; where a chunk ends up memcpyed its stored records
exist but nobody places them; a chunk with a leftover block is not assembled inside the launch and keeps the scratch path."""
import numpy as np

from cimg import synth

BLOCK = 32768
CHUNK = 4 * BLOCK
SHUFFLE = (0, 0, 0, 0, 0, 1)
NOFILTER = (0, 0, 0, 0, 0, 0)
AUTO, ALWAYS = 3, 1


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def cases():
    rng = np.random.Generator(np.random.PCG64(20240611))
    tiled16 = _u8(synth.tiled_channel(np.float16, 1024, 192))            # 3 chunks; per block: coded high plane, stored low plane
    random16 = _u8(synth.random_channel(np.float16, 1024, 64))           # 1 chunk of noise: both planes stored, the chunk memcpyed
    natural16 = _u8(synth.natural_channel(np.float16, 1024, 192))
    tiled32 = _u8(synth.tiled_channel(np.float32, 1024, 96))             # per block: plane 3 a run, planes 2 and 1 coded, plane 0 stored
    out = []
    out.append(("a_tiled_f16", 2, SHUFFLE, AUTO, tiled16, [CHUNK] * 3, CHUNK + 32, None, 12, 12))
    mixed = np.concatenate([tiled16[:CHUNK], random16, tiled16[CHUNK:2 * CHUNK]])
    out.append(("b_random_chunk_memcpyed", 2, SHUFFLE, AUTO, mixed, [CHUNK] * 3, CHUNK + 32, None, 4 + 8 + 4, 4 + 4))
    out.append(("c_natural_f16", 2, SHUFFLE, AUTO, natural16, [CHUNK] * 3, CHUNK + 32, None, 0, 0))
    out.append(("d_zero", 2, SHUFFLE, AUTO, np.zeros(3 * CHUNK, np.uint8), [CHUNK] * 3, CHUNK + 32, None, 0, 0))
    out.append(("e_tiled_f32", 4, SHUFFLE, AUTO, tiled32, [CHUNK] * 3, CHUNK + 32, None, 12, 12))
    # no filter, split forced: stream s of a block is its s-th half -- the first a short pattern repeated (coded), the second noise (stored)
    halves = []
    for b in range(12):
        halves.append(np.resize(rng.integers(0, 256, 48 + b, dtype=np.uint8), BLOCK // 2))
        halves.append(rng.integers(0, 256, BLOCK // 2, dtype=np.uint8))
    out.append(("f_nofilter_ts2", 2, NOFILTER, ALWAYS, np.concatenate(halves), [CHUNK] * 3, CHUNK + 32, None, 12, 12))
    # the middle chunk ends in a short block: planes through scratch, laid out and placed by the two kernels behind the launch
    short = 3 * BLOCK + 1696
    g = np.concatenate([tiled16[:CHUNK], tiled16[CHUNK:CHUNK + short], tiled16[2 * CHUNK:]])
    out.append(("g_leftover_chunk_between", 2, SHUFFLE, AUTO, g, [CHUNK, short, CHUNK], CHUNK + 32, None, 8, 8))
    # chunks 1 and 2 off a 4-byte boundary: bstarts[] cannot be written through, layout and placing take the fenced branch
    out.append(("h_odd_comp_off", 2, SHUFFLE, AUTO, tiled16, [CHUNK] * 3, CHUNK + 32, CHUNK + 32 + 65, 12, 12))
    # zeros but for the low bytes of the very last block: one stored plane, in the last block of the last chunk
    last = np.zeros(3 * CHUNK, np.uint8)
    last[-BLOCK::2] = rng.integers(0, 256, BLOCK // 2, dtype=np.uint8)
    out.append(("i_only_last_block", 2, SHUFFLE, AUTO, last, [CHUNK] * 3, CHUNK + 32, None, 1, 1))
    return out
