"""blosc2 special chunks for the tests, written from the format alone (no code shared with csrc/): a 32-byte header whose
blosc2_flags byte names the kind in bits 4-6, followed -- for a repeated value -- by the value's typesize bytes.

    byte 0 version (5)   1 codec format version (1)   2 flags   3 typesize   4 nbytes   8 blocksize   12 cbytes
    16..21 filters   22 compcode   24..29 filters_meta   31 blosc2_flags

Every chunk a test reads is first decoded by the oracle (`want`), and that is the expectation; the oracle's destination is zeroed
beforehand, which is what an uninit chunk reads as here.
"""
import struct

import numpy as np

import _oracle as O

ZERO, NAN, VALUE, UNINIT = 1, 2, 3, 4
KINDS = {"zero": ZERO, "nan": NAN, "value": VALUE, "uninit": UNINIT}
ERR_DATA = -3
FLAGS_LZ4_UNSPLIT = 0x01 | 0x04 | 0x10 | (1 << 5)          # shuffle + bitshuffle bits (extended header), dont-split, codec format 1


def header(typesize, nbytes, blocksize, special, cbytes, flags=FLAGS_LZ4_UNSPLIT, filters=(0, 0, 0, 0, 0, 1), compcode=1,
           filters_meta=(0, 0, 0, 0, 0, 0)):
    h = bytearray(32)
    h[0], h[1], h[2], h[3] = 5, 1, flags, typesize
    h[4:16] = struct.pack("<iii", nbytes, blocksize, cbytes)
    h[16:22] = bytes(filters)
    h[22] = compcode
    h[24:30] = bytes(filters_meta)
    h[31] = special << 4
    return bytes(h)


def value_bytes(typesize, seed=0):
    """typesize bytes, all different where they can be, none zero"""
    return bytes((seed * 37 + 11 + 5 * k) % 255 + 1 for k in range(typesize))


def chunk(kind, typesize, nbytes, blocksize, value=None, **kw):
    """One special chunk with a hand-set geometry."""
    special = KINDS[kind] if isinstance(kind, str) else kind
    tail = (value_bytes(typesize) if value is None else bytes(value)) if special == VALUE else b""
    return header(typesize, nbytes, blocksize, special, 32 + len(tail), **kw) + tail


def from_cparams(p, kind, nbytes, value=None):
    """The chunk c-blosc2's constructors write for the oracle cparams `p`: the header of a special-zero chunk of those cparams (block
    size and flags by the oracle's geometry, never the memcpyed bit), with the special field and cbytes of the kind."""
    g = O.geometry(p, nbytes)
    return chunk(kind, p.typesize, nbytes, g.blocksize, value=value, flags=g.flags & ~0x02, filters=tuple(p.filters),
                 compcode=p.compcode, filters_meta=tuple(p.filters_meta))


def want(c):
    """The oracle's decode of chunk c (uint8); a refusal comes back as the negative code."""
    r, out = O.decompress(c)
    return out if r >= 0 else r


def geometry_nbytes(typesize, blocksize=4096):
    """two blocks and a leftover, rounded down to the typesize"""
    return (2 * blocksize + 1000) // typesize * typesize


def read_cases():
    """(id, chunk) over every kind and typesize of the read matrix: 4 KiB blocks, two of them and a leftover.  A block size that is no
    multiple of the typesize (typesize 3, 12, 255 here) makes blocks start at every element phase."""
    out = []
    for ts in (1, 2, 3, 4, 8, 12, 16, 255):
        out.append(("value-ts%d" % ts, chunk("value", ts, geometry_nbytes(ts), 4096)))
    for ts in (4, 8):
        out.append(("nan-ts%d" % ts, chunk("nan", ts, geometry_nbytes(ts), 4096)))
    for kind in ("uninit", "zero"):
        for ts in (1, 4):
            out.append(("%s-ts%d" % (kind, ts), chunk(kind, ts, geometry_nbytes(ts), 4096)))
    return out


def refused_cases():
    """(id, chunk): each must come back as ERR_DATA"""
    ts = 4
    n = geometry_nbytes(ts)
    short = header(ts, n, 4096, VALUE, 32 + ts - 1) + value_bytes(ts)[:ts - 1]
    ragged = chunk("value", 3, 2 * 4096 + 1001, 4096)                      # 9193 = 3 * 3064 + 1
    return [("value-short", short), ("value-ragged", ragged), ("nan-ts2", chunk("nan", 2, geometry_nbytes(2), 4096))]


def regular_chunk(typesize, nbytes, blocksize=4096, seed=1, clevel=5):
    """A good regular chunk (the oracle's) and its pixels: the neighbours of a refused chunk."""
    rng = np.random.default_rng(seed)
    raw = (np.arange(nbytes, dtype=np.int64) // 7 % 251).astype(np.uint8)
    raw[::53] ^= rng.integers(0, 255, raw[::53].size, dtype=np.uint8)
    p = O.cparams(typesize, clevel=clevel, blocksize=blocksize)
    r, c = O.compress(p, raw, destsize=nbytes + 64)
    assert r > 0
    return c, raw


# ---- a plane of 256 x 96 float32 in six 16-row chunks: regular, value, nan, zero, memcpyed, uninit ---------------------------------
PW, PH, ROWS, TS = 256, 96, 16, 4
CHUNK = PW * ROWS * TS
KINDS6 = ["regular", "value", "nan", "zero", "memcpyed", "uninit"]


def plane_params():
    return O.cparams(TS, clevel=5, blocksize=4096)


def six_chunks():
    """regular, value, nan, zero, memcpyed, uninit -- all with the header the same cparams give -> (chunks, decoded plane as float32 bits)"""
    p = plane_params()
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:ROWS, 0:PW]
    smooth = ((x // 7) * 0.5 + (y // 3) * 2.0).astype(np.float32).view(np.uint8).ravel()
    noise = rng.integers(0, 256, CHUNK, dtype=np.uint8)
    r, regular = O.compress(p, smooth, destsize=CHUNK + 32)
    assert r > 0
    r, zero = O.compress(p, np.zeros(CHUNK, np.uint8), destsize=CHUNK + 32)
    assert r == 32
    r, memcpyed = O.compress(p, noise, destsize=CHUNK + 32)
    assert r == CHUNK + 32
    value = from_cparams(p, "value", CHUNK, np.float32(-2.75).tobytes())
    nan = from_cparams(p, "nan", CHUNK)
    uninit = from_cparams(p, "uninit", CHUNK)
    chunks = [regular, value, nan, zero, memcpyed, uninit]
    return chunks, np.concatenate([want(c) for c in chunks])


def plane_regions():
    """(x, y, w, h): inside one chunk of every kind, across all six, rows that cross every boundary, 1 x 1 probes"""
    r = [(3, 16 * k + 2, 250, 9) for k in range(6)]
    r += [(0, 0, PW, PH), (17, 5, 200, 86), (255, 0, 1, PH), (0, 15, PW, 2), (100, 31, 50, 34)]
    r += [(0, 16 * k, 1, 1) for k in range(6)] + [(PW - 1, 16 * k + 15, 1, 1) for k in range(6)] + [(77, 40, 1, 1)]
    return r


# ---- the blosc2_chunk_* constructors through ctypes (lib: libcimg_hip.so or the mock library, with argtypes set) ---------------------
def _hip():
    from cimg import hip
    return hip


def _p(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def b2params(ts, clevel=5, blocksize=4096, compcode=1, splitmode=3, filt=1, trunc=None):
    cp = _hip().Blosc2CParams()
    cp.compcode, cp.clevel, cp.typesize, cp.nthreads, cp.blocksize, cp.splitmode = compcode, clevel, ts, 1, blocksize, splitmode
    cp.filters[5] = filt
    if trunc is not None:
        cp.filters[4], cp.filters_meta[4] = 4, trunc
    return cp


def construct(lib, kind, cp, nbytes, destsize=None, value=None):
    destsize = 32 + cp.typesize if destsize is None else destsize
    dest = np.full(destsize + 16, 0xA5, np.uint8)
    if kind == "value":
        v = np.frombuffer(value, np.uint8).copy()
        rc = lib.blosc2_chunk_repeatval(cp, nbytes, _p(dest), destsize, _p(v))
    else:
        rc = getattr(lib, {"zero": "blosc2_chunk_zeros", "nan": "blosc2_chunk_nans", "uninit": "blosc2_chunk_uninit"}[kind])(cp, nbytes, _p(dest), destsize)
    assert (dest[max(rc, 0):] == 0xA5).all()
    return rc, dest[:max(rc, 0)].tobytes()
