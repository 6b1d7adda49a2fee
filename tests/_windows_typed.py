"""Helpers of the typed window tests (test_emu_windows_typed.py, test_gpu_windows_typed.py): the build of
tests/emu/window_typed_emu.cpp, the cimg_window_typed struct, planes of every stored type that hold the values a conversion can get
wrong, and the expectation of a typed call.

Expectations never come from the code under test: a window's values are numpy indexing into the oracle's decode (or the source
pixels), converted by numpy with two separate ufunc calls -- (v.astype(float32) * float32(scale) + float32(offset)).astype(out) --
and compared bit for bit; where the expectation is NaN the result must be NaN.  Every other byte of the output keeps its canary."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle as O
import _special_chunks as S
import _windows_grouped as G
from _windows import CANARY, oracle_chunks, plane_of
from _windows_strided import StridedWindow, element_index

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
FLAGS = G.FLAGS + ["-ffp-contract=off"]
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_typed_emu.cpp")]

U8, I8, U16, I16, U32, I32, F16, F32, F64 = range(9)                  # CIMG_T_*
DTYPE = {U8: np.uint8, I8: np.int8, U16: np.uint16, I16: np.int16, U32: np.uint32, I32: np.int32, F16: np.float16, F32: np.float32,
         F64: np.float64}
SIZE = {t: np.dtype(d).itemsize for t, d in DTYPE.items()}
# scale / offset pairs that round in both steps; 3.0e-41 takes a float32 source into the subnormals, 7e4 a float16 output to inf
AFFINE = [(1 / 255, -0.4851), (-0.4851, 1 / 255), (3.0e-41, 0.0), (7e4, 0.0), (1.0, 0.0), (1 / 255, 3.0e-41), (0.1, 1e-3)]


class TypedWindow(C.Structure):
    _fields_ = StridedWindow._fields_ + [("elem_pitch", C.c_int64), ("src_type", C.c_int32), ("out_type", C.c_int32),
                                         ("scale", C.c_float), ("offset", C.c_float)]


assert C.sizeof(TypedWindow) == 80


def twindows(specs):
    arr = (TypedWindow * max(len(specs), 1))()
    for i, s in enumerate(specs):
        for k, v in s.items():
            setattr(arr[i], k, float(v) if k in ("scale", "offset") else int(v))
    return arr


def build_emu(out_dir, sanitize=False):
    """tests/emu/window_typed_emu.cpp with emu.cpp and wide_emu.cpp as a library (or, sanitize: with window_typed_asan_main.cpp as a
    stand-alone program under ASan / UBSan, LDS modelled with zero slack); the multiply-add is never contracted"""
    if sanitize:
        out = os.path.join(str(out_dir), "window_typed_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                               os.path.join(EMU, "window_typed_asan_main.cpp"), *SOURCES, "-o", out])
        return out
    out = os.path.join(str(out_dir), "libwindow_typed_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    dev = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.wnemu_windows_typed_device.argtypes = L.wnemu_windows_grouped_device.argtypes = dev
    L.wnemu_typed_unit_order.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int]
    L.wnemu_window_stats.argtypes = [vp]
    L.wemu_compress_batch.argtypes = [C.POINTER(G.EmuCParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.emu_set_write_order.argtypes = [C.c_int]
    return L


def _table(t, rng):
    """64 values of type t: the ones a conversion can get wrong, then random ones"""
    d = np.dtype(DTYPE[t])
    if t in (U8, I8, U16, I16, U32, I32):
        info = np.iinfo(d)
        v = [info.min, info.max, 0, 1, info.max // 2, info.max // 2 + 1, info.max - 1, 127 % (info.max + 1), 100]
        if t in (U32, I32):                                           # above 2^24: (float)v rounds, ties to even both ways
            v += [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 30 + 64, 2 ** 30 + 65, 2 ** 31 - 1, 2 ** 31 - 65, 123456789]
        if t == U32:
            v += [2 ** 32 - 1, 2 ** 32 - 129, 2 ** 31 + 128, 2 ** 31 + 384, 4000000001]
        if t == I32:
            v += [-(2 ** 24 + 1), -(2 ** 24 + 3), -(2 ** 31), -(2 ** 31 - 65), -123456789]
        if info.min < 0:
            v += [-1, -2, info.min + 1]
        a = np.array(v, np.int64)
        a = np.concatenate([a, rng.integers(info.min, int(info.max) + 1, 64 - a.size, dtype=np.int64)])
        return a.astype(d)
    if t == F16:
        bits = [0x7E00, 0x7C01, 0xFE55, 0x7DFF, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00, 0x3C01,
                0x3555, 0x5BF8, 0x5BF9]
        a = np.array(bits, np.uint16)
        a = np.concatenate([a, rng.integers(0, 0x7C00, 64 - a.size).astype(np.uint16) | (rng.integers(0, 2, 64 - a.size).astype(np.uint16) << 15)])
        return a.view(np.float16)
    if t == F32:
        bits = [0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x80000001,
                0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,
                0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,        # 1 + 2^-11 (a float16 tie), 1 + 3 * 2^-11 (tie, odd), either side
                0x477FEFFF, 0x477FF000, 0x477FE000, 0x33000000, 0x33000001, 0x33800000, 0x337FFFFF, 0x38800000, 0x387FFFFF, 0x387FE000]
        a = np.array(bits, np.uint32)
        r = (rng.standard_normal(64 - a.size) * 10.0 ** rng.integers(-6, 6, 64 - a.size)).astype(np.float32)
        return np.concatenate([a.view(np.float32), r])
    v = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 - 2.0 ** -50,
         1e-40, -1e-40, 1.401298464324817e-45, 0.7e-45, 0.70064924e-45, 1e-50, 1e39, -1e39, 3.4028235677973366e38, 3.4028234663852886e38,
         65504.0, 65519.999, 65520.0, 0.1, 1 / 3, 255.0, 254.99999999]
    a = np.array(v, np.float64)
    r = rng.standard_normal(64 - a.size) * 10.0 ** rng.integers(-8, 8, 64 - a.size)
    return np.concatenate([a, r])


_planes = {}


def plane(t, n=G.W * G.H, seed=0):
    """n values of type t (read-only, shared): runs of 1 .. 8 equal values drawn from _table, so the codecs find matches and every
    special value turns up many times"""
    key = (t, n, seed)
    if key not in _planes:
        rng = np.random.default_rng(500 + 16 * seed + t)
        tab = _table(t, rng)
        idx = np.repeat(rng.integers(0, 64, n), rng.integers(1, 9, n))[:n]
        a = tab[idx].copy()
        a.setflags(write=False)
        _planes[key] = a
    return _planes[key]


def identity(s):
    return s["src_type"] == s["out_type"] and np.float32(s.get("scale", 1.0)) == 1 and np.float32(s.get("offset", 0.0)) == 0


def out_size(s):
    return SIZE[s["out_type"]]


def typed(spec, src_type, out_type, scale=1.0, offset=0.0, pitch_mult=1):
    """a cimg_window_strided spec dict -> a cimg_window_typed one (out_off / out_pitch: pack_typed)"""
    return dict(spec, src_type=src_type, out_type=out_type, scale=scale, offset=offset, elem_pitch=pitch_mult * SIZE[out_type])


def pack_typed(specs, gap=24, lead=8):
    """Give each window its own stretch of the output: `lead` canary bytes before it, rows of (width - 1) * elem_pitch + the output
    size + `gap` canary bytes, everything a multiple of 8.  Returns (specs, output size)."""
    at, out = 0, []
    for s in specs:
        s = dict(s)
        row = max(s["width"] - 1, 0) * s["elem_pitch"] + out_size(s)
        s.setdefault("out_pitch", (row + gap + 7) // 8 * 8)
        s["out_off"] = at + lead
        at = (s["out_off"] + s["out_pitch"] * max(s["height"], 1) + 15) // 8 * 8
        out.append(s)
    return out, at + 64


def convert(v, s):
    """numpy's answer for the stored values v of window s"""
    if identity(s):
        return v
    with np.errstate(all="ignore"):
        x = v.astype(np.float32)
        y = x * np.float32(s["scale"])
        y = y + np.float32(s["offset"])
        return y.astype(DTYPE[s["out_type"]])


def positions(s):
    """output byte offset of every element of window s: (height, width) int64"""
    return (s["out_off"] + np.arange(s["height"], dtype=np.int64)[:, None] * (s["out_pitch"] if s["height"] > 1 else 0) +
            np.arange(s["width"], dtype=np.int64)[None, :] * s["elem_pitch"])


def check_output(out, values, specs):
    """out: the uint8 output of a typed call over a canary-filled buffer; values[k]: the decoded plane of window k as an array of its
    src_type.  Every element bit for bit (NaN where numpy gives NaN), every other byte the canary."""
    rest = out.copy()
    for v, s in zip(values, specs):
        if s["width"] == 0 or s["height"] == 0:
            continue
        want = convert(np.asarray(v)[element_index(s)], s)
        osz = want.dtype.itemsize
        assert osz == (SIZE[s["src_type"]] if identity(s) else out_size(s))
        at = positions(s)[..., None] + np.arange(osz, dtype=np.int64)
        got = np.ascontiguousarray(out[at]).view(want.dtype)[..., 0]
        ubits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[osz]
        nan = np.zeros(want.shape, bool) if identity(s) or want.dtype.kind != "f" else np.isnan(want)
        same = got.view(ubits) == np.ascontiguousarray(want).view(ubits)
        bad = ~(same | nan)
        assert not bad.any(), (s, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
        if nan.any():
            assert np.isnan(got[nan]).all(), s
        rest[at.ravel()] = CANARY
    assert (rest == CANARY).all(), np.flatnonzero(rest != CANARY)[:8]

def raw_of(values):
    return np.ascontiguousarray(values).view(np.uint8).ravel()


def dress(rects, src, out, k0=0):
    """the rectangles as typed windows: scale / offset and elem_pitch (1, 3, 4 output sizes) cycle through the list"""
    specs = []
    for k, r in enumerate(rects):
        sc, of = AFFINE[(k + k0) % len(AFFINE)]
        specs.append(typed(r, src, out, sc, of, pitch_mult=(1, 3, 4)[(k + k0) % 3]))
    return specs


def modes_chunks(zstd_chunk, src):
    """one plane through every mode of WindowBlock::byte_at: chunk 0 lz4 + shuffle, 1 lz4 + bitshuffle, 2 blosclz, 3 memcpyed noise,
    4 zeros, 5 a repeated value, 6 NaN, 7 zstd (the whole route: copy mode; zstd_chunk(ts, raw, blocksize) writes it) -- 16 rows of W a chunk"""
    ts = SIZE[src]
    d = np.dtype(DTYPE[src])
    ce = 16 * G.W
    v = plane(src, 8 * ce, seed=1).copy()
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, ce * ts, dtype=np.uint8)
    v[3 * ce:4 * ce] = noise.view(d)
    v[4 * ce:5 * ce] = np.zeros(ce, d)
    val = plane(src, 64)[5:6]
    v[5 * ce:6 * ce] = val[0]
    raw = raw_of(v)
    bsize = 4096
    piece = lambda i: raw[i * ce * ts:(i + 1) * ce * ts]
    one = lambda p, i: oracle_chunks(p, piece(i), ce * ts)[0]
    chunks = [one(O.cparams(ts, clevel=5, blocksize=bsize), 0), one(O.cparams(ts, clevel=5, blocksize=bsize, filters=(0, 0, 0, 0, 0, 2)), 1),
              one(O.cparams(ts, clevel=5, blocksize=bsize, compcode=G.BLOSCLZ), 2), one(O.cparams(ts, clevel=0, blocksize=bsize), 3),
              S.chunk("zero", ts, ce * ts, bsize), S.chunk("value", ts, ce * ts, bsize, value=raw_of(val).tobytes()),
              S.chunk("nan", ts, ce * ts, bsize) if d.kind == "f" and ts >= 4 else S.chunk("uninit", ts, ce * ts, bsize),    # (blosc2: NaN chunks of float32 / float64 only)
              zstd_chunk(ts, piece(7), bsize)]
    assert chunks[3][2] & 0x02                                               # (the noise chunk is memcpyed)
    decoded = plane_of(chunks)
    return chunks, decoded.view(d)


def three_planes(src=U8):
    """a three-channel image: three planes of the W x H geometry, one batch (channel c: chunks [c * n, (c + 1) * n))"""
    ts = SIZE[src]
    cbytes, bsize = G.GEOMETRY[ts]
    vals = [plane(src, seed=c) for c in range(3)]
    per = [oracle_chunks(O.cparams(ts, clevel=5, blocksize=bsize), raw_of(v), cbytes) for v in vals]
    return vals, [c for p in per for c in p], len(per[0])


def pixel_major(regions, n, src, out, scales, offsets, nchan=3):
    """regions (x, y, w, h, sx, sy) -> 3 windows each writing the channel slots of (N, oh, ow, C) rows, and the output size"""
    osz = SIZE[out]
    specs, at = [], 64
    for (x, y, w, h, sx, sy) in regions:
        ow, oh = (w + sx - 1) // sx, (h + sy - 1) // sy
        for c in range(nchan):
            specs.append(dict(typed(G.rect(x, y, w, h, sx, sy, nchunks=n, chunk_first=c * n), src, out, scales[c], offsets[c], pitch_mult=nchan),
                              out_off=at + c * osz, out_pitch=ow * nchan * osz))
        at += oh * ow * nchan * osz
    return specs, at + 64
