"""Helpers of the typed window-write tests (test_emu_window_writes_typed.py, test_gpu_window_writes_typed.py): the build of
tests/emu/window_write_typed_emu.cpp, source tables of float32 / float16 memory that hold what the way back can get wrong, the
numpy conversion, and the two-step check of a call's new chunks.

Expectations never come from the code under test.  A written pixel is numpy's answer for its memory value y, each step a separate
ufunc call: x = y.astype(float32); d = subtract(x, float32(offset)); t = divide(d, float32(scale)); then, for an integer plane,
clip(rint(where(isnan(t), 0, t).astype(float64)), min, max).astype(type) (the float64 step only states the 32-bit bounds exactly),
for a float16 plane t.astype(float16), for a float32 plane t.  The converted windows are assigned into the oracle's decode of the
old chunks in call order (_window_writes_strided.expected).  A NaN's bits are not fixed for float planes, so a call's new chunks
are checked in two steps (check_new): (a) the oracle's decode of the new chunk equals the edited pixels bit for bit, NaN where
numpy has NaN; (b) the new chunk's bytes equal the oracle's compress of those decoded pixels."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle as O
import _window_writes_strided as S
import _windows_grouped as G
import _windows_typed as T
from _windows_strided import element_index
from _windows_typed import DTYPE, F16, F32, F64, I8, I16, I32, SIZE, U8, U16, U32  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
FLAGS = G.FLAGS + ["-ffp-contract=off"]
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_write_typed_emu.cpp")]

# stored -> memory is y = v * scale + offset; the write applies the inverse with the same pair
PAIRS = [(1 / 255, 0.0), (1 / 255, -0.4851), (1 / (255 * 0.229), -0.485 / 0.229), (2 / 65535, -1.0), (-0.5, 3.0), (1.0, 0.0)]
INTS = (U8, I8, U16, I16, U32, I32)
WORD = 0x5A5A5A5A                                         # canary of new_cbytes / status words


def build_emu(out_dir, sanitize=False):
    """tests/emu/window_write_typed_emu.cpp with emu.cpp and wide_emu.cpp as a library (or, sanitize: with
    window_write_typed_asan_main.cpp as a stand-alone program under ASan / UBSan, LDS modelled with zero slack); the subtraction and
    the division are never contracted"""
    if sanitize:
        out = os.path.join(str(out_dir), "window_write_typed_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                               os.path.join(EMU, "window_write_typed_asan_main.cpp"), *SOURCES, "-o", out])
        return out
    out = os.path.join(str(out_dir), "libwindow_write_typed_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.wwtemu_update_device.argtypes = L.wwsemu_update_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.wwemu_update_stats.argtypes = [vp]
    L.wwsemu_schedule_stats.argtypes = [vp]
    L.wemu_compress_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.wemu_decompress_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emu_set_write_order.argtypes = [C.c_int]
    return L


def unconvert(y, stored, scale=1.0, offset=0.0):
    """numpy's answer for the memory values y written to a plane of type `stored`"""
    d = np.dtype(DTYPE[stored])
    with np.errstate(all="ignore"):
        x = y.astype(np.float32)
        t = np.subtract(x, np.float32(offset))
        t = np.divide(t, np.float32(scale))
        if d.kind in "iu":
            info = np.iinfo(d)
            r = np.rint(np.where(np.isnan(t), np.float32(0), t).astype(np.float64))
            return np.clip(r, info.min, info.max).astype(d)
        return t.astype(d)


def division_teeth():
    """the elements at which a true division and a multiply by the reciprocal disagree, for scale float32(1 / 255)"""
    s = np.float32(1 / 255)
    y = (np.arange(512) / 2).astype(np.float32) * s
    return y, int((np.rint(y / s) != np.rint(y * np.float32(255))).sum())


_tables = {}


def table(mem, stored, scale=1.0, offset=0.0):
    """values of memory type `mem` (F32 or F16) for a plane of type `stored` under (scale, offset): NaN, +-inf, +-0; ties
    (k + 0.5) * scale + offset for even and odd k; the saturation edges lo - 0.5, lo - 0.51, hi + 0.49, hi + 0.5, hi + 1; +-2^31,
    2^32, 2^24 + 1; float32 subnormals; 65504 and half subnormals; values a half result rounds at a tie; half steps k / 2 that tell
    a true division from a reciprocal multiply; random values around the range (read-only, shared)"""
    key = (mem, stored, float(np.float32(scale)), float(np.float32(offset)))
    if key in _tables:
        return _tables[key]
    rng = np.random.default_rng(900 + 16 * mem + stored)
    d = np.dtype(DTYPE[stored])
    s, o = float(np.float32(scale)), float(np.float32(offset))
    lo, hi = (np.iinfo(d).min, np.iinfo(d).max) if d.kind in "iu" else (-70000, 70000)
    mid = np.clip(np.array([0, 1, 2, 3, 4, 5, 100, 101, 126, 127, 128, 254, 1000, 1001, 32766, 32767, 65534, -1, -2, -3, -4, -127, -128, -129,
                            -32768, -32769], np.float64), lo - 2, hi + 2)
    stored_units = np.concatenate([mid + 0.5, mid - 0.5, mid + 0.25, mid, [lo - 0.5, lo - 0.51, lo - 1, lo, hi + 0.49, hi + 0.5, hi + 1, hi, hi - 0.5],
                                   [2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 2.0 ** 24 + 1, 2.0 ** 31 - 64, 2.0 ** 31 - 128, -2.0 ** 31 - 256, 2.0 ** 32 - 128],
                                   [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 65504.0, 65519.9, 65520.0, 6e-8, 3 * 2.0 ** -25,
                                    2.0 ** -25, 2.0 ** -24, 6.1e-5, 1e-40, -1e-40, 1.4e-45],
                                   rng.uniform(lo - 2.0, hi + 2.0, 160) if hi - lo < 2 ** 17 else
                                   np.concatenate([rng.uniform(lo - 2.0, hi + 2.0, 80), rng.uniform(-300, 300, 80)])])
    f32 = np.float32
    with np.errstate(all="ignore"):
        y = stored_units.astype(f32) * f32(s) + f32(o)                                # (how a typed read makes them)
        halves = (np.arange(512) / 2).astype(f32) * f32(s) + f32(o)
        raw = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38, 65504.0, -65504.0, 65520.0, 6e-8,
                        1.0, 0.5, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 2.0 ** 24 + 1, 3.4e38, -3.4e38, o, o + s / 2, o - s / 2], np.float64).astype(f32)
        a = np.concatenate([raw, y, halves]).astype(DTYPE[mem])
    nanb = np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32).view(f32) if mem == F32 else np.array([0x7E01, 0xFE55, 0x7C01], np.uint16).view(np.float16)
    a = np.concatenate([nanb, a])
    a.setflags(write=False)
    _tables[key] = a
    return a


assert division_teeth()[1] > 0, "the tie table can no longer tell a division from a reciprocal multiply"


def typed(spec, stored, mem, scale=1.0, offset=0.0, pitch_mult=1):
    """a cimg_window_strided spec dict -> a cimg_window_typed one for a WRITE: src_type the plane's, out_type the memory's"""
    return T.typed(spec, stored, mem, scale, offset, pitch_mult)


def dress(rects, stored, mem, pairs=PAIRS, k0=0):
    """the rectangles as typed windows: scale / offset pairs and elem_pitch (1, 3, 4 memory sizes) cycle through the list"""
    return [typed(r, stored, mem, *pairs[(k + k0) % len(pairs)], pitch_mult=(1, 3, 4)[(k + k0) % 3]) for k, r in enumerate(rects)]


def source(specs, seed=3, tables=None):
    """Lay the windows' SOURCE elements out (T.pack_typed: rows with gaps, elem_pitch as each spec says) in a buffer of random bytes
    and fill every element from the window's table, each window starting further into it.
    -> (specs with out_off / out_pitch, uint8 source, the memory values of every window as (height, width) arrays)"""
    specs, size = T.pack_typed(specs)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size, dtype=np.uint8)
    vals = []
    for k, s in enumerate(specs):
        n = s["width"] * s["height"]
        if T.identity(s):
            tab = T.plane(s["src_type"], 64)
        else:
            tab = table(s["out_type"], s["src_type"], s["scale"], s["offset"]) if tables is None else tables[k]
        v = tab[(np.arange(n) + 37 * k) % tab.size].reshape(s["height"], s["width"])
        vals.append(v)
        if n:
            msz = v.dtype.itemsize
            at = T.positions(s)[..., None] + np.arange(msz, dtype=np.int64)
            src[at.ravel()] = np.ascontiguousarray(v).view(np.uint8).ravel()
    return specs, src, vals


def dense(specs, vals):
    """the CONVERTED windows as strided specs with a dense source of the stored type (for _window_writes_strided.expected)"""
    plain = [{k: s[k] for k in ("chunk_first", "chunk_count", "origin", "row_pitch", "col_pitch", "width", "height")} for s in specs]
    ts = SIZE[specs[0]["src_type"]] if specs else 1
    plain, dsrc = S.source(plain, ts)
    for s, t, v in zip(plain, specs, vals):
        if not v.size:
            continue
        c = v if T.identity(t) else unconvert(v, t["src_type"], t["scale"], t["offset"])
        b = np.ascontiguousarray(c).view(np.uint8).reshape(t["height"], -1)
        for r in range(t["height"]):
            o = s["out_off"] + r * s["out_pitch"]
            dsrc[o:o + b.shape[1]] = b[r]
    return plain, dsrc


def expected(p, chunks, specs, vals, destsize, compress=None, planes=None):
    """-> (want: numpy's new chunk of every touched chunk, None for the others; edited: {chunk_first: the edited plane, uint8})"""
    ts = SIZE[specs[0]["src_type"]]
    plain, dsrc = dense(specs, vals)
    return S.expected(p, chunks, plain, ts, dsrc, destsize, compress=compress, planes=planes)


def check_new(p, chunks, specs, new, want, edited, decode=None, compress=None):
    """the two steps of the module docstring over a call's new chunks (decode / compress: the oracle's unless given; with a
    compress of its own a codec has no byte-exact oracle, and step (b) asks for what that compress gives)"""
    stored = specs[0]["src_type"]
    d = np.dtype(DTYPE[stored])
    nb = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8))[0] for c in chunks]
    seen = set()
    for s in specs:
        cf, cn = s["chunk_first"], s["chunk_count"]
        off = 0
        for c in range(cf, cf + cn):
            o, off = off, off + nb[c]
            if c in seen:
                continue
            seen.add(c)
            assert (new[c] is None) == (want[c] is None), (c, new[c] is None)
            if new[c] is None:
                continue
            got = O.decompress(new[c])[1] if decode is None else decode(new[c], nb[c])
            exp = edited[cf][o:o + nb[c]]
            assert got.size == exp.size, (c, got.size, exp.size)
            same = got == exp
            if not same.all() and d.kind == "f":
                n = nb[c] // d.itemsize * d.itemsize
                g, e = got[:n].view(d), exp[:n].view(d)
                bad = ~((g.view(np.uint8).reshape(-1, d.itemsize) == e.view(np.uint8).reshape(-1, d.itemsize)).all(axis=1) | (np.isnan(g) & np.isnan(e)))
                assert not bad.any() and same[n:].all(), (c, np.flatnonzero(bad)[:6], g[bad][:6], e[bad][:6])
            else:
                assert same.all(), (c, np.flatnonzero(~same)[:8], got[~same][:8], exp[~same][:8])
            if compress is None:
                r, b = O.compress(p, got, destsize=len(new[c]) + 64)
                assert r > 0 and b == new[c], (c, r, len(new[c]))
            elif compress is not False:
                assert compress(got, len(new[c]) + 64) == new[c], c


def pixel_major(regions, n, stored, mem, scales, offsets, nchan=3):
    """regions (x, y, w, h, sx, sy) -> nchan windows each, reading the channel slots of (N, oh, ow, C) rows"""
    specs, size = T.pixel_major(regions, n, stored, mem, scales, offsets, nchan)
    return specs, size


def fill_pixel_major(specs, size, seed=5):
    """a pixel-major source for pixel_major()'s windows: every slot from its window's table"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size, dtype=np.uint8)
    vals = []
    for k, s in enumerate(specs):
        tab = table(s["out_type"], s["src_type"], s["scale"], s["offset"])
        n = s["width"] * s["height"]
        v = tab[(np.arange(n) * 7 + 11 * k) % tab.size].reshape(s["height"], s["width"])
        vals.append(v)
        at = T.positions(s)[..., None] + np.arange(v.dtype.itemsize, dtype=np.int64)
        src[at.ravel()] = np.ascontiguousarray(v).view(np.uint8).ravel()
    return src, vals
