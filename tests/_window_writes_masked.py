"""Helpers of the masked / constant window-write tests (test_emu_window_writes_masked.py, test_gpu_window_writes_masked.py): the build
of tests/emu/window_write_masked_emu.cpp, the four forms of a window (array / constant x masked / unmasked), the masks, and the
expected new chunks.

Expectations never come from the code under test: the edited pixels are np.copyto(view, src_or_value, where=mask) into the oracle's
decode of the old chunks, window after window in call order -- view = plane[origin + r * row_pitch + c * col_pitch] --, then the
oracle's compress per touched chunk (or a caller's compress, for codecs without a byte-exact oracle).  A chunk is touched if it holds
a byte of an element of a window, whatever the window's mask says."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle as O
import _window_writes_strided as S
import _windows_grouped as G
from _windows_strided import element_index
from cimg import hip

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
FLAGS = G.FLAGS + ["-ffp-contract=off"]                    # (the typed emulator this one includes wants it)
SOURCES = [os.path.join(EMU, f) for f in ("emu.cpp", "wide_emu.cpp", "window_write_masked_emu.cpp")]

WM_CONST, WM_MASK = 1, 2
FORMS = {"array": 0, "const": WM_CONST, "array_masked": WM_MASK, "const_masked": WM_CONST | WM_MASK}
MASKS = ("ones", "zeros", "checker", "one", "random", "values", "runs")
WORD = 0x5A5A5A5A                                         # canary of new_cbytes / status words


def build_emu(out_dir, sanitize=False):
    """tests/emu/window_write_masked_emu.cpp with emu.cpp and wide_emu.cpp as a library (or, sanitize: with
    window_write_masked_asan_main.cpp as a stand-alone program under ASan / UBSan, LDS modelled with zero slack)"""
    if sanitize:
        out = os.path.join(str(out_dir), "window_write_masked_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMU_LDS_SLACK=0", *FLAGS,
                               os.path.join(EMU, "window_write_masked_asan_main.cpp"), *SOURCES, "-o", out])
        return out
    out = os.path.join(str(out_dir), "libwindow_write_masked_emu.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", *FLAGS, *SOURCES, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.wwsemu_update_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.wwsemu_update_host.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.wwmemu_update_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.wwmemu_update_host.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.wwemu_update_stats.argtypes = [vp]
    L.wwsemu_schedule_stats.argtypes = [vp]
    L.wwemu_free.argtypes = [vp]
    L.wemu_compress_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.emu_set_write_order.argtypes = [C.c_int]
    return L


mwindows = hip.masked_windows                              # spec dicts -> a ctypes array of cimg_window_masked


def make_mask(kind, h, w, rng):
    """(h, w) uint8.  ones / zeros; checker; one: exactly one element set; random: 50 %; values: 0, 2 and 255 (any nonzero byte
    writes); runs: runs of 1, 2 and 3 set bytes with gaps of 1 and 2, period 10 -- against the dword period of 4 every alignment of
    every run length comes up"""
    if kind == "ones":
        return np.ones((h, w), np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    if kind == "checker":
        return ((r + c) & 1).astype(np.uint8)
    if kind == "one":
        m = np.zeros((h, w), np.uint8)
        m[h // 2, w // 2] = 1
        return m
    if kind == "random":
        return (rng.random((h, w)) < 0.5).astype(np.uint8)
    if kind == "values":
        return rng.choice(np.array([0, 2, 255], np.uint8), (h, w))
    assert kind == "runs"
    pat = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 0], np.uint8)
    return pat[(r * 3 + c) % 10]


def dress(specs, form, ts, mask="random", seed=1):
    """Strided spec dicts -> cimg_window_masked spec dicts in `form` (a key of FORMS, or "mixed": the four forms in turn), with a
    source buffer and a mask buffer.  Source rows lie as _window_writes.source lays them; mask rows start at ODD offsets with an odd
    pitch.  mask: a kind of MASKS, or "cycle": the kinds in turn.
    -> (specs, uint8 source, uint8 masks)"""
    rng = np.random.default_rng(seed)
    forms = list(FORMS)
    out, sat, mat = [], 0, 0
    mparts = []
    for k, s in enumerate(specs):
        s = dict(s)
        s.setdefault("col_pitch", 1)
        f = FORMS[forms[k % 4] if form == "mixed" else form]
        s["flags"] = f
        s["out_off"], s["out_pitch"], s["mask_off"], s["mask_pitch"] = 0, 0, 0, 0
        s["value"] = bytes(rng.integers(0, 256, ts, dtype=np.uint8)) if f & WM_CONST else b""
        if not f & WM_CONST:
            s["out_pitch"] = s["width"] * ts + 5
            s["out_off"] = sat + 1
            sat += 1 + s["out_pitch"] * max(s["height"], 1) + 8
        if f & WM_MASK:
            h, w = s["height"], s["width"]
            s["mask_pitch"] = w + (2 if w & 1 else 3)
            mat += 1 - (mat & 1)                         # odd
            s["mask_off"] = mat
            kind = MASKS[k % len(MASKS)] if mask == "cycle" else mask
            m = np.full((max(h, 1), s["mask_pitch"]), 7, np.uint8)        # (the bytes between rows are set: they must not be read as mask)
            m[:h, :w] = make_mask(kind, h, w, rng)
            mparts.append((mat, m))
            mat += m.size + 4
        out.append(s)
    src = rng.integers(0, 256, sat + 64, dtype=np.uint8)
    masks = np.full(mat + 64, 9, np.uint8)
    for at, m in mparts:
        masks[at:at + m.size] = m.ravel()
    return out, src, masks


def mask_of(s, masks):
    """the (height, width) bool mask of a window (all True without WM_MASK)"""
    h, w = s["height"], s["width"]
    if not s["flags"] & WM_MASK:
        return np.ones((h, w), bool)
    at = s["mask_off"] + np.arange(h)[:, None] * s["mask_pitch"] + np.arange(w)[None, :]
    return masks[at] != 0


def apply(planes, specs, ts, src, masks):
    """planes: {chunk_first: uint8 plane}; np.copyto(view, src_or_value, where=mask), the windows one after the other"""
    planes = {k: v.copy() for k, v in planes.items()}
    for s in specs:
        h, w = s["height"], s["width"]
        if w == 0 or h == 0:
            continue
        pl = planes[s["chunk_first"]]
        px = pl[:pl.size // ts * ts].reshape(-1, ts)
        e = element_index(s)
        if s["flags"] & WM_CONST:
            new = np.broadcast_to(np.frombuffer(s["value"][:ts], np.uint8), (h, w, ts))
        else:
            at = s["out_off"] + np.arange(h)[:, None] * s["out_pitch"] + np.arange(w * ts)[None, :]
            new = src[at].reshape(h, w, ts)
        view = px[e]                                       # (h, w, ts): the window's elements (distinct inside one window)
        np.copyto(view, new, where=mask_of(s, masks)[:, :, None])
        px[e] = view
    return planes


def expected(p, chunks, specs, ts, src, masks, destsize, compress=None, planes=None):
    """-> (the new chunk of every chunk that holds a byte of an element of a window, None for the others; the edited planes)"""
    nb = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8))[0] for c in chunks]
    bs = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8))[2] for c in chunks]
    if planes is None:
        planes = {}
        for s in specs:
            cf, cn = s["chunk_first"], s["chunk_count"]
            if cf not in planes:
                planes[cf] = np.concatenate([O.decompress(c)[1] for c in chunks[cf:cf + cn]])
    edited = apply(planes, specs, ts, src, masks)
    tch = {c for c, _ in S.touched_blocks(specs, nb, bs, ts)}
    want = [None] * len(chunks)
    for s in specs:
        cf, cn = s["chunk_first"], s["chunk_count"]
        off = 0
        for c in range(cf, cf + cn):
            if c in tch and want[c] is None:
                raw = edited[cf][off:off + nb[c]]
                if compress is None:
                    r, b = O.compress(p, raw, destsize=destsize[c])
                    want[c] = b if r > 0 else b""
                else:
                    want[c] = compress(raw, destsize[c])
            off += nb[c]
    return want, edited


def strided_of(specs):
    """the cimg_window_strided fields of masked specs (for the flags == 0 comparison)"""
    keys = ("chunk_first", "chunk_count", "origin", "row_pitch", "col_pitch", "width", "height", "out_off", "out_pitch")
    return [{k: s[k] for k in keys} for s in specs]


def rmw_windows(kind, nchunks=1):
    """The cases that would expose a read-modify-write of unit bytes, for a uint8 plane of one 8 KiB block (ROW = 180).
    columns: two windows on even and odd columns (col_pitch 2, origins 1 apart): every dword of the rows holds bytes of both.
    (The planner's proof is conservative -- the bytes between a row's samples count as written -- so THIS unit runs under the ORDERED
    schedule: the sharing is between lanes of a wave and between the waves of one item, with a barrier between the two windows.)
    rows: two col_pitch 1 windows of odd width on alternating rows: the rows' ends share dwords, and the unit's schedule is disjoint.
    tiles: 50 col_pitch 1 windows 3 bytes wide and 40 rows high, side by side: the DISJOINT schedule (four waves, no barrier, the
    windows dealt round-robin over them) with every dword of the covered area holding bytes of two windows, hence of two waves."""
    R = S.ROW
    if kind == "columns":
        return [S.win(R * 2 + 1, 80, 40, col_pitch=2, nchunks=nchunks), S.win(R * 2 + 2, 80, 40, col_pitch=2, nchunks=nchunks)]
    if kind == "tiles":
        return [S.win(R * 2 + 1 + 3 * k, 3, 40, nchunks=nchunks) for k in range(50)]
    assert kind == "rows"
    return [S.win(R * 2 + 3, 177, 20, row_pitch=2 * R, nchunks=nchunks), S.win(R * 3 + 3, 177, 20, row_pitch=2 * R, nchunks=nchunks)]
