"""Helpers of the window-write tests (test_emu_window_writes.py, test_gpu_window_writes.py): window sources, the expected new chunks
(the windows written into the oracle's decode of the old chunks, in call order, then compressed from scratch), and the cases."""
import numpy as np

import _oracle as O
from _windows import Window, windows  # noqa: F401  (re-exported)

BLOSCLZ, LZ4, LZ4HC, ZSTD = 0, 1, 2, 5


def source(specs, ts, seed=1, fill=None):
    """Give each window an out_off / out_pitch into a fresh source buffer (rows `gap` bytes apart) -> (specs, uint8 source)."""
    rng = np.random.default_rng(seed)
    at, out = 0, []
    for s in specs:
        s = dict(s)
        s.setdefault("out_pitch", s["width"] * ts + 5)
        s["out_off"] = at + 1
        at += 1 + s["out_pitch"] * max(s["height"], 1) + 8
        out.append(s)
    src = rng.integers(0, 256, at + 64, dtype=np.uint8) if fill is None else np.full(at + 64, fill, np.uint8)
    return out, src


def apply(planes, specs, ts, src):
    """planes: {chunk_first: uint8 plane}; the windows written in, one after the other."""
    planes = {k: v.copy() for k, v in planes.items()}
    for s in specs:
        if s["width"] == 0 or s["height"] == 0:
            continue
        pl = planes[s["chunk_first"]]
        rp = s["row_pitch"] if s["height"] > 1 else 0
        wb = s["width"] * ts
        for r in range(s["height"]):
            a = (s["origin"] + r * rp) * ts
            o = s["out_off"] + r * s["out_pitch"]
            pl[a:a + wb] = src[o:o + wb]
    return planes


def touched(nbytes, specs, ts):
    """chunk indices some window row meets"""
    starts = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)
    t = set()
    for s in specs:
        if s["width"] == 0 or s["height"] == 0:
            continue
        cf, cn = s["chunk_first"], s["chunk_count"]
        base = starts[cf]
        rp = s["row_pitch"] if s["height"] > 1 else 0
        for r in range(s["height"]):
            a = base + (s["origin"] + r * rp) * ts
            e = a + s["width"] * ts
            for c in range(cf, cf + cn):
                if starts[c] < e and starts[c + 1] > a and nbytes[c] > 0:
                    t.add(c)
    return t


def expected(p, chunks, specs, ts, src, destsize, compress=None):
    """the new chunk of every touched chunk (None for the others): the edited pixels compressed from scratch (the oracle, or
    `compress(raw_bytes, destsize)` for codecs without a byte-exact oracle)"""
    nb = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8))[0] for c in chunks]
    firsts = sorted({s["chunk_first"] for s in specs})
    planes = {}
    for s in specs:
        cf, cn = s["chunk_first"], s["chunk_count"]
        planes[cf] = np.concatenate([O.decompress(c)[1] for c in chunks[cf:cf + cn]])
    edited = apply(planes, specs, ts, src)
    want = [None] * len(chunks)
    tch = touched(np.array(nb), specs, ts)
    for s in specs:
        cf, cn = s["chunk_first"], s["chunk_count"]
        off = 0
        for c in range(cf, cf + cn):
            if c in tch:
                raw = edited[cf][off:off + nb[c]]
                if compress is None:
                    r, b = O.compress(p, raw, destsize=destsize[c])
                    want[c] = b if r > 0 else b""
                else:
                    want[c] = compress(raw, destsize[c])
            off += nb[c]
    assert firsts
    return want, edited
