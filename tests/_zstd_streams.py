"""Spec-built Zstandard frames (RFC 8878) and the buffers they are defined to produce: the zstd counterpart of tests/_streams.py.

Test infrastructure for test_emu_zstd_streams.py (CPU) and test_gpu_zstd_streams.py (-m gpu).  It shares no code with csrc/ or
oracle/: a frame is a list of blocks (raw, RLE, compressed), a compressed block is a list of (literals, offset, match length)
sequences with ACTUAL offsets plus choices of encoding, and the expected output is _streams.run_sequences over the concatenated
sequences and nothing else.  The writer below puts the blocks down as the format description says:

  bits      forward streams (FSE table descriptions) and backward ones (a final 1 bit closes them; the reader starts there)
  FSE       normalised counts -> decoding table (the spec's spread, "less than 1" symbols placed last); the encoder is derived from
            that table (going backwards: the state of the symbol that holds the successor's state number); the description writer
            knows -1 probabilities and the 2-bit zero-run flags with chained 3s
  Huffman   weights -> codes; direct weights (header byte >= 128) and FSE-compressed weights (two interleaved states); one stream
            and four streams behind the 6-byte jump table
  literals  raw / RLE with 1-, 2- and 3-byte headers; compressed with the four size formats; treeless
  sequences the count in 1, 2 or 3 bytes; every table Predefined, RLE, FSE-described or Repeat; codes and extra bits; the writer keeps
            its own repeat-offset history, emits a repeat code where a sequence asks for one (with the shifted meaning at literal
            length 0 and "rep1 - 1") and asserts that the code resolves to the sequence's actual offset
  frame     single-segment with a content size of 1, 2 (minus 256), 4 or 8 bytes, window descriptor with and without content size,
            content checksum (XXH64, written out below)

Everything is generated from seeds: the CPU and the GPU leg build identical bytes (tests/golden/zstd_streams_digests.json holds
the sha256 of every frame, written after libzstd accepted them all).
"""
import hashlib

import numpy as np

import _streams as S

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 131072
LL_PREDEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_PREDEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_PREDEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
PREDEF = {"ll": (LL_PREDEF, 6), "of": (OF_PREDEF, 5), "ml": (ML_PREDEF, 6)}
MAXLOG = {"ll": 9, "of": 8, "ml": 9}
NSYM = {"ll": 36, "of": 32, "ml": 53}
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _code(base, v):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c


def ll_code(v):
    return _code(LL_BASE, v)


def ml_code(v):
    return _code(ML_BASE, v)


# ---- bit writers ----------------------------------------------------------------------------------------------------------------
class Bits:
    """bits appended LSB first.  forward(): padded with zeros to a byte; backward(): closed with a 1 bit (the reader starts below it)"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def add(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        self.acc |= v << self.n
        self.n += nb

    def forward(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")

    def backward(self):
        return (self.acc | (1 << self.n)).to_bytes((self.n + 8) // 8, "little")


# ---- FSE ------------------------------------------------------------------------------------------------------------------------
def fse_table(norm, log):
    """normalised counts -> [(symbol, bits, baseline)] per state (RFC 8878 4.1.1)"""
    size = 1 << log
    assert sum(abs(p) for p in norm) == size, (sum(abs(p) for p in norm), size)
    sym = [None] * size
    high = size
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            sym[high] = s
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and None not in sym
    nxt = [1 if p == -1 else p for p in norm]
    table = []
    for st in range(size):
        s = sym[st]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


class FseEncoder:
    """The decoding table read backwards: the states of a symbol partition the state numbers by [baseline, baseline + 2^bits)."""

    def __init__(self, table, log):
        self.log, self.table = log, table
        self.by_sym = {}
        for st, (s, nb, base) in enumerate(table):
            self.by_sym.setdefault(s, []).append((base, nb, st))
        for v in self.by_sym.values():
            v.sort()

    def first(self, s, want_bits=False):
        """a state for the LAST symbol of a stream (nothing follows it); want_bits: one whose successor would cost bits"""
        for base, nb, st in self.by_sym[s]:
            if nb > 0 or not want_bits:
                return st
        raise AssertionError("every state of symbol %d is free" % s)

    def before(self, s, succ):
        """-> (state of symbol s that leads to state succ, value, bits to write)"""
        for base, nb, st in self.by_sym[s]:
            if base <= succ < base + (1 << nb):
                return st, succ - base, nb
        raise AssertionError("no state of symbol %d reaches %d" % (s, succ))


def rle_table(s):
    return [(s, 0, 0)]


def fse_description(norm, log):
    """the table description (RFC 8878 4.1.1): trailing zero probabilities are not written"""
    b = Bits()
    b.add(log - 5, 4)
    remaining = 1 << log
    s = 0
    while remaining > 0:
        p = norm[s]
        value = p + 1
        bits = (remaining + 1).bit_length()
        lower = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if value < threshold:
            b.add(value, bits - 1)
        elif value <= lower:
            b.add(value, bits)
        else:
            b.add(value + threshold, bits)
        remaining -= abs(p)
        s += 1
        if p == 0:
            run = 0
            while s + run < len(norm) and norm[s + run] == 0:
                run += 1
            assert s + run < len(norm), "a zero run ends in a used symbol"
            s += run
            while run >= 3:
                b.add(3, 2)
                run -= 3
            b.add(run, 2)
    assert remaining == 0 and all(p == 0 for p in norm[s:])
    return b.forward()


def normalise(counts, log, minus_one=()):
    """counts per symbol -> normalised counts summing to 2^log: every used symbol at least 1, those in minus_one "less than 1" """
    size = 1 << log
    norm = [0] * len(counts)
    used = [s for s, c in enumerate(counts) if c > 0]
    for s in minus_one:
        assert counts[s] > 0
        norm[s] = -1
    rest = [s for s in used if s not in minus_one]
    room = size - len(minus_one)
    total = sum(counts[s] for s in rest)
    assert rest and room >= len(rest), "table too small for its symbols"
    for s in rest:
        norm[s] = max(1, counts[s] * room // total)
    big = max(rest, key=lambda s: norm[s])
    while sum(abs(p) for p in norm) > size:                   # (the floor of 1 can overshoot: take from the largest in turn)
        big = max(rest, key=lambda s: norm[s])
        assert norm[big] > 1
        norm[big] -= 1
    norm[big] += size - sum(abs(p) for p in norm)
    assert norm[big] < size, "one symbol alone is RLE mode's business"
    return norm


# ---- Huffman --------------------------------------------------------------------------------------------------------------------
def huf_codes(weights):
    """weights of symbols 0 .. len-1 (0: unused) -> ({symbol: (code, bits)}, max bits) (RFC 8878 4.2.1)"""
    total = sum(1 << (w - 1) for w in weights if w)
    maxbits = total.bit_length() - 1
    assert total == 1 << maxbits and 1 <= maxbits <= 16, "weights do not fill a tree"
    codes, cursor = {}, 0
    for w in range(1, maxbits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (cursor >> (w - 1), maxbits + 1 - w)
                cursor += 1 << (w - 1)
    assert cursor == total
    return codes, maxbits


def huf_weights_for(data, maxbits=11):
    """weights of a complete prefix code over the bytes in data (at least two different ones), no code longer than maxbits"""
    counts = np.bincount(np.frombuffer(bytes(data), np.uint8), minlength=256)
    used = [int(s) for s in np.nonzero(counts)[0]]
    assert len(used) >= 2
    total = int(counts.sum())
    ln = {s: min(maxbits, max(1, int(np.ceil(-np.log2(counts[s] / total))))) for s in used}
    full = 1 << maxbits
    kraft = lambda: sum(1 << (maxbits - l) for l in ln.values())
    for s in sorted(used, key=lambda s: counts[s]):          # too full: the rarest symbols get longer codes
        while kraft() > full and ln[s] < maxbits:
            ln[s] += 1
    assert kraft() <= full
    while kraft() < full:                                      # room left: shorten, longest codes first (the gap is a multiple of theirs)
        gap = full - kraft()
        for s in sorted(used, key=lambda s: (-ln[s], -counts[s])):
            if ln[s] > 1 and (1 << (maxbits - ln[s])) <= gap:
                ln[s] -= 1
                break
        else:
            raise AssertionError("cannot complete the code")
    if len(used) > 129 and len(set(ln.values())) == 1:         # (more than 128 equal weights have no description: one code shorter, two longer)
        order = sorted(used, key=lambda s: counts[s])
        ln[order[-1]] -= 1
        ln[order[0]] += 1
        ln[order[1]] += 1
    top = max(ln.values())
    w = [0] * (max(used) + 1)
    for s in used:
        w[s] = top + 1 - ln[s]
    return w


def huf_tree_description(weights, how):
    """the tree description: every weight but the last used symbol's, direct (4 bits each) or FSE-compressed"""
    last = max(s for s, w in enumerate(weights) if w)
    listed = list(weights[:last])
    others = sum(1 << (w - 1) for w in listed if w)
    maxbits = others.bit_length()
    left = (1 << maxbits) - others
    assert left == 1 << (weights[last] - 1), "the last weight is not the one the others imply"
    if how == "auto":
        how = "direct" if len(listed) <= 128 else "fse"
    if how == "direct":
        assert 1 <= len(listed) <= 128
        vals = listed + [0] * (len(listed) & 1)
        return bytes([127 + len(listed)]) + bytes((vals[i] << 4) | vals[i + 1] for i in range(0, len(vals), 2))
    log = how[1] if isinstance(how, tuple) else 6
    counts = [0] * (max(listed) + 1)
    for w in listed:
        counts[w] += 1
    norm = normalise(counts, log)
    enc = FseEncoder(fse_table(norm, log), log)
    n = len(listed)
    assert n >= 2
    # weight i belongs to state i & 1; the last two weights are what the final states hold, and the update behind weight n - 2
    # must ask for bits that are not there (that is how the reader learns that the stream is over)
    state = {(n - 1) & 1: enc.first(listed[n - 1], True), (n - 2) & 1: enc.first(listed[n - 2], True)}
    b = Bits()
    for i in range(n - 3, -1, -1):
        st, v, nb = enc.before(listed[i], state[i & 1])
        b.add(v, nb)
        state[i & 1] = st
    b.add(state[1], log)
    b.add(state[0], log)
    body = fse_description(norm, log) + b.backward()
    assert len(body) < 128, "compressed weights take %d bytes" % len(body)
    return bytes([len(body)]) + body


def huf_stream(data, codes):
    b = Bits()
    for s in reversed(bytes(data)):
        c, nb = codes[s]
        b.add(c, nb)
    return b.backward()


def huf_streams(data, codes, streams):
    if streams == 1:
        return huf_stream(data, codes)
    per = (len(data) + 3) // 4
    parts = [huf_stream(data[k * per:(k + 1) * per] if k < 3 else data[3 * per:], codes) for k in range(4)]
    assert 3 * per <= len(data) and all(len(p) < 65536 for p in parts[:3])
    return b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)


# ---- XXH64 (the content checksum is its low four bytes) ---------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, lane):
    return (_rotl((acc + lane * _P2) & _M, 31) * _P1) & _M


def _merge(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        words = np.frombuffer(data[:n // 32 * 32], "<u8").reshape(-1, 4).tolist()
        for row in words:
            v = [_round(a, w) for a, w in zip(v, row)]
        p = n // 32 * 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for a in v:
            h = _merge(h, a)
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & _M), 11) * _P1) & _M
        p += 1
    h = ((h ^ (h >> 33)) * _P2) & _M
    h = ((h ^ (h >> 29)) * _P3) & _M
    return h ^ (h >> 32)


# ---- the frame writer -------------------------------------------------------------------------------------------------------------
def literals_header(kind, regen, comp=None, size_format=None, streams=1):
    """kind 0 raw, 1 RLE, 2 compressed, 3 treeless.  size_format: bytes of a raw / RLE header (1, 2, 3); for coded literals the
    format number 0 .. 3 (one stream / 10 bits; four streams / 10, 14, 18 bits)"""
    if kind < 2:
        sf = size_format or (1 if regen < 32 else 2 if regen < 4096 else 3)
        if sf == 1:
            assert regen < 32
            return bytes([kind | (regen << 3)])
        if sf == 2:
            assert regen < 4096
            return (kind | (1 << 2) | (regen << 4)).to_bytes(2, "little")
        assert regen < (1 << 20)
        return (kind | (3 << 2) | (regen << 4)).to_bytes(3, "little")
    if size_format is None:
        size_format = 0 if streams == 1 else 1 if max(regen, comp) < 1024 else 2 if max(regen, comp) < 16384 else 3
    assert (size_format == 0) == (streams == 1)
    bits = (10, 10, 14, 18)[size_format]
    assert regen < (1 << bits) and comp < (1 << bits), (regen, comp, size_format)
    return (kind | (size_format << 2) | (regen << 4) | (comp << (4 + bits))).to_bytes((3, 3, 4, 5)[size_format], "little")


class Frame:
    """Blocks appended one by one; the writer carries what the format carries from block to block: the three FSE tables, the Huffman
    tree and the repeat offsets."""

    def __init__(self):
        self.blocks = []                  # (type, body, regenerated size)
        self.seqs = []                    # every sequence of the frame, for run_sequences
        self.rep = [1, 4, 8]
        self.tables = {}                  # kind -> (FseEncoder, log)
        self.huf = None                   # codes of the last tree
        self.pos = 0

    # -- blocks that carry no entropy state
    def raw(self, data):
        data = bytes(data)
        self.blocks.append((0, data, len(data)))
        self.seqs.append((data, 0, 0))
        self.pos += len(data)
        return self

    def rle(self, byte, n):
        self.blocks.append((1, bytes([byte]), n))
        self.seqs.append((bytes([byte]) * n, 0, 0))
        self.pos += n
        return self

    # -- a compressed block
    def _literals(self, lits, how, size_format, streams, weights, tree):
        if how == "raw":
            return literals_header(0, len(lits), size_format=size_format) + lits
        if how == "rle":
            assert len(lits) >= 1 and lits == lits[:1] * len(lits)
            return literals_header(1, len(lits), size_format=size_format) + lits[:1]
        if how == "huf":
            w = weights if weights is not None else huf_weights_for(lits)
            self.huf, _ = huf_codes(w)
            desc = huf_tree_description(w, tree)
        else:
            assert how == "treeless" and self.huf is not None
            desc = b""
        body = desc + huf_streams(lits, self.huf, streams)
        return literals_header(2 if how == "huf" else 3, len(lits), len(body), size_format, streams) + body

    def _offset_value(self, off, ll, rep):
        """the offset value a sequence is coded with, and the history it leaves"""
        r = self.rep
        if rep == "auto":
            rep = 0
            cand = [r[0], r[1], r[2]] if ll else [r[1], r[2], r[0] - 1]
            for k, c in enumerate(cand):
                if c == off and c > 0:
                    rep = k + 1
                    break
        if not rep:
            self.rep = [off, r[0], r[1]]
            return off + 3
        idx = rep + (0 if ll else 1)
        got = r[idx - 1] if idx <= 3 else r[0] - 1
        assert got == off, "repeat code %d at literal length %d is %d, the sequence's offset is %d" % (rep, ll, got, off)
        if idx == 2:
            self.rep = [r[1], r[0], r[2]]
        elif idx == 3:
            self.rep = [r[2], r[0], r[1]]
        elif idx == 4:
            self.rep = [r[0] - 1, r[0], r[1]]
        return rep

    def _table(self, kind, mode, codes):
        """-> (mode number, bytes in the section header, encoder)"""
        if mode == "predef":
            norm, log = PREDEF[kind]
            enc = FseEncoder(fse_table(norm, log), log)
            self.tables[kind] = enc
            return 0, b"", enc
        if mode == "rle":
            assert len(set(codes)) == 1, "RLE mode: one code for every sequence"
            enc = FseEncoder(rle_table(codes[0]), 0)
            self.tables[kind] = enc
            return 1, bytes([codes[0]]), enc
        if mode == "repeat":
            return 3, b"", self.tables[kind]
        if mode[0] == "fse?":                                   # (described where the block has two codes to describe)
            return self._table(kind, "rle" if len(set(codes)) == 1 else ("fse",) + tuple(mode[1:]), codes)
        assert mode[0] == "fse"
        log = mode[1]
        if len(mode) > 2 and isinstance(mode[2], list):
            norm = mode[2]
        else:
            counts = [0] * NSYM[kind]
            for c in codes:
                counts[c] += 1
            for c in (mode[3] if len(mode) > 3 else ()):        # symbols the table describes and no sequence uses
                counts[c] += 1
            norm = normalise(counts, log, tuple(mode[2]) if len(mode) > 2 else ())
        assert 5 <= log <= MAXLOG[kind]
        enc = FseEncoder(fse_table(norm, log), log)
        self.tables[kind] = enc
        return 2, fse_description(norm, log), enc

    def block(self, seqs, tail=b"", lits="raw", lit_format=None, streams=None, weights=None, tree="auto",
              ll="predef", of="predef", ml="predef", nseq_form=None, junk_bits=0):
        """seqs: (literals, offset, match length) or (literals, offset, match length, repeat code 1 .. 3 / "auto")"""
        seqs = [tuple(s) + (0,) * (4 - len(s)) for s in seqs]
        tail = bytes(tail)
        all_lits = b"".join(bytes(s[0]) for s in seqs) + tail
        if streams is None:                                     # (one stream has the 10-bit size format only)
            streams = 1 if len(all_lits) < 1024 else 4
        body = bytearray(self._literals(all_lits, lits, lit_format, streams, weights, tree))
        n = len(seqs)
        if nseq_form is None:
            nseq_form = 1 if n < 128 else 2 if n < 0x7F00 else 3
        if nseq_form == 1:
            assert n < 128
            body.append(n)
        elif nseq_form == 2:
            assert n < 0x7F00
            body += bytes([128 + (n >> 8), n & 255])
        else:
            assert n >= 0x7F00
            body += b"\xff" + (n - 0x7F00).to_bytes(2, "little")
        regen = len(tail)
        if n:
            vals = []
            for lit, off, mlen, rep in seqs:
                llen = len(lit)
                assert mlen >= 3
                ov = self._offset_value(off, llen, rep)
                vals.append((llen, ll_code(llen), mlen, ml_code(mlen), ov, ov.bit_length() - 1))
                regen += llen + mlen
            modes = [self._table(k, m, [v[i] for v in vals]) for k, m, i in (("ll", ll, 1), ("of", of, 5), ("ml", ml, 3))]
            self.modes_at = len(body)                           # (of the last block written: the negative cases patch bytes there)
            body.append((modes[0][0] << 6) | (modes[1][0] << 4) | (modes[2][0] << 2))
            for _, desc, _ in modes:
                body += desc
            el, eo, em = modes[0][2], modes[1][2], modes[2][2]
            b = Bits()
            b.add(0, junk_bits)                                 # (invalid on purpose: bits nobody reads at the bottom of the stream)
            sl = so = sm = None
            for i in range(n - 1, -1, -1):
                llen, lc, mlen, mc, ov, oc = vals[i]
                if i == n - 1:
                    sl, so, sm = el.first(lc), eo.first(oc), em.first(mc)
                else:
                    so, v, nb = eo.before(oc, so)
                    b.add(v, nb)
                    sm, v, nb = em.before(mc, sm)
                    b.add(v, nb)
                    sl, v, nb = el.before(lc, sl)
                    b.add(v, nb)
                b.add(llen - LL_BASE[lc], LL_BITS[lc])
                b.add(mlen - ML_BASE[mc], ML_BITS[mc])
                b.add(ov - (1 << oc), oc)
            b.add(sm, em.log)
            b.add(so, eo.log)
            b.add(sl, el.log)
            body += b.backward()
        assert regen <= BLOCK_MAX and len(body) < BLOCK_MAX, (regen, len(body))
        self.blocks.append((2, bytes(body), regen))
        self.seqs += [(bytes(s[0]), s[1], s[2]) for s in seqs] + [(tail, 0, 0)]
        self.pos += regen
        return self

    def finish(self, single=True, fcs_bytes=None, checksum=False, window_log=None, fcs=None, fhd_or=0, last=True, invalid=False):
        """-> (frame bytes, expected output as a uint8 array).  invalid: the sequences cannot be run (a negative case): the
        expected output is `pos` zero bytes"""
        want = np.zeros(self.pos, np.uint8) if invalid else S.run_sequences(self.seqs)
        n = want.size if fcs is None else fcs
        assert want.size == self.pos
        if single:
            fcs_bytes = fcs_bytes or (1 if n < 256 else 2 if n < 65536 + 256 else 4)
            flag = {1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
            head = bytes([(flag << 6) | 0x20 | (4 if checksum else 0) | fhd_or])
        else:
            fcs_bytes = fcs_bytes or 0
            flag = {0: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
            wl = window_log or max(10, int(max(want.size, 1) - 1).bit_length())
            head = bytes([(flag << 6) | (4 if checksum else 0) | fhd_or, (wl - 10) << 3])
        if fcs_bytes == 2:
            assert 256 <= n < 65536 + 256
            head += (n - 256).to_bytes(2, "little")
        elif fcs_bytes:
            head += n.to_bytes(fcs_bytes, "little")
        out = bytearray(MAGIC + head)
        blocks = self.blocks or [(0, b"", 0)]
        self.block_at = []                                      # where every block's body begins in the frame
        for k, (typ, body, regen) in enumerate(blocks):
            size = len(body) if typ != 1 else regen
            self.block_at.append(len(out) + 3)
            out += ((1 if last and k == len(blocks) - 1 else 0) | (typ << 1) | (size << 3)).to_bytes(3, "little")
            out += body
        if checksum:
            out += (xxh64(want.tobytes()) & 0xFFFFFFFF).to_bytes(4, "little")
        return bytes(out), want


# ---- sequence sources -----------------------------------------------------------------------------------------------------------
def _text(rng, n, nsym=40, skew=1.3, syms=None):
    """n bytes over nsym symbols with a skewed distribution (what Huffman coding pays for)"""
    p = 1.0 / np.arange(1, nsym + 1) ** skew
    syms = rng.permutation(256)[:nsym].astype(np.uint8) if syms is None else syms
    return syms[rng.choice(nsym, n, p=p / p.sum())].tobytes()


class ZB(S.Builder):
    """_streams.Builder for zstd: matches from 3 bytes, offsets as far as the output reaches; the literal source can be text"""

    def __init__(self, rng, text=False):
        S.Builder.__init__(self, rng, S.LZ4)
        self.min_ml, self.max_off, self.text = 3, 1 << 30, text
        self.syms = rng.permutation(256)[:40].astype(np.uint8)

    def lit(self, n=None, data=None):
        if data is None and self.text:
            data = _text(self.rng, n, syms=self.syms)
        return S.Builder.lit(self, n, data)


def split_blocks(seqs, limit=BLOCK_MAX):
    """a sequence list -> [(seqs of the block, literals behind its last match)], every block regenerating at most `limit` bytes
    (the first blocks as full as whole sequences make them; a literal run is cut where a block ends)"""
    out, cur, size = [], [], 0
    for lit, off, ml in seqs:
        lit = bytes(lit)
        while size + len(lit) + ml > limit:
            room = min(len(lit), limit - size)
            out.append((cur, lit[:room]))
            lit, cur, size = lit[room:], [], 0
        if ml:
            cur.append((lit, off, ml, "auto"))
            size += len(lit) + ml
        else:
            out.append((cur, lit))
            cur, size = [], 0
    if cur:
        out.append((cur, b""))
    return out


def frame_of(seqs, style=0, **finish):
    """A sequence list (as _streams.Builder leaves it) as a frame.  style picks the encodings: 0 raw literals / predefined tables,
    1 Huffman literals (four streams from 1 KiB) / described tables, 2 the same with treeless literals and repeated tables from
    the second block on"""
    f = Frame()
    for k, (bseqs, tail) in enumerate(split_blocks(seqs)):
        lits = b"".join(s[0] for s in bseqs) + tail
        if not bseqs and len(set(lits)) <= 1 and len(lits) > 0 and style == 0:
            f.rle(lits[0], len(lits))
            continue
        if not bseqs and not lits:
            continue
        kw = {}
        if style and len(set(lits)) >= 2 and len(lits) >= 6:
            again = style == 2 and f.huf is not None and set(lits) <= set(f.huf)
            w = huf_weights_for(lits)
            listed = w[:max(s for s, x in enumerate(w) if x)]
            tree = "fse" if len(set(listed)) >= 2 and (k % 2 or len(listed) > 128) else "direct"
            kw.update(lits="treeless" if again else "huf", streams=4 if len(lits) >= 1024 else 1, tree=tree, weights=None if again else w)
        if style and len(bseqs) >= 8:
            codes = {"ll": {ll_code(len(s[0])) for s in bseqs}, "ml": {ml_code(s[2]) for s in bseqs}}
            for kind in ("ll", "ml"):
                # (Repeat mode needs every code of this block in the table the last block left)
                if style == 2 and kind in f.tables and codes[kind] <= set(f.tables[kind].by_sym):
                    kw[kind] = "repeat"
                else:
                    kw[kind] = "rle" if len(codes[kind]) == 1 else ("fse", 7 + k % 3)
            kw["of"] = "predef" if style == 1 else ("fse", 6 + k % 3)
        f.block(bseqs, tail, **kw)
    return f.finish(**finish)


def random_frame(rng, n, style=0, text=None, **finish):
    b = ZB(rng, text=bool(style) if text is None else text)
    b.lit(int(rng.integers(1, 9)))
    b.random(n - 1, lit_scale=2.0 if style else 1.0)
    seqs, ref = b.finish(n)
    frame, want = frame_of(seqs, style, **finish)
    assert np.array_equal(want, ref)
    return frame, want


# ---- the named cases ------------------------------------------------------------------------------------------------------------
FRAME_A = bytes.fromhex("28b52ffd200e" "5c0000" "2061626364" "01" "54" "040200" "07" "450000" "207778797a" "01" "fc" "07")
FRAME_B = bytes.fromhex("28b52ffd200e" "5c0000" "2061626364" "01" "54" "040200" "07" "5d0000" "207778797a" "01" "54" "040200" "07")
FRAME_C = bytes.fromhex("28b52ffd200b" "5c0000" "2061626364" "01" "54" "040200" "07" "350000" "207778797a" "00")
TAILS = (1, 15, 16, 17, 33)


class Hist:
    """The repeat offsets as the case generators track them (on their own: the writer asserts that its history agrees)."""

    def __init__(self):
        self.r = [1, 4, 8]

    def new(self, off):
        self.r = [off, self.r[0], self.r[1]]
        return off

    def peek(self, code, ll):
        idx = code + (0 if ll else 1)
        return self.r[idx - 1] if idx <= 3 else self.r[0] - 1

    def rep(self, code, ll):
        off = self.peek(code, ll)
        idx = code + (0 if ll else 1)
        if idx > 1:
            rest = [x for k, x in enumerate(self.r) if k != idx - 1] if idx <= 3 else self.r[:2]
            self.r = [off] + rest[:2]
        return off


def _syms_for(rng, weights, n):
    """n literal bytes over the symbols of a weight list, likely ones more often; every symbol at least once when n allows"""
    syms = np.array([s for s, w in enumerate(weights) if w], np.uint8)
    p = np.array([float(1 << (weights[s] - 1)) for s in syms])
    out = syms[rng.choice(syms.size, n, p=p / p.sum())]
    k = min(n, syms.size)
    out[rng.permutation(n)[:k]] = syms[:k]
    return out.tobytes()


def full_block_seqs(rng, n=BLOCK_MAX, text=False):
    b = ZB(rng, text=text)
    b.lit(7).random(n - 1)
    seqs, _ = b.finish(n)
    return [(l, o, m, "auto") for l, o, m in seqs[:-1]], seqs[-1][0]


def _small_seqs(rng, f, count, hist=None, ll_choices=(0, 1, 2, 3, 5), ml_hi=9):
    """count short sequences against the frame's output so far (new offsets only)"""
    out, pos = [], f.pos
    for _ in range(count):
        ll = int(rng.choice(ll_choices)) if pos else 1 + int(rng.integers(0, 3))
        ml = int(rng.integers(3, ml_hi))
        pos += ll
        off = int(rng.integers(1, min(pos, 300) + 1))
        if hist is not None:
            hist.new(off)
        out.append((rng.integers(0, 256, ll, dtype=np.uint8).tobytes(), off, ml))
        pos += ml
    return out


def block_structure_cases(rng):
    out = [("frame_A", FRAME_A, np.frombuffer(b"abcdabcwxyzwxy", np.uint8)), ("frame_B", FRAME_B, np.frombuffer(b"abcdabcwxyzwxy", np.uint8)),
           ("frame_C", FRAME_C, np.frombuffer(b"abcdabcwxyz", np.uint8))]
    # the writer's own A, B and C are the bytes above
    f = Frame().block([(b"abcd", 4, 3)], ll="rle", of="rle", ml="rle").block([(b"wxyz", 4, 3)], ll="repeat", of="repeat", ml="repeat")
    assert f.finish()[0] == FRAME_A
    f = Frame().block([(b"abcd", 4, 3)], ll="rle", of="rle", ml="rle").block([(b"wxyz", 4, 3)], ll="rle", of="rle", ml="rle")
    assert f.finish()[0] == FRAME_B
    f = Frame().block([(b"abcd", 4, 3)], ll="rle", of="rle", ml="rle").block([], b"wxyz")
    assert f.finish()[0] == FRAME_C
    # a short last block behind a full one (a compressed block with sequences regenerates at least 3 bytes: 3 and 7 stand in for 1)
    for style in (0, 1):
        seqs, tail = full_block_seqs(rng, text=bool(style))
        enc = dict(lits="huf", streams=4, tree="fse", ll=("fse", 8), of=("fse", 7), ml=("fse", 8)) if style else {}
        for t in (3, 7) + TAILS[1:]:
            f = Frame().block(seqs, tail, **enc)
            lit = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            if t < 13:
                f.block([(lit(t - 3), 5, 3)])
            else:
                a = (t - 7) // 2
                f.block([(lit(4), 4, 3), (lit(a), int(rng.integers(1, 2000)), t - 7 - a)], ll="predef" if style else "rle" if a == 4 else "predef")
            out.append(("tail_seq%d_s%d" % (t, style),) + f.finish())
        for t in TAILS:
            lit = rng.integers(0, 256, t, dtype=np.uint8).tobytes()
            out.append(("tail_lits%d_s%d" % (t, style),) + Frame().block(seqs, tail, **enc).block([], lit).finish())
            out.append(("tail_raw%d_s%d" % (t, style),) + Frame().block(seqs, tail, **enc).raw(lit).finish())
            out.append(("tail_rle%d_s%d" % (t, style),) + Frame().block(seqs, tail, **enc).rle(0x5C, t).finish())
            if t > 1:
                out.append(("tail_rlelits%d_s%d" % (t, style),) + Frame().block(seqs, tail, **enc).block([], bytes([7]) * t, lits="rle").finish())
    out.append(("block_128k",) + Frame().block(seqs, tail).finish())
    # raw and RLE blocks between compressed ones: tables, tree and repeat offsets survive them
    f = Frame()
    b = ZB(rng, text=True)
    b.lit(600).random(3000)
    s1, _ = b.finish(3100)
    h = Hist()
    first = [(l, o, m) for l, o, m in s1[:-1]]
    for l, o, m in first:
        h.new(o)
    w = huf_weights_for(b"".join(s[0] for s in s1))
    f.block(first, s1[-1][0], lits="huf", weights=w, tree="fse", ll=("fse", 7), of=("fse", 6), ml=("fse", 7))
    f.raw(rng.integers(0, 256, 100, dtype=np.uint8).tobytes()).rle(0xEE, 300)
    again = []
    for k in range(len(first)):
        l, _, m = first[k]
        ll = len(l)
        code = 1 + k % 3
        off = h.peek(code, ll)
        if k % 4 == 0 and 0 < off:
            again.append((l, h.rep(code, ll), m, code))
        else:
            again.append((l, h.new(first[k][1]), m))
    f.block(again, b"", lits="treeless", ll="repeat", of=("fse", 6, (), (0, 1)), ml="repeat")
    out.append(("raw_rle_between",) + f.finish())
    # eight small blocks
    f = Frame()
    for k in range(8):
        if k == 3:
            f.raw(b"0123456789")
        elif k == 5:
            f.rle(k, 33)
        else:
            f.block(_small_seqs(rng, f, 1 + 9 * k), bytes(rng.integers(0, 256, k, dtype=np.uint8)),
                    **(dict(ll=("fse", 6), of=("fse", 5), ml=("fse", 6)) if k in (2, 6) else dict(ll="repeat", ml="repeat") if k == 7 else {}))
    out.append(("eight_blocks",) + f.finish())
    out.append(("empty",) + Frame().finish())
    out.append(("only_raw",) + Frame().raw(rng.integers(0, 256, 777, dtype=np.uint8).tobytes()).finish())
    out.append(("only_rle",) + Frame().rle(0xC3, 40000).finish())
    return out


def count_cases(rng):
    out = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        for style in (0, 1):
            f = Frame()
            f.block(_small_seqs(rng, f, n), bytes(rng.integers(0, 256, 5, dtype=np.uint8)),
                    **(dict(ll=("fse", 6), of=("fse", 6), ml=("fse", 5)) if style and n >= 8 else {}))
            out.append(("nseq%d_s%d" % (n, style),) + f.finish())
    f = Frame()
    f.block(_small_seqs(rng, f, 100), nseq_form=2)                      # (the two-byte form is valid below 128 as well)
    out.append(("nseq100_two_bytes",) + f.finish())
    # the three-byte form: 0x7F00 sequences and more in one block (match length 3, literal length 0 - 1)
    f = Frame()
    seqs, pos = [], 0
    for k in range(0x7F00 + 37):
        ll = 1 if k == 0 else k & 1
        pos += ll
        seqs.append((bytes([k & 255] * ll), 1 + int(rng.integers(0, min(pos, 9))), 3, "auto"))
        pos += 3
    f.block(seqs, b"xy", ll=("fse", 5), of=("fse", 5), ml="rle")
    out.append(("nseq_three_bytes",) + f.finish())
    return out


def repeat_cases(rng):
    out = []
    lit = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for code in (1, 2, 3):
        for ll0 in (False, True):
            f, h = Frame(), Hist()
            f.block([(lit(16), h.new(7), 5), (lit(3), h.new(12), 4), (lit(2), h.new(3), 3)])
            for blk in range(2):
                seqs = []
                count = 130 if blk == 0 else 3
                for k in range(count):
                    ll = 0 if ll0 else 1 + k % 4
                    if k in (0, 63, 64, count - 1) and h.peek(code, ll) > 0:
                        seqs.append((lit(ll), h.rep(code, ll), 3 + k % 5, code))
                    else:
                        seqs.append((lit(1 + k % 3), h.new(int(rng.integers(2, 30))), 3 + k % 4))
                assert sum(len(s) == 4 for s in seqs) >= (4 if blk == 0 else 2)
                f.block(seqs, lit(blk), **(dict(ll=("fse", 6), of=("fse", 5), ml=("fse", 6)) if code == 2 and blk == 0 else {}))
            out.append(("rep%d_%s" % (code, "ll0" if ll0 else "lit"),) + f.finish())
    # 70 repeat codes in a row
    f, h = Frame(), Hist()
    seqs = [(lit(20), h.new(9), 4), (lit(1), h.new(14), 4), (lit(1), h.new(5), 4)]
    for k in range(70):
        ll = (0, 2, 0, 1, 5)[k % 5]
        code = 1 + (k * 7 + k // 3) % 3
        if h.peek(code, ll) <= 0:
            code = 1 if ll else 2
        seqs.append((lit(ll), h.rep(code, ll), 3 + k % 9, code))
    f.block(seqs, b"end")
    out.append(("rep_run70",) + f.finish())
    # the initial history 1, 4, 8 used directly
    f, h = Frame(), Hist()
    f.raw(lit(16))
    f.block([(lit(2), h.rep(3, 2), 5, 3), (lit(1), h.rep(3, 1), 6, 3), (b"", h.rep(1, 0), 4, 1), (lit(3), h.rep(1, 3), 7, 1)], ll="predef")
    out.append(("rep_initial_history",) + f.finish())
    return out


def length_cases(rng):
    out = []
    lls = sorted({v for c in range(36) for v in (LL_BASE[c], LL_BASE[c] + (1 << LL_BITS[c]) - 1) if v <= 65536})
    mls = sorted({v for c in range(53) for v in (ML_BASE[c], ML_BASE[c] + (1 << ML_BITS[c]) - 1) if v <= 65539})
    pairs = [(lls[k % len(lls)], mls[-1 - k % len(mls)]) for k in range(max(len(lls), len(mls)))]
    assert {ll_code(a) for a, _ in pairs} == set(range(36)) and {ml_code(b) for _, b in pairs} == set(range(53))
    for name, enc in (("predef", {}), ("fse9", dict(ll=("fse?", 9), of=("fse?", 5), ml=("fse?", 9)))):
        f = Frame()
        cur, size = [], 0
        for a, b in pairs:
            if size + a + b > BLOCK_MAX:
                f.block(cur, **enc)
                cur, size = [], 0
            pos = f.pos + size + a
            cur.append((bytes([len(cur) + 1]) * a if a > 300 else rng.integers(0, 256, a, dtype=np.uint8).tobytes(),
                        1 + int(rng.integers(0, min(pos, 70000))) if pos else 1, b, "auto"))
            if pos == 0:
                cur[-1] = (b"\x01", 1, b, "auto")
                size += 1
            size += a + b
        f.block(cur, **enc)
        out.append(("every_length_code_" + name,) + f.finish())
    # 256 KiB in two blocks: every offset code up to 17, and the sequence with the most extra bits that fits a block -- literal
    # length code 35 and match length code 52 (16 bits each) are 131075 bytes together, three more than a block: 15 + 16 + 17
    f = Frame()
    seqs, tail = full_block_seqs(rng)
    f.block(seqs, tail)
    big = (rng.integers(0, 256, 32768 + 32767 - 70, dtype=np.uint8).tobytes(), 131071 - 3 + 0, 65539 + 3, 0)
    f.block([big], b"")
    assert ll_code(len(big[0])) == 34 and ml_code(big[2]) == 52 and (big[1] + 3).bit_length() - 1 == 16
    out.append(("max_extra_bits_of16",) + f.finish())
    f = Frame()
    f.block(seqs, tail)
    f.block([(rng.integers(0, 256, 60000, dtype=np.uint8).tobytes(), 131072 + 59990, 65539 + 5400, 0)], b"", of="rle", ml="rle", ll="rle")
    out.append(("max_extra_bits_of17_rle52",) + f.finish())
    f = Frame()
    f.block(seqs, tail)
    pos, cur = BLOCK_MAX, []
    for c in list(range(2, 18)) * 3:
        lo, hi = (1 << c) - 3, min((2 << c) - 4, pos + 2)
        ll = int(rng.integers(0, 4))
        off = int(rng.choice([max(lo, 1), hi, int(rng.integers(max(lo, 1), hi + 1))]))
        cur.append((rng.integers(0, 256, ll, dtype=np.uint8).tobytes(), off, int(rng.integers(3, 40)), 0))
        pos += ll + cur[-1][2]
    f.block(cur, b"", of=("fse", 8))
    out.append(("offset_codes_2_to_17",) + f.finish())
    # offset 1, offset below the length, offset equal to the output position
    f = Frame()
    f.block([(b"q", 1, 300), (b"ab", 2, 7), (b"xyz", 306 + 6, 5), (b"", 3, 64), (b"k", 306 + 6 + 5 + 64 + 1, 306 + 6 + 5 + 64 + 1 + 9)])
    out.append(("offset_1_overlap_and_position",) + f.finish())
    return out


def fse_cases(rng):
    out = []
    lit = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def seqs_with(f, lcodes, mcodes, count, offs=(1, 40)):
        res, pos = [], f.pos
        for k in range(count):
            lc, mc = lcodes[k % len(lcodes)], mcodes[(k * 3 + k // 5) % len(mcodes)]
            ll = LL_BASE[lc] + int(rng.integers(0, 1 << LL_BITS[lc]))
            ml = ML_BASE[mc] + int(rng.integers(0, 1 << min(ML_BITS[mc], 6)))
            if pos + ll == 0:
                ll = 1
            pos += ll
            res.append((lit(ll), int(rng.integers(offs[0], min(pos, offs[1]) + 1)), ml))
            pos += ml
        return res

    for name, ll, of, ml in (("log5", ("fse", 5), ("fse", 5), ("fse", 5)), ("log_max", ("fse", 9), ("fse", 8), ("fse", 9)),
                             ("mixed_a", "predef", ("fse", 6), "rle"), ("mixed_b", ("fse", 6), "rle", "predef"), ("mixed_c", "rle", "predef", ("fse", 7))):
        f = Frame()
        f.raw(lit(50))
        one_ll, one_ml, one_of = ll == "rle", ml == "rle", of == "rle"
        s = seqs_with(f, [3] if one_ll else [0, 1, 2, 3, 5, 8, 16, 20], [4] if one_ml else [0, 1, 2, 5, 9, 30, 33, 40], 90,
                      offs=(13, 28) if one_of else (1, 40))
        f.block(s, lit(3), ll=ll, of=of, ml=ml)
        out.append(("fse_" + name,) + f.finish())
    # -1 entries and zero runs of 1, 2, 3, 4 and 7 between the used symbols; the first symbol unused
    f = Frame()
    f.raw(lit(80))
    s = seqs_with(f, [1, 3, 6, 10, 15, 23], [2, 4, 7, 11, 16, 24], 120)
    f.block(s, b"", ll=("fse", 6, (6, 23)), of=("fse", 5, (), ()), ml=("fse", 7, (2, 16, 24)))
    out.append(("fse_zero_runs_minus_one",) + f.finish())
    # only two symbols used; the last symbol of an alphabet (offsets: described, 2^31 is out of reach)
    f = Frame()
    f.raw(lit(80))
    f.block(seqs_with(f, [2, 7], [0, 12], 40, offs=(3, 12)), b"z", ll=("fse", 5), of=("fse", 5), ml=("fse", 5))
    out.append(("fse_two_symbols",) + f.finish())
    f = Frame()
    f.block([(lit(65536 + 100), 77, 9), (lit(3), 5, 30)], b"", ll=("fse", 6), of=("fse", 5, (), (31,)), ml=("fse", 5))
    f.block([(lit(9), 7, 65539 + 200), (lit(1), 2, 11)], b"", ll=("fse", 5), of=("fse", 6, (), (30, 31)), ml=("fse", 6))
    out.append(("fse_last_symbols",) + f.finish())
    # RLE mode with the largest symbol (offsets: code 17 in length_cases)
    f = Frame()
    f.block([(lit(65536 + 4000), 300, 3)], b"tail", ll="rle", of="rle", ml="rle")
    f.block([(lit(2), 1, 65539 + 4000)], b"", ll="rle", of="rle", ml="rle")
    out.append(("fse_rle_largest",) + f.finish())
    # Repeat after FSE, after RLE, after Predefined
    for prev in ("fse", "rle", "predef"):
        f = Frame()
        f.raw(lit(60))
        mode = lambda log: ("fse", log) if prev == "fse" else prev
        one = prev == "rle"
        lc, mc = ([4], [6]) if one else ([0, 2, 4, 9, 17], [0, 3, 6, 20, 35])
        offs = (13, 28) if one else (1, 40)
        f.block(seqs_with(f, lc, mc, 70, offs), lit(2), ll=mode(7), of=mode(6), ml=mode(7))
        f.block(seqs_with(f, lc, mc, 1 if one else 66, offs), lit(1), ll="repeat", of="repeat" if one or prev == "predef" else ("fse", 5), ml="repeat")
        f.rle(9, 20)
        f.block(seqs_with(f, lc, mc, 5, offs), b"", ll="repeat", of="repeat", ml="repeat")
        out.append(("fse_repeat_after_" + prev,) + f.finish())
    return out


def huffman_cases(rng):
    out = []
    w256 = [2] * 256
    w256[17], w256[3], w256[255] = 3, 1, 1
    w255 = [1] * 255
    w255[100] = 2
    w11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    trees = (("2sym", [0] * 64 + [1, 1], "direct"), ("3sym", [1, 1, 2], "direct"), ("3sym_spread", [1] + [0] * 200 + [2] + [0] * 53 + [1], "fse"),
             ("128sym", [1] * 128, "direct"), ("255sym", w255, "fse"), ("256sym", w256, "fse"), ("len11", w11, "direct"),
             ("len11_fse", [0, 0] + w11, ("fse", 5)), ("4sym", [2, 1, 1, 3], "direct"), ("13sym_fse_odd", w11[:-1] + [0, 0, 1], "fse"))
    for name, w, tree in trees:
        f = Frame()
        n = 300 if len(w) < 100 else 3000
        lits = _syms_for(rng, w, n)
        f.block([(lits[:40], 9, 5), (lits[40:n - 20], 30, 8)], lits[n - 20:], lits="huf", weights=w, tree=tree, streams=1 if n < 1000 else 4)
        f.block([(lits[5:60], 100, 4)], lits[:9], lits="treeless", streams=1)
        out.append(("huf_" + name,) + f.finish())
    # regenerated sizes around the size formats
    w = huf_weights_for(_text(rng, 4000, 60, syms=np.arange(33, 93, dtype=np.uint8)))
    for n, fmts in ((6, (0, 1)), (7, (0, 1)), (1023, (0, 1, 2)), (1024, (2, 3)), (16383, (2, 3)), (16384, (3,)), (20001, (3,))):
        for fmt in fmts:
            lits = _syms_for(rng, w, n)
            f = Frame()
            f.block([], lits, lits="huf", weights=w, tree="direct" if fmt & 1 else "fse", streams=1 if fmt == 0 else 4, lit_format=fmt)
            cut = n // 3
            f.block([(lits[:cut], 4, 3)], lits[cut:], lits="treeless", streams=1 if fmt == 0 else 4, lit_format=fmt)
            out.append(("huf_regen%d_fmt%d" % (n, fmt),) + f.finish())
    # raw and RLE literals with every header size
    # (no literals behind a 1-byte header and no sequences is a 2-byte block: libzstd wants three, so that one is left out)
    for n, sizes in ((0, (2, 3)), (31, (1, 2, 3)), (32, (2, 3)), (4095, (2, 3)), (4096, (3,)), (70000, (3,))):
        for hs in sizes:
            f = Frame()
            lits = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            f.block([(lits[:n // 2], 1, 3)] if n else [], lits[n // 2:], lit_format=hs)
            if n:
                f.block([(b"\x33" * (n // 2), 2, 3)], b"\x33" * (n - n // 2), lits="rle", lit_format=hs)
            out.append(("lits_raw_rle%d_hdr%d" % (n, hs),) + f.finish())
    # 24000 literals over 128 symbols: more than 20 KiB coded (the walk's stage holds 8), with a tree and treeless behind it
    w = [1] * 128
    f = Frame()
    for how in ("huf", "treeless"):
        lits = _syms_for(rng, w, 24000)
        seqs, at = [], 0
        for k in range(50):
            at += 400
            seqs.append((lits[at - 400:at], 1 + int(rng.integers(0, min(3000, f.pos + at))), 3 + k % 30))
        f.block(seqs, lits[at:], lits=how, weights=w, streams=4)
        assert len(f.blocks[-1][1]) > 20480
    out.append(("huf_20k_tree_then_treeless",) + f.finish())
    # a sequence bit stream above 8 KiB: 4200 sequences with offset codes 12 - 15
    f = Frame()
    f.raw(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())
    seqs, pos = [], 40000
    for k in range(4200):
        ll = int(rng.integers(0, 3))
        pos += ll
        seqs.append((rng.integers(0, 256, ll, dtype=np.uint8).tobytes(), int(rng.integers(4100, 39000)), int(rng.integers(3, 12))))
        pos += seqs[-1][2]
    f.block(seqs, b"", ll=("fse", 6), of=("fse", 7), ml=("fse", 8))
    assert len(f.blocks[-1][1]) > 8192 + 4200
    out.append(("seq_stream_above_8k",) + f.finish())
    return out


def header_cases(rng):
    out = []
    for n in (0, 100, 255, 256, 300, 65535 + 256, 70000):
        for fb in (1, 2, 4, 8):
            if (fb == 1 and n > 255) or (fb == 2 and not 256 <= n < 65536 + 256):
                continue
            fr, want = random_frame(rng, n, 0, fcs_bytes=fb) if n >= 40 else (Frame().raw(bytes(range(n % 256))[:n]).finish(fcs_bytes=fb) if n else Frame().finish(fcs_bytes=fb))
            out.append(("fcs%d_n%d" % (fb, n), fr, want))
    for fb in (0, 2, 4, 8):
        for ck in (False, True):
            fr, want = random_frame(rng, 3000, 1, single=False, fcs_bytes=fb, checksum=ck)
            out.append(("window_fcs%d_ck%d" % (fb, ck), fr, want))
    fr, want = random_frame(rng, 140000, 2, checksum=True)
    out.append(("checksum_two_blocks", fr, want))
    fr, want = random_frame(rng, 31, 0, checksum=True)
    out.append(("checksum_31", fr, want))
    return out


_CACHE = {}


def frame_cases():
    """[(name, frame bytes, expected output)]: every named case, then random frames in the three styles"""
    if "frames" not in _CACHE:
        rng = np.random.default_rng(20261019)
        cases = []
        for group in (block_structure_cases, count_cases, repeat_cases, length_cases, fse_cases, huffman_cases, header_cases):
            cases += group(rng)
        for k in range(12):
            n = int(rng.choice([13, 40, 257, 4096, 30000, 65536, 100000, 131072 + 15, 200000]))
            cases.append(("random%d_s%d_%d" % (k, k % 3, n),) + random_frame(rng, n, k % 3))
        assert len({c[0] for c in cases}) == len(cases)
        _CACHE["frames"] = cases
    return _CACHE["frames"]


def digests(cases):
    return {name: [hashlib.sha256(fr).hexdigest(), hashlib.sha256(want.tobytes()).hexdigest()] for name, fr, want in cases}


# ---- frames every decoder must refuse -------------------------------------------------------------------------------------------
def bad_frames():
    """[(name, frame, n, status or None)]: n is the size the frame claims (the capacity a chunk gives it); status: the one code the
    format asks for (None: any negative one).  Each is a valid frame of about 1300 bytes with ONE thing wrong."""
    rng = np.random.default_rng(77)
    lit = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = []

    def base(**kw):
        f = Frame()
        f.block([(lit(30), 7, 500), (lit(6), 100, 40), (lit(3), 20, 700)], lit(5), **kw)
        return f

    def patched(f, at, fn, **fin):
        fr, want = f.finish(**fin)
        fr = bytearray(fr)
        at = f.block_at[-1] + at
        fr[at] = fn(fr[at])
        return bytes(fr), want

    f = base()
    fr, want = patched(f, f.modes_at, lambda b: 0xFC)
    out.append(("repeat_mode_without_predecessor", fr, want.size, None))
    f = Frame().block([(_text(rng, 400), 7, 500), (lit(0), 100, 40)], _text(rng, 300), lits="huf", streams=1)
    fr, want = patched(f, 0, lambda b: b | 3)
    out.append(("treeless_without_predecessor", fr, want.size, None))
    f = base(ll=("fse", 9))
    fr, want = patched(f, f.modes_at + 1, lambda b: (b & 0xF0) | 5)
    out.append(("accuracy_log_10", fr, want.size, None))
    w12 = [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    l12 = _syms_for(rng, w12, 600)
    fr, want = Frame().block([(l12[:300], 7, 500)], l12[300:], lits="huf", weights=w12, streams=1).finish()
    out.append(("huffman_12_bits", fr, want.size, None))
    f = Frame().raw(lit(16)).block([(b"", 0, 900, 3), (lit(4), 9, 300)], b"")
    fr, want = f.finish(invalid=True)
    out.append(("rep1_minus_1_is_0", fr, want.size, None))
    f = Frame().block([(lit(30), 7, 500), (lit(6), 537, 40), (lit(3), 20, 700)], lit(5))
    fr, want = f.finish(invalid=True)
    out.append(("offset_beyond_output", fr, want.size, None))
    fr, want = base().finish(fhd_or=0x08)
    out.append(("reserved_fhd_bit", fr, want.size, None))
    fr, want = base().finish(fhd_or=0x01)
    out.append(("dictionary_id", fr[:5] + b"\x07" + fr[5:], want.size, -7))
    fr, want = base(junk_bits=8).finish()
    out.append(("sequence_stream_leftover_bits", fr, want.size, None))
    fr, want = base().finish(fcs=1283)
    assert want.size == 1284
    out.append(("fcs_differs", fr, want.size, None))
    fr, want = base().finish(last=False)
    out.append(("last_block_missing", fr, want.size, None))
    assert all(len(fr) < n for _, fr, n, _ in out)
    return out


# ---- streams of chunks (tests/_streams.py: coded_stream) ---------------------------------------------------------------------------
FLAVORS = ("raw", "huf", "repeat", "tokens", "blocks", "counts", "tail")


def coded_frame(rng, n, flavor):
    """(frame, reference) of a stream of n bytes drawn from the case families above, or None where it would not be smaller than n"""
    lit = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    if n < 16:
        return None
    if flavor == "tail" and n > BLOCK_MAX + 13:
        # a full block, then the rest as sequences with no literals behind them: the tail's literals lie at the very end of the output
        seqs, tail = full_block_seqs(rng, text=True)
        f = Frame().block(seqs, tail, lits="huf", tree="fse", ll=("fse", 8), of=("fse", 7), ml=("fse", 8))
        left = n - BLOCK_MAX
        cur = []
        while left > 40000:
            cur.append((lit(3), int(rng.integers(1, 5000)), 30000))
            left -= 30003
        a = (left - 7) // 2
        cur += [(lit(4), 4, 3), (lit(a), int(rng.integers(1, 2000)), left - 7 - a)]
        f.block(cur, b"")
        got = f.finish()
    elif flavor == "tokens" and n >= 256:
        b = ZB(rng, text=True)
        b.lit(64)
        count = int(rng.integers(70, 300))
        while b.pos < n - 80 and count > 0:
            b.match(int(rng.integers(1, min(64, b.pos) + 1)), int(rng.integers(3, 9)))
            if rng.integers(0, 8) == 0:
                b.lit(int(rng.integers(1, 4)))
            count -= 1
        b.random(n - 1)
        got = frame_of(b.finish(n)[0], 1 + int(rng.integers(0, 2)))
    elif flavor == "counts" and n >= 1200:
        f = Frame()
        f.block(_small_seqs(rng, f, int(rng.choice([63, 64, 65, 127, 128, 129]))), b"", ll=("fse", 6), of=("fse", 6), ml=("fse", 5))
        if f.pos > n - 8:
            return None
        f.block([(lit(2), 1 + int(rng.integers(0, 50)), n - f.pos - 2 - 3)], lit(3))
        got = f.finish(checksum=bool(rng.integers(0, 2)))
    elif flavor == "blocks" and 2000 <= n <= 4 * BLOCK_MAX:
        f, h = Frame(), Hist()
        t = _text(rng, 500)
        f.block([(t[:200], h.new(3), 60), (t[200:420], h.new(11), 90), (b"", h.new(200), 40)], t[420:], lits="huf", tree="fse",
                ll=("fse", 5), of=("fse", 5), ml=("fse", 5))
        f.raw(lit(37)).rle(int(rng.integers(0, 256)), 150)
        f.block([(t[:200], h.rep(2, 200), 60, 2), (t[200:420], h.rep(3, 220), 90, 3), (b"", h.rep(3, 0), 40, 3)], t[420:], lits="treeless",
                ll="repeat", of=("fse", 5, (), (5, 9)), ml="repeat")
        if f.pos > n - 8:
            return None
        left = n - f.pos
        while left > BLOCK_MAX:
            f.block([(lit(1), 1, BLOCK_MAX - 1)])
            left -= BLOCK_MAX
        f.block([(lit(2), 1 + int(rng.integers(0, 900)), left - 5)], lit(3)) if left >= 8 else f.raw(lit(left))
        got = f.finish(single=bool(rng.integers(0, 2)), fcs_bytes=None)
    else:
        got = random_frame(rng, n, {"raw": 0, "huf": 1, "repeat": 2}.get(flavor, int(rng.integers(0, 3))))
    frame, ref = got
    assert ref.size == n, (flavor, n, ref.size)
    return (frame, ref) if len(frame) < n else None


def mix_streams(count=120, seed=5):
    """{name: bytes}: streams of random and constant pieces whose lengths cover every literal-length and match-length code (the
    make-up of the `mix*` inputs of test_emu_zstd.py's encoder test, from a generator of their own).  The frames the repository's
    encoder makes of them keep their literals raw and their runs long: what the decoder's literal copies are tested on."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in range(count):
        n = int(rng.integers(64, 40000))
        pieces, left = [], n
        while left > 0:
            m = int(min(left, rng.choice([1, 3, 15, 16, 40, 70, 130, 300, 2000])))
            pieces.append(rng.integers(0, 256, m, dtype=np.uint8) if rng.random() < 0.5 else np.full(m, rng.integers(0, 256), np.uint8))
            left -= m
        out["mix%d" % k] = np.concatenate(pieces)
    return out


def chunkable(frames, limit=262144):
    """the (name, frame, output) cases a blosc2 chunk can carry as the one coded stream of a block: the stream must be SHORTER than the
    block (a stream of the block's length is a stored one, a longer one is refused) and a block holds 1 .. 256 KiB"""
    return [(name, fr, want) for name, fr, want in frames if 0 < len(fr) < want.size <= limit]


def chunk_of_frame(fr, want):
    """one chunk, one block, one stream: typesize 1, no filter"""
    return S.chunk_of_streams(S.ZSTD, [(bytes(fr), want)])


# The LDS of cimg_decode_zstd follows the largest block of its batch and holds stage and tables beside it: the forms of the read path
# that need that kernel (fused, plans_overflow, no memory for plans) refuse a batch with a 150 000-byte block (ERR_CODEC_SUPPORT).  A
# batch that every form must take stops at the largest block the planes of _streams.zstd_plane_cases prove every form takes
# (zstd_tail33); blocks beyond LDS_BLOCK_MAX take the wide route.
FORM_BLOCK_MAX = 131072 + 33
LDS_BLOCK_MAX = 163840


def frame_chunk_cases(golden_dir, encode):
    """[(name, chunk, expected bytes)] for the batched frame tests of both legs: every spec-built frame a chunk can carry (expected:
    what its sequences define), the frames libzstd made of inputs up to 160 KiB (tests/golden/zstd_kat.npz; expected: the golden
    input) and the frames `encode` -- the emulated encoder in ascending order -- makes of the mix streams (expected: the stream).
    The last two groups hold every frame the decoder's literal copies got wrong in the other write orders."""
    import os
    if "frame_chunks" not in _CACHE:
        cases = list(frame_cases())
        kat = np.load(os.path.join(golden_dir, "zstd_kat.npz"))
        for key in kat["frames"]:
            key = str(key)
            src = kat["in|" + key.split("|")[0]]
            if src.size <= 163840:
                cases.append(("kat|" + key, kat["frame|" + key].tobytes(), src))
        for name, src in mix_streams().items():
            fr = encode(src)
            if fr:
                cases.append((name, fr, src))
        _CACHE["frame_chunks"] = [(name, chunk_of_frame(fr, want), want) for name, fr, want in chunkable(cases)]
    return _CACHE["frame_chunks"]

