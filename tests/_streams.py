"""Spec-built LZ4 and BloscLZ streams and blosc2 chunks, with the buffers they are defined to produce.

Test infrastructure for test_emu_stream_conformance.py (CPU) and test_gpu_stream_conformance.py (-m gpu).  It shares no code with
oracle/ or csrc/: a stream is a list of sequences (literal bytes, then a match given as (offset, length), overlap allowed), the
reference output is what running those sequences produces, and the writers below put the same sequences down in the LZ4 block
format and in the BloscLZ stream format (the one described at the top of oracle/blosclz.c):

  LZ4      token (literal count : match length - 4, 4 bits each, 15 = more bytes follow, 255 = and more), literals, 16-bit LE
           offset, match length bytes.  The last sequence is literals only (at least 5 of them), and the last match starts at
           least 12 bytes before the end of the block.
  BloscLZ  ctrl < 32: ctrl + 1 literals follow (at most 32; the first ctrl of a stream has bit 5 set as a marker).  ctrl >= 32: a
           match of (ctrl >> 5) + 2 bytes; (ctrl >> 5) == 7 adds length bytes (each 255 continues); then the distance: near
           (distance - 1 = (ctrl & 31) << 8 | byte, up to 8191) or far ((ctrl & 31) == 31 and byte == 255, then two big-endian
           bytes: distance = 8192 + that, up to 73727).  A stream does not end in a match.

Everything is generated from seeds: the CPU and the GPU leg build the same streams and chunks.

Codec "zstd" (codec format 4, compcode 5): a stream of a chunk is one complete zstd frame, written by tests/_zstd_streams.py
(coded_stream hands over to it; zstd_plane_cases are its planes, for test_emu_zstd_streams.py and test_gpu_zstd_streams.py).
"""
import numpy as np

LZ4, BLOSCLZ, ZSTD = "lz4", "blosclz", "zstd"
COMPCODE = {BLOSCLZ: 0, LZ4: 1, ZSTD: 5}
COMPFORMAT = {BLOSCLZ: 0, LZ4: 1, ZSTD: 4}
LZ4_MAX_OFFSET = 65535
BLZ_MAX_NEAR = 8191
BLZ_MAX_FAR = 65535 + 8192
NOFILTER, SHUFFLE, BITSHUFFLE = 0, 1, 2
HEADER_LEN = 32
CANARY = 0xA5


# ---- sequences and the reference ------------------------------------------------------------------------------------------------
def run_sequences(seqs):
    """The buffer a list of (literals, offset, length) sequences produces (length 0: no match)."""
    out = bytearray()
    for lit, off, ml in seqs:
        out += lit
        if ml:
            if not 1 <= off <= len(out):
                raise ValueError("match offset %d at output position %d" % (off, len(out)))
            start = len(out) - off
            if off >= ml:
                out += out[start:start + ml]
            else:                                    # overlapping: byte t of the match is byte t mod offset of the pattern
                pat = bytes(out[start:])
                out += (pat * (ml // off + 1))[:ml]
    return np.frombuffer(bytes(out), np.uint8)


def check_lz4(seqs, n):
    """The rules of a valid LZ4 block (raises on a broken one)."""
    pos = 0
    for k, (lit, off, ml) in enumerate(seqs):
        pos += len(lit)
        if k == len(seqs) - 1:
            assert ml == 0 and len(lit) >= 5, "the last sequence is >= 5 literals"
        else:
            assert ml >= 4 and 1 <= off <= min(pos, LZ4_MAX_OFFSET), (k, off, ml, pos)
            assert pos <= n - 12, "a match starts at least 12 bytes before the end"
            pos += ml
    assert pos == n


def check_blosclz(seqs, n):
    pos = 0
    for k, (lit, off, ml) in enumerate(seqs):
        if k == 0:
            assert len(lit) >= 1, "a BloscLZ stream starts with literals"
        pos += len(lit)
        if k == len(seqs) - 1:
            assert ml == 0 and len(lit) >= 1, "a BloscLZ stream ends in literals"
        else:
            assert ml >= 3 and 1 <= off <= min(pos, BLZ_MAX_FAR), (k, off, ml, pos)
            pos += ml
    assert pos == n


# ---- writers --------------------------------------------------------------------------------------------------------------------
def _lz4_len(out, v):
    out += b"\xff" * (v // 255)
    out.append(v % 255)


def lz4_block(seqs):
    out = bytearray()
    for lit, off, ml in seqs:
        L = len(lit)
        m = ml - 4
        out.append((min(L, 15) << 4) | (min(m, 15) if ml else 0))
        if L >= 15:
            _lz4_len(out, L - 15)
        out += lit
        if ml:
            out += off.to_bytes(2, "little")
            if m >= 15:
                _lz4_len(out, m - 15)
    return bytes(out)


def blosclz_stream(seqs):
    out = bytearray()
    for k, (lit, off, ml) in enumerate(seqs):
        for a in range(0, len(lit), 32):
            run = lit[a:a + 32]
            out.append(len(run) - 1)
            out += run
        if ml:
            d = off - 1
            far = off > BLZ_MAX_NEAR
            if far:
                d -= BLZ_MAX_NEAR
            hi = 31 if far else d >> 8
            if ml <= 8:
                out.append(((ml - 2) << 5) | hi)
            else:
                out.append((7 << 5) | hi)
                _lz4_len(out, ml - 9)
            if far:
                out += bytes([255, d >> 8, d & 255])
            else:
                out.append(d & 255)
    out[0] |= 32
    return bytes(out)


# ---- sequence sources -----------------------------------------------------------------------------------------------------------
_LITS = np.array([0, 0, 0, 1, 2, 3, 4, 5, 7, 8, 14, 15, 16, 19, 33, 64])


class Builder:
    """Sequences appended one by one, with the output so far (so that offsets can be chosen against it)."""

    def __init__(self, rng, codec):
        self.rng, self.codec = rng, codec
        self.seqs, self.pending, self.out = [], bytearray(), bytearray()
        self.min_ml = 3 if codec == BLOSCLZ else 4
        self.max_off = BLZ_MAX_FAR if codec == BLOSCLZ else LZ4_MAX_OFFSET

    @property
    def pos(self):
        return len(self.out)

    def lit(self, n=None, data=None):
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes() if data is None else bytes(data)
        self.pending += data
        self.out += data
        return self

    def match(self, off, ml):
        self.seqs.append((bytes(self.pending), off, ml))
        self.pending = bytearray()
        start = len(self.out) - off
        assert 1 <= off <= len(self.out) and off <= self.max_off and ml >= self.min_ml, (off, ml, len(self.out))
        if off >= ml:
            self.out += self.out[start:start + ml]
        else:
            pat = bytes(self.out[start:])
            self.out += (pat * (ml // off + 1))[:ml]
        return self

    def random(self, upto, lit_scale=1.0):
        """random sequences until the output is about `upto` bytes long (never longer)"""
        rng = self.rng
        while True:
            L = int(_LITS[rng.integers(len(_LITS))] * lit_scale)
            if self.pos == 0 and L == 0:
                L = 1
            kind = rng.integers(0, 10)
            ml = (int(rng.integers(self.min_ml, 19)) if kind < 6 else int(rng.integers(19, 80)) if kind < 9
                  else int(rng.integers(80, 700)))
            if self.pos + L + ml > upto:
                L = min(L, 2)
                ml = upto - self.pos - L
                if ml < self.min_ml or self.pos + L == 0:
                    return self
            self.lit(L)
            r = rng.integers(0, 10)
            hi = min(self.pos, self.max_off)
            off = (int(rng.integers(1, min(9, hi + 1))) if r < 3 else int(rng.integers(1, min(65, hi + 1))) if r < 6
                   else int(rng.integers(1, min(1100, hi + 1))) if r < 8 else int(rng.integers(1, hi + 1)))
            self.match(off, ml)

    def ensure(self, n):
        """at least n bytes of output"""
        if self.pos < n:
            self.random(n)
        if self.pos < n:
            self.lit(n - self.pos)
        return self

    def finish(self, n):
        """end the stream with literals so that the output is n bytes; returns (seqs, reference output)"""
        assert self.pos <= n
        self.lit(n - self.pos)
        self.seqs.append((bytes(self.pending), 0, 0))
        self.pending = bytearray()
        ref = run_sequences(self.seqs)
        assert ref.tobytes() == bytes(self.out)
        return self.seqs, ref


def end_room(codec):
    """room a generator leaves at the end: LZ4's last match starts >= 12 bytes before the end, its last 5 bytes are literals"""
    return 12 if codec == LZ4 else 1


def random_stream(rng, n, codec, lit_scale=1.0):
    b = Builder(rng, codec)
    b.lit(int(rng.integers(1, 9)))
    b.random(n - end_room(codec), lit_scale)
    return b.finish(n)


def head_tail(rng, n, codec, slack=1):
    """One literal, one maximal offset-1 match, then an incompressible literal tail: the stream is `slack` bytes (or a few more)
    below n.  The in-place decoder's write pointer then runs right behind its read pointer for the whole tail."""
    tail_of = lambda M: n - 1 - M
    for M in range(4, n):
        T = tail_of(M)
        if codec == LZ4:
            size = 1 + 1 + 2 + ((M - 19) // 255 + 1 if M - 4 >= 15 else 0) + 1 + ((T - 15) // 255 + 1 if T >= 15 else 0) + T
        else:
            size = 2 + 1 + ((M - 9) // 255 + 1 if M > 8 else 0) + 1 + T + (T + 31) // 32
        if size <= n - slack and T >= 5:
            b = Builder(rng, codec)
            b.lit(1).match(1, M)
            return b.finish(n)
    return random_stream(rng, n, codec)


def zero_literal_run(rng, n, codec, count=200):
    """more than 64 tokens in a row, most of them matches with no literals of their own"""
    b = Builder(rng, codec)
    b.lit(64)
    while b.pos < n - 64 - end_room(codec) and count > 0:
        ml = int(rng.integers(b.min_ml, 9))
        b.match(int(rng.integers(1, min(64, b.pos) + 1)), ml)
        if rng.integers(0, 8) == 0:
            b.lit(int(rng.integers(1, 4)))
        count -= 1
    b.random(n - end_room(codec))
    return b.finish(n)


def lz4_edges(rng):
    """(name, seqs, reference) of the targeted LZ4 edge classes"""
    out = []

    def add(name, b, n=None):
        seqs, ref = b.finish(b.pos + 12 if n is None else n)
        check_lz4(seqs, ref.size)
        out.append((name, seqs, ref))

    offs = [1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 1023, 1024, 1025, 65535]
    for off in offs:
        b = Builder(rng, LZ4)
        b.lit(16).ensure(off + 40)
        for ml in (4, 5, off, off + 1, 17, 63, 64, 65, 200, 1100):
            b.lit(int(rng.integers(0, 3))).match(off, max(ml, 4))
        b.lit(3).match(min(off, b.pos), 4096 + off % 7)
        add("lz4_off%d" % off, b)
    for ml in (4, 18, 19, 270, 271, 65536, 70001):
        for off in (1, 3, 7, 100, 5000):
            b = Builder(rng, LZ4)
            b.lit(16).ensure(5100)
            b.lit(1).match(off, ml).lit(2).match(off, ml)
            add("lz4_ml%d_off%d" % (ml, off), b)
    for L in (0, 1, 14, 15, 16, 269, 270, 271, 4097, 5000):
        b = Builder(rng, LZ4)
        b.lit(8).match(8, 30000)
        for _ in range(3):
            b.lit(L).match(int(rng.integers(1, 3000)), 3000)
        b.lit(L).match(11, 4)
        add("lz4_lit%d" % L, b)
    # end-of-block limits hit exactly: the last match starts 12 bytes before the end; the last 5 bytes are literals
    for n in (13, 16, 100, 4096, 65536):
        b = Builder(rng, LZ4)
        b.lit(1)
        if n - 12 - 1 >= 4:
            b.random(n - 12 - 4)
        b.lit(n - 12 - b.pos).match(1, 7)
        seqs, ref = b.finish(n)
        assert seqs[-2][2] == 7 and len(seqs[-1][0]) == 5
        check_lz4(seqs, n)
        out.append(("lz4_end%d" % n, seqs, ref))
    b = Builder(rng, LZ4)
    b.lit(200).random(1000 - 16)
    b.lit(1000 - 12 - b.pos).match(13, 4)                 # match starts exactly at n - 12, 8 literals behind it
    seqs, ref = b.finish(1000)
    check_lz4(seqs, 1000)
    out.append(("lz4_end_start12", seqs, ref))
    for n in (4096, 65536, 131072):
        seqs, ref = zero_literal_run(rng, n, LZ4, count=300)
        check_lz4(seqs, n)
        out.append(("lz4_tokens%d" % n, seqs, ref))
    for n in (2048, 32768, 65536, 131072, 262144):
        for slack in (1, 3, 16):
            seqs, ref = head_tail(rng, n, LZ4, slack)
            check_lz4(seqs, n)
            out.append(("lz4_headtail%d_%d" % (n, slack), seqs, ref))
    return out


def blosclz_edges(rng):
    out = []

    def add(name, b, n=None):
        seqs, ref = b.finish(b.pos + 1 if n is None else n)
        check_blosclz(seqs, ref.size)
        out.append((name, seqs, ref))

    for off in (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 255, 256, 8191, 8192, 8193, 65535, 73724, 73725, 73726, 73727):
        b = Builder(rng, BLOSCLZ)
        b.lit(16).ensure(off + 40)
        for ml in (3, 4, 8, 9, 10, off, off + 1, 64, 65, 264, 519, 1100):
            b.lit(int(rng.integers(0, 3))).match(off, max(ml, 3))
        add("blz_off%d" % off, b)
    for ml in (3, 4, 5, 8, 9, 10, 263, 264, 265, 774, 2559, 25509, 76509):
        for off in (1, 2, 5, 40, 8191, 8192):
            b = Builder(rng, BLOSCLZ)
            b.lit(16).ensure(8300)
            b.lit(1).match(off, ml).match(off, ml).lit(2).match(off, ml)
            add("blz_ml%d_off%d" % (ml, off), b)
    for L in (1, 31, 32, 33, 64, 65, 300, 4097):
        b = Builder(rng, BLOSCLZ)
        b.lit(L).match(1, 500)
        for _ in range(3):
            b.lit(L).match(int(rng.integers(1, 400)), 400)
        add("blz_lit%d" % L, b, b.pos + L)
    for n in (4096, 65536, 131072):
        seqs, ref = zero_literal_run(rng, n, BLOSCLZ, count=300)
        check_blosclz(seqs, n)
        out.append(("blz_tokens%d" % n, seqs, ref))
    for n in (2048, 32768, 65536, 131072, 262144):
        for slack in (1, 3, 16):
            seqs, ref = head_tail(rng, n, BLOSCLZ, slack)
            check_blosclz(seqs, n)
            out.append(("blz_headtail%d_%d" % (n, slack), seqs, ref))
    return out


def stream_cases(seed=2024, nrandom=40):
    """[(name, codec, stream bytes, reference)]: the edge classes of both formats, then random streams of both"""
    rng = np.random.default_rng(seed)
    cases = [(nm, LZ4, lz4_block(s), r) for nm, s, r in lz4_edges(rng)]
    cases += [(nm, BLOSCLZ, blosclz_stream(s), r) for nm, s, r in blosclz_edges(rng)]
    for k in range(nrandom):
        n = int(rng.choice([13, 40, 257, 4096, 30000, 65536, 100000]))
        for codec in (LZ4, BLOSCLZ):
            seqs, ref = random_stream(rng, n, codec, lit_scale=float(rng.choice([0.5, 1, 3])))
            (check_lz4 if codec == LZ4 else check_blosclz)(seqs, n)
            cases.append(("%s_random%d_%d" % (codec, k, n), codec, (lz4_block if codec == LZ4 else blosclz_stream)(seqs), ref))
    # the same sequences in both formats (valid for both: offsets <= 65535, matches >= 4, literals first)
    for k in range(8):
        n = int(rng.choice([300, 5000, 65536]))
        seqs, ref = random_stream(rng, n, LZ4)
        check_blosclz(seqs, n)
        cases.append(("both_random%d_lz4" % k, LZ4, lz4_block(seqs), ref))
        cases.append(("both_random%d_blz" % k, BLOSCLZ, blosclz_stream(seqs), ref))
    return cases


# ---- filters (numpy restatements) -----------------------------------------------------------------------------------------------
def unshuffle(ts, src):
    src = np.asarray(src, np.uint8)
    ne = src.size // ts
    out = src.copy()
    if ts > 1 and ne:
        out[:ne * ts] = src[:ne * ts].reshape(ts, ne).T.ravel()
    return out


def bitunshuffle(ts, src):
    """bit row 8j + k holds bit k of byte j of every element (element i: byte i / 8, bit i % 8); whole groups of 8 elements only"""
    src = np.asarray(src, np.uint8)
    ne = src.size // ts
    ne8 = ne - ne % 8
    out = src.copy()
    if ne8:
        rows = src[:ne8 * ts].reshape(8 * ts, ne8 // 8)
        bits = np.unpackbits(rows, axis=1, bitorder="little").reshape(ts, 8, ne8)
        out[:ne8 * ts] = np.packbits(bits, axis=1, bitorder="little").reshape(ts, ne8).T.ravel()
    return out


def unfilter(filt, ts, block):
    return unshuffle(ts, block) if filt == SHUFFLE else bitunshuffle(ts, block) if filt == BITSHUFFLE else np.asarray(block, np.uint8)


# ---- chunks ---------------------------------------------------------------------------------------------------------------------
def header(codec, ts, nbytes, blocksize, cbytes, filt, split):
    """the 32-byte blosc2 header (oracle/chunk.c write_header, csrc/plan.h): extended-header flags, split bit, codec format"""
    h = bytearray(HEADER_LEN)
    h[0], h[1] = 5, 1
    h[2] = 0x01 | 0x04 | (0 if split else 0x10) | (COMPFORMAT[codec] << 5)
    h[3] = ts
    h[4:8] = int(nbytes).to_bytes(4, "little")
    h[8:12] = int(blocksize).to_bytes(4, "little")
    h[12:16] = int(cbytes).to_bytes(4, "little")
    h[16 + 5] = filt
    h[22] = COMPCODE[codec]
    return h


def coded_stream(rng, n, codec, flavor):
    """(stream bytes, reference) of a coded plane of n bytes, or None when the flavor's stream would not be smaller than n"""
    if codec == ZSTD:                                # (one complete frame per stream: tests/_zstd_streams.py)
        import _zstd_streams as Z
        return Z.coded_frame(rng, n, flavor)
    if flavor == "headtail" and n >= 64:
        seqs, ref = head_tail(rng, n, codec, slack=int(rng.choice([1, 2, 9])))
    elif flavor == "tokens" and n >= 256:
        seqs, ref = zero_literal_run(rng, n, codec, count=int(rng.integers(70, 300)))
    elif flavor == "far" and codec == BLOSCLZ and n > BLZ_MAX_FAR + 200:
        b = Builder(rng, codec)
        b.lit(16).ensure(BLZ_MAX_FAR + 64)
        for off in (BLZ_MAX_FAR, BLZ_MAX_FAR - 3, 65535 + 8191 - 1, 8192, 8191):
            b.lit(int(rng.integers(0, 3))).match(min(off, b.pos), int(rng.choice([3, 9, 9 + 255 * int(rng.integers(1, 40))])))
        b.random(n - end_room(codec))
        seqs, ref = b.finish(n)
    elif flavor == "long" and n >= 4096:
        b = Builder(rng, codec)
        b.lit(32).random(1000)
        b.lit(3).match(int(rng.integers(1, 9)), n // 2 - b.pos)
        b.random(n - end_room(codec))
        seqs, ref = b.finish(n)
    else:
        if n < 16:
            return None
        seqs, ref = random_stream(rng, n, codec, lit_scale=float(rng.choice([0.5, 1, 2])))
    (check_lz4 if codec == LZ4 else check_blosclz)(seqs, n)
    s = lz4_block(seqs) if codec == LZ4 else blosclz_stream(seqs)
    return (s, ref) if len(s) < n else None


def make_chunk(rng, codec, ts, blocksize, nbytes, filt, split, layout="natural", policy="any", flavors=("random",)):
    """A blosc2 chunk of generated streams -> (chunk bytes, expected pixels, {kind: count}).

    Every stream picks a kind on its own: coded (a generated stream of one of `flavors`), stored, zero run or byte run
    (policy "lean": at most one coded plane a block, the blocks the lean decode kernel takes; "coded": mostly coded planes; "all":
    every plane coded).  layout: "natural" (blocks in
    order, back to back), "shuffled" (bstarts in a shuffled order) or "gaps" (shuffled, with garbage between the blocks)."""
    assert blocksize % ts == 0 and blocksize <= nbytes
    nblocks = -(-nbytes // blocksize)
    counts = {"coded": 0, "stored": 0, "zero": 0, "run": 0}
    blocks, pixels = [], []
    for j in range(nblocks):
        bsize = min(blocksize, nbytes - j * blocksize)
        ns = ts if split and bsize == blocksize else 1
        ne = bsize // ns
        coded_plane = int(rng.integers(0, ns + 1)) if policy == "lean" else -1
        body, filtered = bytearray(), []
        for s in range(ns):
            if policy == "lean":
                kind = "coded" if s == coded_plane else str(rng.choice(["stored", "zero", "run"]))
            elif policy == "all":
                kind = "coded"
            else:
                kind = str(rng.choice(["coded"] * (6 if policy == "coded" else 3) + ["stored", "zero", "run"]))
            got = coded_stream(rng, ne, codec, str(rng.choice(list(flavors)))) if kind == "coded" else None
            if kind == "coded" and got is None:
                kind = "stored"
            counts[kind] += 1
            if kind == "coded":
                s_bytes, ref = got
                body += len(s_bytes).to_bytes(4, "little", signed=True) + s_bytes
                filtered.append(ref)
            elif kind == "stored":
                raw = rng.integers(0, 256, ne, dtype=np.uint8)
                body += ne.to_bytes(4, "little", signed=True) + raw.tobytes()
                filtered.append(raw)
            elif kind == "zero":
                body += bytes(4)
                filtered.append(np.zeros(ne, np.uint8))
            else:
                v = int(rng.integers(1, 256))
                body += (-v).to_bytes(4, "little", signed=True) + b"\x01"
                filtered.append(np.full(ne, v, np.uint8))
        blocks.append(bytes(body))
        pixels.append(unfilter(filt, ts, np.concatenate(filtered)))
    order = np.arange(nblocks) if layout == "natural" else rng.permutation(nblocks)
    at = HEADER_LEN + 4 * nblocks
    bstarts = [0] * nblocks
    payload = bytearray()
    for j in order:
        if layout == "gaps":
            g = int(rng.integers(1, 48))
            payload += rng.integers(0, 256, g, dtype=np.uint8).tobytes()
            at += g
        bstarts[j] = at
        payload += blocks[j]
        at += len(blocks[j])
    cbytes = at
    chunk = bytes(header(codec, ts, nbytes, blocksize, cbytes, filt, split)) + b"".join(
        int(b).to_bytes(4, "little") for b in bstarts) + bytes(payload)
    assert len(chunk) == cbytes
    return chunk, np.concatenate(pixels), counts


def plane_cases():
    """The chunk sets both legs decode: (name, codec, typesize, [chunk kwargs ...]).  Each set is one plane of chunks of the
    same typesize (the window calls need that), the last chunk ragged."""
    cases = []
    layouts = ("natural", "shuffled", "gaps")
    k = 0
    for codec in (LZ4, BLOSCLZ):
        for ts in (1, 2, 3, 4, 8, 16):
            for filt in (NOFILTER, SHUFFLE, BITSHUFFLE):
                split = filt == SHUFFLE and ts > 1
                bs = {1: 8192, 2: 8192, 3: 6144, 4: 16384, 8: 8192, 16: 16384}[ts]
                cases.append(("%s_ts%d_f%d" % (codec, ts, filt), codec, ts, dict(
                    blocksize=bs, chunk=4 * bs + (0 if ts == 16 else 3 * ts), last=bs + 5 * ts + (ts > 1) * 0, filt=filt, split=split,
                    layout=layouts[k % 3], policy="any", flavors=("random", "random", "headtail", "tokens", "long"))))
                k += 1
        for ts in (2, 4):
            cases.append(("%s_lean_ts%d" % (codec, ts), codec, ts, dict(
                blocksize=32768, chunk=4 * 32768, last=32768 + 2 * ts, filt=SHUFFLE, split=True, layout=layouts[k % 3], policy="lean",
                flavors=("random", "headtail", "tokens"))))
            k += 1
    return cases


def zstd_plane_cases():
    """Planes of zstd chunks (codec format 4; every stream one spec-built frame of tests/_zstd_streams.py): typesizes 1, 2, 4, 8, split and
    unsplit, the three filters, leftover blocks and the three layouts; then unsplit blocks of 128 KiB + 15 / 17 / 33 bytes (a
    tight second zstd block in every frame) and blocks of 192 KiB (frames of two blocks)."""
    cases = []
    layouts = ("natural", "shuffled", "gaps")
    flavors = ("raw", "huf", "repeat", "tokens", "blocks", "counts")
    k = 0
    for ts in (1, 2, 4, 8):
        for filt in (NOFILTER, SHUFFLE, BITSHUFFLE):
            split = filt == SHUFFLE and ts > 1
            bs = {1: 8192, 2: 8192, 4: 16384, 8: 32768}[ts]
            cases.append(("zstd_ts%d_f%d" % (ts, filt), ZSTD, ts, dict(
                blocksize=bs, chunk=4 * bs + 3 * ts, last=bs + 5 * ts, filt=filt, split=split, layout=layouts[k % 3],
                policy="any" if k % 2 else "coded", flavors=flavors)))
            k += 1
    cases.append(("zstd_ts4_unsplit_shuffle", ZSTD, 4, dict(blocksize=16384, chunk=3 * 16384 + 8, last=16384 + 4, filt=SHUFFLE, split=False,
                                                            layout="gaps", policy="coded", flavors=flavors)))
    for t in (15, 17, 33):
        cases.append(("zstd_tail%d" % t, ZSTD, 1, dict(blocksize=131072 + t, chunk=131072 + t, last=131072 + t + 5, filt=NOFILTER, split=False,
                                                       layout=layouts[t % 3], policy="all", flavors=("tail", "tail", "huf"), nchunks=2)))
    cases.append(("zstd_192k", ZSTD, 2, dict(blocksize=196608, chunk=196608, last=196608 + 98, filt=SHUFFLE, split=False, layout="shuffled",
                                             policy="all", flavors=("tail", "repeat", "blocks"), nchunks=2)))
    return cases


def wide_cases():
    """Blocks of 128 to 256 KiB: the wide decode kernel, BloscLZ planes beyond 64 KiB with far matches and long headers"""
    return [
        ("blz_wide_ts1", BLOSCLZ, 1, dict(blocksize=262144, chunk=2 * 262144, last=262144 + 777, filt=NOFILTER, split=False,
                                          layout="gaps", policy="coded", flavors=("far", "headtail", "long", "random"))),
        ("blz_wide_ts2_unsplit", BLOSCLZ, 2, dict(blocksize=196608, chunk=2 * 196608, last=196608 + 98, filt=SHUFFLE, split=False,
                                                  layout="shuffled", policy="coded", flavors=("far", "headtail", "random"))),
        ("blz_wide_ts2_split", BLOSCLZ, 2, dict(blocksize=262144, chunk=262144 * 2, last=262144 + 10, filt=SHUFFLE, split=True,
                                                layout="natural", policy="coded", flavors=("far", "headtail", "long", "random"))),
        ("lz4_wide_ts1", LZ4, 1, dict(blocksize=262144, chunk=2 * 262144, last=262144 + 3, filt=NOFILTER, split=False,
                                      layout="shuffled", policy="coded", flavors=("headtail", "long", "random", "tokens"))),
        ("lz4_wide_ts4", LZ4, 4, dict(blocksize=262144, chunk=262144, last=262144 + 44, filt=SHUFFLE, split=True,
                                      layout="gaps", policy="coded", flavors=("headtail", "long", "random"))),
        ("lz4_wide_bitshuffle", LZ4, 4, dict(blocksize=262144, chunk=262144, last=262144 + 36, filt=BITSHUFFLE, split=False,
                                             layout="natural", policy="coded", flavors=("headtail", "long", "random"))),
    ]


def build_plane(name, codec, ts, kw, seed=7, nchunks=4):
    """-> (chunks, plane pixels, kind counts): nchunks chunks (kw['nchunks'] where a case says so), the last one `kw['last']` bytes"""
    nchunks = kw.get("nchunks", nchunks)
    rng = np.random.default_rng([seed, sum(name.encode())])
    chunks, pix = [], []
    counts = {"coded": 0, "stored": 0, "zero": 0, "run": 0}
    for i in range(nchunks):
        nbytes = kw["chunk"] if i < nchunks - 1 else kw["last"]
        c, p, n = make_chunk(rng, codec, ts, kw["blocksize"], nbytes, kw["filt"], kw["split"], kw["layout"], kw["policy"], kw["flavors"])
        chunks.append(c)
        pix.append(p)
        for key in counts:
            counts[key] += n[key]
    return chunks, np.concatenate(pix), counts


def blosclz_ending_in_match(rng, n, far=False):
    """an invalid BloscLZ stream: its last sequence is a match (its length-7 form, or a far one), output exactly n"""
    b = Builder(rng, BLOSCLZ)
    b.lit(16).ensure(BLZ_MAX_NEAR + 300 if far else 200)
    b.lit(4)
    ml = n - b.pos
    assert ml >= 9
    b.match(BLZ_MAX_NEAR + 1 + int(rng.integers(0, 50)) if far else int(rng.integers(1, 60)), ml)
    seqs = b.seqs
    return blosclz_stream(seqs), np.frombuffer(bytes(b.out), np.uint8)


def chunk_of_streams(codec, streams, ts=1, filt=NOFILTER):
    """one unsplit block per stream, every block coded with the given bytes (negative cases)"""
    ne = len(streams[0][1])
    body, bstarts = bytearray(), []
    at = HEADER_LEN + 4 * len(streams)
    for s, ref in streams:
        assert len(ref) == ne
        bstarts.append(at)
        rec = len(s).to_bytes(4, "little") + s
        body += rec
        at += len(rec)
    return bytes(header(codec, ts, ne * len(streams), ne, at, filt, False)) + b"".join(b.to_bytes(4, "little") for b in bstarts) + bytes(body)


def bad_chunks():
    """(name, codec, chunk, bare stream, plane size): streams every decoder must refuse"""
    rng = np.random.default_rng(11)
    out = []
    for far in (False, True):
        n = 20000
        s, ref = blosclz_ending_in_match(rng, n, far)
        good_s, good_ref = random_stream(rng, n, BLOSCLZ)
        good = blosclz_stream(good_s)
        assert len(s) < n and len(good) < n
        out.append(("blosclz_ends_in_%s_match" % ("far" if far else "long"), BLOSCLZ,
                    chunk_of_streams(BLOSCLZ, [(good, good_ref), (s, ref)]), s, n))
    # LZ4: the second match reaches one byte before the block start
    b = Builder(rng, LZ4)
    b.lit(40).match(10, 2000)
    b.lit(20)
    seqs, _ = b.finish(b.pos + 30)
    seqs = list(seqs)
    seqs.insert(1, (b"x" * 5, 40 + 2000 + 6, 100))              # offset = output position + 1
    s = lz4_block(seqs)
    n = 40 + 2000 + 5 + 100 + 20 + 30
    good_s, good_ref = random_stream(rng, n, LZ4)
    out.append(("lz4_offset_before_start", LZ4, chunk_of_streams(LZ4, [(lz4_block(good_s), good_ref), (s, np.zeros(n, np.uint8))]),
                s, n))
    return out
