"""Planes for the head paths of the wave LZ4 encoder (csrc/encode_kernel.h: scalar head, run path, three-probe path, extension,
parked sequences), built from the LZ4 block format and the fast compressor's published search order -- nothing here comes from
another implementation's data.  `model()` is a plain sequential restatement of LZ4_compress_fast (byU16 table, acceleration 1,
no output limit) that also reports what each sequence went through; tests/test_emu_head_masks.py first pins it to the oracle's
bytes and then uses its report to assert that every plane really has the property it was built for."""
import numpy as np

HASH_MUL = 2654435761


def h13(v):
    return ((v * HASH_MUL) & 0xFFFFFFFF) >> 19


def _rd32(s, p):
    return int(s[p]) | int(s[p + 1]) << 8 | int(s[p + 2]) << 16 | int(s[p + 3]) << 24


def _emit(out, lits, off, mlen):
    """one sequence (mlen = match length - 4, or None for the last literals)"""
    ll = len(lits)
    tok = (15 if ll >= 15 else ll) << 4
    if mlen is not None:
        tok |= 15 if mlen >= 15 else mlen
    out.append(tok)
    if ll >= 15:
        r = ll - 15
        out.extend([255] * (r // 255)); out.append(r % 255)
    out.extend(lits)
    if mlen is not None:
        out.extend([off & 255, off >> 8])
        if mlen >= 15:
            r = mlen - 15
            out.extend([255] * (r // 255)); out.append(r % 255)


def model(src):
    """-> (stream bytes, [events]); an event is a dict: probe (-1 post-match probe, k = k-th probe of a search), cand, back, mlen
    (match length - 4), lits, and for searches that start right after a match the hashes' `clean` count of the first three probes."""
    s = [int(x) for x in src] + [0] * 8
    n = len(src)
    out, ev = [], []
    anchor = 0
    if n >= 13:
        mflimit_p1, matchlimit = n - 11, n - 5
        tab = {}
        tab[h13(_rd32(s, 0))] = 0
        ip = 1
        done = False
        while not done:
            # ---- search
            fwd, nb, step, k = ip, 64, 1, 0
            while True:
                ip = fwd
                fwd += step
                step = nb >> 6
                nb += 1
                if fwd > mflimit_p1:
                    done = True
                    break
                hh = h13(_rd32(s, ip))
                m = tab.get(hh, 0)
                tab[hh] = ip
                if _rd32(s, m) == _rd32(s, ip):
                    break
                k += 1
            if done:
                break
            back = 0
            while ip > anchor and m > 0 and s[ip - 1] == s[m - 1]:
                ip -= 1; m -= 1; back += 1
            probe = k
            while True:
                lits = s[anchor:ip]
                ml = 0
                while ip + 4 + ml < matchlimit and s[ip + 4 + ml] == s[m + 4 + ml]:
                    ml += 1
                _emit(out, lits, ip - m, ml)
                e = dict(probe=probe, cand=m, back=back, mlen=ml, lits=len(lits), ip=ip)
                ev.append(e)
                ip += 4 + ml
                anchor = ip
                if ip >= mflimit_p1:
                    done = True
                    break
                if mflimit_p1 - (ip + 1) >= 3 and _rd32(s, ip) != _rd32(s, ip + 1):      # the scalar head's three probes
                    a, b, c = (h13(_rd32(s, ip + i)) for i in range(3))
                    e["clean"] = 1 if b == a else (2 if (c == a or c == b) else 3)
                    e["h"] = (a == b, b == c, a == c)
                tab[h13(_rd32(s, ip - 2))] = ip - 2
                hh = h13(_rd32(s, ip))
                m = tab.get(hh, 0)
                tab[hh] = ip
                if _rd32(s, m) == _rd32(s, ip):
                    probe, back = -1, 0
                    continue
                ip += 1
                break
    _emit(out, s[anchor:n], 0, None)
    return bytes(out), ev


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def fresh(rng, n, avoid=()):
    """n bytes in which no four-byte group repeats (and none of `avoid`, a set of groups): literals that never match"""
    seen = set(avoid)
    out = []
    while len(out) < n:
        b = int(rng.integers(0, 256))
        if len(out) >= 3:
            g = (out[-3], out[-2], out[-1], b)
            if g in seen or len(set(g)) == 1:
                continue
            seen.add(g)
        out.append(b)
    return out


def collide(rng, which):
    """six bytes whose groups v0 = b[0:4], v1 = b[1:5], v2 = b[2:6] differ but share a table slot: which = '10' (h1 == h0),
    '21' (h2 == h1) or '20' (h2 == h0)"""
    while True:
        b = rng.integers(0, 256, (200000, 6), dtype=np.int64)
        v = [b[:, i] | b[:, i + 1] << 8 | b[:, i + 2] << 16 | b[:, i + 3] << 24 for i in range(3)]
        hh = [((x * HASH_MUL) & 0xFFFFFFFF) >> 19 for x in v]
        i, j = int(which[0]), int(which[1])
        other = 3 - i - j
        ok = (hh[i] == hh[j]) & (v[i] != v[j]) & (hh[other] != hh[i]) & (v[0] != v[1])
        idx = np.flatnonzero(ok)
        if idx.size:
            return [int(x) for x in b[idx[0]]]


def planes():
    """[(name, uint8 plane, property)]: property is a predicate over model()'s events, or None"""
    rng = np.random.default_rng(2025)
    P = []

    def add(name, seq, prop=None):
        P.append((name, np.asarray(seq, np.int64).astype(np.uint8), prop))

    # plane lengths around every threshold: flat tiles with a step every few bytes (run path + post-match hits), and literals only
    for n in (13, 14, 16, 17, 76, 77, 80, 255, 256, 257, 258, 259, 260, 261, 16384):
        tile = np.repeat(rng.integers(0, 4, n // 5 + 2), rng.integers(5, 23, n // 5 + 2))[:n]
        add("tiles_%d" % n, tile)
        add("fresh_%d" % n, fresh(rng, n))
        add("flat_%d" % n, [7] * n)
    # a run that ends at matchlimit (n - 5) and one byte either side of it; entered through the run path with an offset-1 match
    # (the run's byte is new) and with a hit of the post-match probe (an older run of the same byte is the candidate)
    for n in (120, 700):
        for d in (-1, 0, 1):
            for older in (0, 1):
                head = ([9] * 8 if older else []) + fresh(rng, 12) + [5] * 20
                end = n - 5 + d
                body = head + [9] * (end - len(head))
                add("run_to_matchlimit%+d_n%d_%s" % (d, n, "hit" if older else "off1"), body + fresh(rng, n - len(body), avoid={(9, 9, 9, 9)}),
                    (lambda ev, older=older: any(e["probe"] == -1 for e in ev)) if older else (lambda ev: any(e["ip"] - e["cand"] == 1 and e["lits"] == 1 for e in ev)))
    # runs longer than 256 bytes: both run-path branches go on into match_more
    for older in (0, 1):
        add("long_run_%d" % older, ([9] * 8 if older else []) + fresh(rng, 12) + [5] * 20 + [9] * 700 + fresh(rng, 40),
            lambda ev: any(e["mlen"] > 256 for e in ev))
    # a candidate at position 0 whose slot still holds the initial zero... and really is the probe's four bytes
    f = fresh(rng, 60)
    add("candidate_zero", f[:40] + [5] * 20 + f[:12] + f[40:], lambda ev: any(e["cand"] == 0 and e["mlen"] >= 4 for e in ev))
    # the first three probes of a search share table slots: every value of `clean`, with and without a real hit in front
    for which in ("10", "21", "20"):
        six = collide(rng, which)
        for hit in (None, 0, 1, 2):
            pre = fresh(rng, 30)
            early = six[hit:hit + 4] if hit is not None else []
            seq = pre[:10] + early + pre[10:] + [5] * 20 + six + fresh(rng, 30)
            want = {"10": 1, "21": 2, "20": 2}[which]
            add("slots_%s_hit%s" % (which, hit), seq, lambda ev, want=want: any(e.get("clean") == want for e in ev))
    add("slots_equal_21", fresh(rng, 20) + [5] * 20 + [3, 8, 8, 8, 8, 8, 8, 8] + fresh(rng, 30), lambda ev: any(e.get("h", (0, 0, 0))[1] for e in ev))
    add("slots_equal_20", fresh(rng, 20) + [5] * 20 + [3, 8, 3, 8, 3, 8, 3, 8] + fresh(rng, 30), lambda ev: any(e.get("h", (0, 0, 0))[2] for e in ev))
    # backward extension of 0, 1 and more than 64 bytes.  More than 64: the search reaches step 3 inside noise, so of a block X
    # only every third position enters the table; X comes again at another phase, is missed until the step grows to 4, and the
    # hit then walks back over everything missed
    add("back_0", fresh(rng, 30) + [5] * 20 + fresh(rng, 30), lambda ev: any(e["back"] == 0 and e["probe"] >= 0 for e in ev))
    for da in range(40):                                  # (the phase of the second copy decides: the first length that does it)
        cand = fresh(rng, 196 + da) + 2 * fresh(rng, 100) + fresh(rng, 20)
        if any(e["back"] > 64 for e in model(cand)[1]):
            add("back_over_64", cand, lambda ev: any(e["back"] > 64 for e in ev))
            break
    for seed in range(400):
        r2 = np.random.default_rng(1000 + seed)
        y = fresh(r2, 24)
        cand = fresh(r2, 10) + y + [5] * 20 + [int(r2.integers(0, 256))] + y[int(r2.integers(1, 4)):] + fresh(r2, 20)
        if any(e["back"] == 1 for e in model(cand)[1]):
            add("back_1", cand, lambda ev: any(e["back"] == 1 for e in ev))
            break
    # 64 and 65 sequences in one plane: the parked lanes are flushed exactly once, with nothing / one sequence left behind
    for want in (64, 65):
        for extra in range(40):
            seq = []
            for i in range(want + extra - 20):
                seq += [i & 255] * 6
            seq += fresh(rng, 16)
            if len(model(seq)[1]) == want:
                add("sequences_%d" % want, seq, lambda ev, want=want: len(ev) == want)
                break
    return P
