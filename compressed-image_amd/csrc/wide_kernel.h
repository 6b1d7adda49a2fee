// wide_kernel.h -- blocks whose streams or staging do not fit the LDS of the normal kernels (blocks up to 256 KiB, LZ4 / LZ4HC /
// zstd / BloscLZ write, LZ4 / LZ4HC / BloscLZ read; zstd read: zstd_walk_kernel.h's replay out of a device-memory slot).  wide_plan.h
// decides which batches come here; engine.hip launches the kernels.
//
//   cimg_encode_wide   persistent single-wave workgroups pull streams from one atomic counter.  A stream that needs the byte
//                      shuffle is staged into the wave's own plane in device memory (a stream that is a plain slice of the
//                      pixels is read where it lies); the LZ4 hash table stays in LDS.  The encoder is liblz4 1.9.3's
//                      LZ4_compress_fast walked in wave-uniform order -- the byU16 regime below 65 547 bytes (8192 x u16,
//                      LZ4_hash4), the byU32 regime from there on (4096 x u32, LZ4_hash5, candidates more than 65 535 bytes
//                      back rejected) -- with the 64 lanes used for match extension and literal copies.  Records and
//                      payloads go to the scratch slots exactly as the normal encoder leaves them; cimg_layout_chunks /
//                      cimg_emit_blocks put the chunks together behind the launch.
//   cimg_decode_wide   persistent 256-thread workgroups, each owning one block-sized scratch slot in device memory, walk the
//                      batch's blocks.  The block body is DecodeBlock (decode_kernel.h) with its "LDS" in the slot: the same
//                      header walk (WideDecodeBlock below: each stream decoded relative to its own region), the same wave
//                      decoders and unshuffle, so every bound it keeps (comp_size / cbytes on reads, the slot size on writes)
//                      holds as it does there.
//                      Matches are copied from the slot, at most 64 KiB (LZ4) / ~72 KiB (BloscLZ far) back: L2-resident.
//                      A block of a zstd chunk (codec format 4) is left with STATUS_ZSTD_PENDING[_SPLIT], as cimg_decode_blocks
//                      leaves it: the engine then runs the zstd read path's walk over those blocks and cimg_zstd_replay_wide,
//                      the replay with its planes in a device-memory slot per workgroup (zstd_walk_kernel.h).
//   cimg_encode_wide_zstd  the same persistent waves and staging as cimg_encode_wide; each stream becomes one zstd frame of
//                      ceil(n / 128 KiB) blocks (zstd_wide_encode below, the frame writer of zstd_encode.h).
//   cimg_encode_wide_blosclz  the same persistent waves and staging; each stream goes through blosclz_wide_encode below: the windowed
//                      scan of blosclz_kernel.h over a stream in device memory, with a table of 32-bit positions in the same
//                      16 KiB of LDS.  Bytes are those of BloscLZ 2.3.0 at every length up to 256 KiB.
#pragma once
#include "encode_kernel.h"

namespace cimg {

enum : int {
    WIDE_MAX_BLOCK = 262144,             // largest block the wide kernels take (the planner refuses anything above)
    LZ4_U32_HASHLOG = 12,                // liblz4: LZ4_HASHLOG - 1 for the byU32 table (4096 entries, the same 16 KiB)
    LZ4_U16_HASHLOG = 13,
    LZ4_LIMIT_64K = 65536 + 12 - 1,      // liblz4 LZ4_64Klimit: from this input size on the byU32 regime is used
    LZ4_DIST_MAX = 65535,
};

struct WideEncodeArgs {
    const ChunkDesc* descs;
    int32_t nchunks;
    CodecParams p;
    const uint8_t* raw;        // pixels at raw + desc.raw_off
    uint8_t* scratch;          // block b owns scratch + b * p.slot_bytes (as EncodeArgs)
    StreamRec* recs;           // block b, stream s -> recs[b * p.streams_per_block + s]
    int32_t total_blocks;
    int32_t uniform_nblocks;
    uint8_t* planes;           // wave w stages a shuffled stream at planes + w * plane_stride
    int64_t plane_stride;
    uint32_t* queue;           // one counter, zero at launch
};

struct WideDecodeArgs {
    DecodeArgs d;              // d.lds_bytes = slot bytes; d.done / d.skipped unused
    uint8_t* slots;            // workgroup k owns slots + k * d.lds_bytes
};

CIMG_DEV uint32_t wide_rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
CIMG_DEV uint64_t wide_rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

// bytes in[a + k] == in[b + k] for k = 0, 1, ... while a + k < limit: 64 compares per step
CIMG_DEV int wide_common(const uint8_t* in, int a, int b, int limit)
{
    int k = 0;
    for (;;) {
        LV<bool> diff;
        FOR_LANES(l) { const int i = a + k + l; diff[l] = i >= limit || in[i < limit ? i : a] != in[i < limit ? b + k + l : a]; }
        const uint64_t m = ballot(diff);
        if (m) return k + ctz64(m);
        k += 64;
    }
}

CIMG_DEV void wide_copy(const uint8_t* src, uint8_t* dst, int n)
{
    for (int k = 0; k < n; k += 64) { FOR_LANES(l) { if (k + l < n) dst[k + l] = src[k + l]; } }
}

// an LZ4 length extension of `rem` (rem / 255 bytes 255, then rem % 255) at out[op..); returns the new op
CIMG_DEV int wide_len_ext(uint8_t* out, int op, int rem)
{
    const int full = rem / 255;
    for (int k = 0; k < full; k += 64) { FOR_LANES(l) { if (k + l < full) out[op + k + l] = 255; } }
    LV<int> z;
    FOR_LANES_W(l) { z[l] = 0; if (l == 0) out[op + full] = (uint8_t)(rem - 255 * full); }
    return op + full + 1;
}

CIMG_DEV uint32_t wide_hash(const uint8_t* p, bool u32)
{
    if (u32) return (uint32_t)(((wide_rd64(p) << 24) * 889523592379ull) >> (64 - LZ4_U32_HASHLOG));
    return (wide_rd32(p) * 2654435761u) >> (32 - LZ4_U16_HASHLOG);
}

// Bit-exact LZ4_compress_fast(in, out, n, cap, accel) of liblz4 1.9.3 (noDict, 64-bit host), either table regime.
// tab: 16 KiB of LDS.  Returns bytes written, 0 if the result does not fit cap (limited-output mode); need_out = the
// smallest cap under which it still succeeds (the maximum of the limited-output checks' left-hand sides).
CIMG_DEV int lz4_wide_encode(const uint8_t* in, uint32_t* tab, int n, uint8_t* out, int cap, int accel, int& need_out)
{
    enum { MINMATCH = 4, MFLIMIT = 12, LASTLITERALS = 5, ML_BITS = 4, ML_MASK = 15, RUN_MASK = 15, SKIP_TRIGGER = 6 };
    if (accel < 1) accel = 1;
    if (accel > 65537) accel = 65537;
    const bool u32 = n >= LZ4_LIMIT_64K;
    const bool limited = cap < n + n / 255 + 16;
    uint16_t* tab16 = reinterpret_cast<uint16_t*>(tab);
    for (int k = 0; k < 4096; k += 64) { FOR_LANES(l) { tab[k + l] = 0; } }
    int ip = 0, anchor = 0, op = 0, need = 0;
    const int mflimit_p1 = n - MFLIMIT + 1, matchlimit = n - LASTLITERALS;
    auto get = [&](uint32_t h) -> int { return u32 ? (int)tab[h] : (int)tab16[h]; };
    auto put = [&](uint32_t h, int pos) { LV<int> z; FOR_LANES_W(l) { z[l] = 0; if (l == 0) { if (u32) tab[h] = (uint32_t)pos; else tab16[h] = (uint16_t)pos; } } };
    if (n >= MFLIMIT + 1) {
        put(wide_hash(in, u32), 0);
        ip = 1;
        for (;;) {
            int match = 0;
            {   // search: probe positions with the skip schedule
                int probe = ip, step = 1, nb = accel << SKIP_TRIGGER;
                for (;;) {
                    const int cur = probe, next = cur + step;
                    step = nb++ >> SKIP_TRIGGER;
                    if (next > mflimit_p1) goto last_literals;
                    const uint32_t h = wide_hash(in + cur, u32);
                    match = get(h);
                    put(h, cur);
                    probe = next;
                    if (u32 && match + LZ4_DIST_MAX < cur) continue;
                    if (wide_rd32(in + match) == wide_rd32(in + cur)) { ip = cur; break; }
                }
            }
            while (ip > anchor && match > 0 && in[ip - 1] == in[match - 1]) { ip--; match--; }
            int token_pos, token;
            {   // literals
                const int lit = ip - anchor;
                token_pos = op++;
                const int lhs = op + lit + (2 + 1 + LASTLITERALS) + lit / 255;
                if (limited && lhs > cap) return 0;
                need = imax(need, lhs);
                if (lit >= RUN_MASK) { token = RUN_MASK << ML_BITS; op = wide_len_ext(out, op, lit - RUN_MASK); }
                else token = lit << ML_BITS;
                wide_copy(in + anchor, out + op, lit);
                op += lit;
            }
            for (;;) {
                {   // offset + match length
                    const int off = ip - match;
                    LV<int> z;
                    FOR_LANES_W(l) { z[l] = 0; if (l == 0) { out[op] = (uint8_t)(off & 0xFF); out[op + 1] = (uint8_t)(off >> 8); } }
                    op += 2;
                    int mcode = wide_common(in, ip + MINMATCH, match + MINMATCH, matchlimit);
                    ip += mcode + MINMATCH;
                    const int lhs = op + (1 + LASTLITERALS) + (mcode + 240) / 255;
                    if (limited && lhs > cap) return 0;
                    need = imax(need, lhs);
                    if (mcode >= ML_MASK) { token += ML_MASK; op = wide_len_ext(out, op, mcode - ML_MASK); }
                    else token += mcode;
                    FOR_LANES_W(l) { z[l] = 0; if (l == 0) out[token_pos] = (uint8_t)token; }
                }
                anchor = ip;
                if (ip >= mflimit_p1) goto last_literals;
                put(wide_hash(in + ip - 2, u32), ip - 2);
                // the position right after the match
                const uint32_t h = wide_hash(in + ip, u32);
                match = get(h);
                put(h, ip);
                if ((!u32 || match + LZ4_DIST_MAX >= ip) && wide_rd32(in + match) == wide_rd32(in + ip)) {
                    token_pos = op++;
                    token = 0;
                    continue;
                }
                break;
            }
            ip++;
        }
    }
last_literals:
    {
        const int run = n - anchor;
        const int lhs = op + run + 1 + (run + 255 - RUN_MASK) / 255;
        if (limited && lhs > cap) return 0;
        need = imax(need, lhs);
        LV<int> z;
        if (run >= RUN_MASK) {
            FOR_LANES_W(l) { z[l] = 0; if (l == 0) out[op] = (uint8_t)(RUN_MASK << ML_BITS); }
            op = wide_len_ext(out, op + 1, run - RUN_MASK);
        } else {
            FOR_LANES_W(l) { z[l] = 0; if (l == 0) out[op] = (uint8_t)(run << ML_BITS); }
            op++;
        }
        wide_copy(in + anchor, out + op, run);
        op += run;
    }
    need_out = need;
    return op;
}

// ---- BloscLZ on the wide route ----------------------------------------------------------------------------------------------------
// blosclz_wide_encode is blosclz_encode_body (blosclz_kernel.h) restated for a stream in device memory: the same windows of 64
// positions, collision rule, commit bound, 12-byte look-ahead, parked sequences and counting probe passes, with three differences.
//   * The table holds 4096 x uint32 positions (16 KiB of LDS, the table of the other wide encoders), so a stream may be 256 KiB long.
//   * A candidate MAX_FARDISTANCE (65 535 + 8191 - 1) or more bytes back is no hit; its slot is overwritten all the same.  (Below
//     64 KiB no candidate is that far, which is why the normal-path encoder has no such check.)
//   * The stream is read where it lies, and NO load touches a byte outside [in, in + n): a stream that is a plain slice of the
//     caller's pixels may end with the caller's allocation.  Every dword load whose index is not provably at most n - 4 goes through
//     blzw_ld32, which CLAMPS the index to n - 4 and shifts the bytes down; the bytes it makes up beyond the stream's end lie where
//     the codec's own bound (ip_bound = n - 1) has already cut the comparison.  Byte loads are guarded by their counts.
enum : int { BLZ_MAX_FARDISTANCE = 65535 + BLZ_MAX_DISTANCE - 1 };

// the four bytes in[idx .. idx + 4) of a stream of n >= 4 bytes, idx >= 0; bytes at n and beyond read as zero
CIMG_DEV uint32_t blzw_ld32(const uint8_t* in, int idx, int n)
{
    const int c = imin(idx, n - 4);
    const int over = idx - c;
    return over >= 4 ? 0u : wide_rd32(in + c) >> (8 * over);
}

// blz_count on device memory: equal bytes in[a + k] == in[b + k], k = 0 .. maxc - 1, b < a, a + maxc <= n
CIMG_DEV int blzw_count(const uint8_t* in, int a, int b, int maxc, int n)
{
    int cnt = 0;
    for (int it = 0; it <= n / 256 + 1; ++it) {
        LV<int> len;
        LV<bool> stop;
        FOR_LANES(l) {
            const int k = cnt + 4 * l;
            const uint32_t x = blzw_ld32(in, a + k, n) ^ blzw_ld32(in, b + k, n);
            const int ln = imin(x ? (int)(__builtin_ctz(x) >> 3) : 4, imax(maxc - k, 0));
            len[l] = ln;
            stop[l] = ln < 4;
        }
        const uint64_t sm = ballot(stop);
        if (sm) { const int f = ctz64(sm); return cnt + 4 * f + readlane(len, f); }
        cnt += 256;
    }
    return imin(cnt, maxc);
}

// Bit-exact blosclz_compress(clevel, in, n, out, cap) by one wave for 0 <= n <= WIDE_MAX_BLOCK.  in: device memory, exactly n
// readable bytes; tab: 16 KiB of LDS.  Returns bytes written, 0 if the codec gives up / the result does not fit, < 0 if a loop
// guard tripped.  need_out = smallest cap that still succeeds (max(66, size + 1): blosclz_kernel.h says why).
CIMG_DEV int blosclz_wide_encode(const uint8_t* in, uint32_t* tab, int n, uint8_t* out_generic, int cap, int clevel, int& need_out)
{
    cimg_global_u8p out = CIMG_AS_GLOBAL(out_generic);
    cimg_lds_vu32p tab32 = CIMG_AS_LDS_VU32(tab);
    need_out = 0;
    if (n < 16 || cap < 66 || clevel < 1 || clevel > 9) return 0;
    const int hashlog = clevel == 1 ? BLZ_HASH_LOG - 2 : (clevel == 2 ? BLZ_HASH_LOG - 1 : BLZ_HASH_LOG);
    const int minlen_tab = clevel <= 2 ? 12 : 14 - clevel;
    const int maxlen = n >> 3;
    int pass = clevel == 9 ? 0 : 1;                                   // level 9 probes with ipshift 3 and 4, the others with 4; then the real scan
    int csize3 = 0, csize4 = 0, ipshift = 4;

    LV<int> P_anchor, P_lit, P_dist, P_len;
    FOR_LANES(l) { P_anchor[l] = 0; P_lit[l] = 0; P_dist[l] = 0; P_len[l] = 0; }
    int np = 0, op = 0;
    int anchor = 0;
    int ending = 1;                                                   // 1: go on; 0: give up (stored raw); < 0: a loop guard tripped
    bool saw_hit = false;
    for (; pass < 3; ++pass) {
        const bool probe = pass < 2;
        if (pass == 2) {
            const int cs = clevel == 9 ? imin(csize3, csize4) : csize4;
            ipshift = (clevel == 9 && csize3 < csize4) ? 3 : 4;
            const double cratio = (double)maxlen / (double)cs;
            const double thr = clevel <= 4 ? 2.0 : (clevel == 5 ? 1.8 : (clevel == 6 ? 1.6 : (clevel == 7 ? 1.4 : (clevel == 8 ? 1.2 : 1.1))));
            if (cratio < thr) { ending = 0; break; }
        }
        const int shift = probe ? 32 - BLZ_HASH_LOG : 32 - hashlog;
        const int ips = probe ? (pass == 0 ? 3 : 4) : ipshift;
        const int minlen = probe ? 3 : (clevel == 9 ? ipshift : minlen_tab);
        const int nlim = probe ? maxlen : n;
        const int ip_bound = nlim - 1, ip_limit = nlim - 12;
        for (int k = 0; k < 4096; k += 64) { FOR_LANES(l) { tab32[k + l] = 0; } }
        int ip = probe ? 0 : 4;
        anchor = 0;
        int oc = 5, copyc = 4;                                        // the probe's counters ("4 literals already copied")
        int guard = 0;
        while (ip < ip_limit) {
            if (++guard > n + 2) { ending = -1; break; }              // a window consumes at least one position
            const int nv = imin(64, ip_limit - ip);
            LV<int> pos;
            LV<bool> valid;
            LV<uint32_t> v, h;
            FOR_LANES(l) {
                pos[l] = ip + l;
                valid[l] = l < nv;
                v[l] = wide_rd32(in + (l < nv ? ip + l : 0));          // (ip + l < nlim - 12)
                h[l] = blz_hash(v[l], shift);
            }
            LV<uint32_t> ph, pv;
            lane_prev(h, ph);
            lane_prev(v, pv);
            LV<bool> head, cont;
            LV<uint32_t> old;
            FOR_LANES(l) {
                cont[l] = valid[l] && l > 0 && h[l] == ph[l];
                head[l] = valid[l] && !cont[l];
                old[l] = tab32[h[l]];
            }
            FOR_LANES_W(l) { if (head[l]) tab32[h[l]] = (uint32_t)pos[l]; }
            LV<bool> loser, hit;
            LV<int> cand;
            FOR_LANES(l) {
                const uint32_t rb = tab32[h[l]];
                const uint32_t mvh = wide_rd32(in + old[l]);           // (a table entry is a position below an ip_limit, or 0)
                const uint32_t mv = head[l] ? mvh : pv[l];
                loser[l] = head[l] && rb != (uint32_t)pos[l];
                cand[l] = head[l] ? (int)old[l] : pos[l] - 1;
                // distance 0: position 0 against the empty table; MAX_FARDISTANCE and beyond: not a hit, the slot is written all the same
                hit[l] = valid[l] && mv == v[l] && cand[l] != pos[l] && pos[l] - cand[l] < BLZ_MAX_FARDISTANCE;
            }
            uint64_t involved = ballot(loser);
            if (involved) {
                FOR_LANES_W(l) { if (loser[l]) tab32[h[l]] = (uint32_t)pos[l]; }
                LV<bool> inv;
                FOR_LANES(l) { inv[l] = head[l] && (loser[l] || tab32[h[l]] != (uint32_t)pos[l]); }
                involved = ballot(inv);
            }
            const int k1 = ctz64(involved);
            const int limit = imin(nv - 1, k1);
            const uint64_t below = limit >= 63 ? ~0ull : ((1ull << (limit + 1)) - 1);
            const uint64_t hits = ballot(hit) & below;
            int m = -1;
            if (hits) {
                saw_hit = true;
                // a 4-byte hit is a match only if it is long enough: the next 12 bytes decide every rule
                LV<bool> acc;
                FOR_LANES(l) {
                    const int a = hit[l] ? pos[l] + 4 : 0, b = hit[l] ? cand[l] + 4 : 0;
                    const uint32_t x0 = blzw_ld32(in, a, n) ^ blzw_ld32(in, b, n);
                    const uint32_t x1 = blzw_ld32(in, a + 4, n) ^ blzw_ld32(in, b + 4, n);
                    const uint32_t x2 = blzw_ld32(in, a + 8, n) ^ blzw_ld32(in, b + 8, n);
                    const int kk = x0 ? (int)(__builtin_ctz(x0) >> 3) : (x1 ? 4 + (int)(__builtin_ctz(x1) >> 3) : (x2 ? 8 + (int)(__builtin_ctz(x2) >> 3) : 12));
                    const int room = ip_bound - (pos[l] + 4);
                    const int lenlb = 4 + imin(kk + 1, room) - ips;            // exact below 13, a lower bound from there
                    const bool far = pos[l] - cand[l] - 1 >= BLZ_MAX_DISTANCE;
                    const bool ok = probe ? lenlb >= (far ? 4 : 3) : (lenlb >= minlen && !(lenlb <= 5 && far));
                    acc[l] = hit[l] && ok;
                }
                const uint64_t am = ballot(acc) & below;
                if (am) m = ctz64(am);
            }
            const int B = m >= 0 ? m : limit;
            const uint64_t headmask = ballot(head), contmask = ballot(cont);
            const uint64_t above = B >= 63 ? 0ull : (~0ull << (B + 1));
            if (headmask & above) {
                FOR_LANES_W(l) { if (head[l] && l > B) tab32[h[l]] = old[l]; }
                FOR_LANES_W(l) { if (head[l] && l == B) tab32[h[l]] = (uint32_t)pos[l]; }
            }
            if (contmask & ~above) {
                FOR_LANES_W(l) {
                    if (cont[l] && l <= B && (l == B || !((contmask >> ((l + 1) & 63)) & 1) || l == 63)) tab32[h[l]] = (uint32_t)pos[l];
                }
            }
            if (m < 0) { ip += B + 1; continue; }
            // ---- a match at lane m ------------------------------------------------------------------------------
            const int mpos = readlane(pos, m), mref = readlane(cand, m);
            const int room = ip_bound - (mpos + 4);
            const int k = blzw_count(in, mpos + 4, mref + 4, room, n);
            const int nip = mpos + 4 + (k < room ? k + 1 : room) - ips;
            const int len = nip - mpos, dist = mpos - mref - 1, L = mpos - anchor;
            if (probe) {
                const int t = copyc + L;
                oc += L + (t >> 5);
                if ((t & 31) == 0) oc--;
                copyc = 0;
                oc += (len >= 7 ? blz_div255(len - 7) + 1 : 0) + (dist >= BLZ_MAX_DISTANCE ? 4 : 2) + 1;
            } else {
                const int slot = np;
                FOR_LANES(l) { if (l == slot) { P_anchor[l] = anchor; P_lit[l] = L; P_dist[l] = dist; P_len[l] = len; } }
                if (++np == 64) {
                    if (!blz_emit_pending(in, out, cap, op, np, P_anchor, P_lit, P_dist, P_len)) { ending = 0; break; }
                    np = 0;
                }
            }
            {   // "update the hash at match boundary": positions nip and nip + 1 (nip <= nlim - 1 - ips: four bytes are there)
                LV<uint32_t> s2;
                FOR_LANES(l) { s2[l] = wide_rd32(in + nip); }
                FOR_LANES_W(l) { tab32[blz_hash(s2[l], shift)] = (uint32_t)nip; }
                FOR_LANES_W(l) { tab32[blz_hash(s2[l] >> 8, shift)] = (uint32_t)(nip + 1); }
            }
            ip = nip + 2;
            anchor = ip;
        }
        if (ending <= 0) break;
        if (probe) {
            const int Lc = imax(ip_limit - anchor, 0);
            const int t = copyc + Lc;
            oc += Lc + (t >> 5);
            if ((t & 31) == 0) oc--;
            if (pass == 0) csize3 = oc; else csize4 = oc;
            // (a first probe that never met four equal bytes is the second one too: blosclz_kernel.h)
            if (pass == 0 && !saw_hit) { csize4 = csize3; pass = 1; }
        }
    }
    if (ending <= 0) return ending;
    if (np && !blz_emit_pending(in, out, cap, op, np, P_anchor, P_lit, P_dist, P_len)) return 0;
    const int Lf = n - anchor;
    const int size = op + blz_lit_bytes(Lf);
    if (size + 1 > cap) return 0;
    blz_emit_literals(in, anchor, out, op, Lf);
    need_out = imax(66, size + 1);
    return size;
}

// true if all n bytes equal the first (any alignment)
CIMG_DEV bool wide_is_run(const uint8_t* in, int n, uint32_t& value)
{
    LV<uint32_t> first;
    FOR_LANES(l) { first[l] = in[0]; }
    value = readlane(first, 0);
    const uint32_t w = value * 0x01010101u;
    const int units = n >> 4;
    for (int c = 0; c < units; c += 64) {
        LV<bool> bad;
        FOR_LANES(l) {
            const u128 q = ld128u(in + 16 * (c + l < units ? c + l : 0));
            bad[l] = (c + l < units) & ((q.x != w) | (q.y != w) | (q.z != w) | (q.w != w));
        }
        if (ballot(bad)) return false;
    }
    LV<bool> bad;
    FOR_LANES(l) { bad[l] = 16 * units + l < n && in[16 * units + l] != (uint8_t)value; }
    return ballot(bad) == 0;
}

// what the zstd instance of the wave needs beside WideEncodeArgs
struct WideZstdEncodeArgs {
    WideEncodeArgs w;
    uint64_t* seq;             // wave w keeps the sequences of the zstd block it is coding at seq + w * seq_stride
    int64_t seq_stride;        // (records: ZSTD_BLOCK_MAX / 4, a match is at least four bytes long)
    const ZstdEncTables* tables;
};
enum : int { WIDE_ZSTD_SEQ_STRIDE = ZSTD_BLOCK_MAX / 4 + 64,
             WIDE_ZSTD_LDS = LZ4_HASH_BYTES + (int)((sizeof(ZstdEncTables) + 63) & ~(size_t)63) };   // hash table, FSE tables

// One stream -> one zstd frame of ceil(n / 128 KiB) blocks at out[0, cap) (zstd_encode.h: the frame writer).  Greedy matches from a
// 4096-slot table of 32-bit positions (LZ4_hash5 over five bytes, the byU32 table of lz4_wide_encode) over the whole stream: an
// offset reaches back to the stream's first byte, a match ends at its zstd block's end.  A block whose compressed form is not
// smaller than itself is written as a Raw_Block.  Returns the frame size, 0 when the frame is not smaller than n or does not fit cap.
// tab: 16 KiB of LDS; T: the FSE tables (LDS); seq: ZSTD_BLOCK_MAX / 4 records of device memory.
CIMG_DEV int zstd_wide_encode(const uint8_t* in, uint32_t* tab, const ZstdEncTables* T, int n, uint8_t* out_, int cap, uint64_t* seq)
{
    enum { MINMATCH = 4, SKIP_TRIGGER = 6 };
    cimg_global_u8p out = CIMG_AS_GLOBAL(out_);
    const int fh = zstd_frame_header_bytes(n);
    if (n < 64 || fh + 64 >= cap) return 0;
    for (int k = 0; k < 4096; k += 64) { FOR_LANES(l) { tab[k + l] = 0; } }
    auto put = [&](uint32_t h, int pos) { FOR_LANES_W(l) { if (l == 0) tab[h] = (uint32_t)pos; } };
    const int probe_end = n - 8;                    // (the hash reads eight bytes)
    int op = fh;
    uint32_t rep = 1;                               // the decoder's first repeat offset in front of the next compressed block
    put(wide_hash(in, true), 0);
    for (int blk0 = 0; blk0 < n; blk0 += ZSTD_BLOCK_MAX) {
        const int bend = imin(n, blk0 + ZSTD_BLOCK_MAX), bsz = bend - blk0;
        const bool last = bend == n;
        const int lit_at = op + 6;                  // block header, raw literals header, then the literals
        int lit = 0, nseq = 0, anchor = blk0;
        int ip = blk0 == 0 ? 1 : blk0;
        const int limit = imin(probe_end, bend - MINMATCH);
        bool fits = true;
        while (ip <= limit && fits) {
            int match = 0, cur = ip, nb = 1 << SKIP_TRIGGER;
            bool found = false;
            for (; cur <= limit; ) {                // probe with LZ4's skip schedule
                const uint32_t h = wide_hash(in + cur, true);
                match = (int)uni(tab[h]);
                put(h, cur);
                if (match < cur && wide_rd32(in + match) == wide_rd32(in + cur)) { found = true; break; }
                cur += nb++ >> SKIP_TRIGGER;
            }
            if (!found) break;
            while (cur > anchor && match > 0 && in[cur - 1] == in[match - 1]) { cur--; match--; }
            // (a match may cover a whole zstd block -- 131 072 bytes: the record's 17-bit length field takes one byte less, and the
            // rest of the match is found again as the next sequence)
            const int ml = imin(MINMATCH + wide_common(in, cur + MINMATCH, match + MINMATCH, bend), ZSTD_WIDE_MAX_LEN);
            const int ll = cur - anchor;
            if (lit_at + lit + ll + 64 > cap) { fits = false; break; }
            wide_copy(in + anchor, out_ + lit_at + lit, ll);
            lit += ll;
            const uint64_t r = zstd_wide_rec(ll, ml, cur - match);
            FOR_LANES_W(l) { if (l == 0) seq[nseq] = r; }
            nseq++;
            ip = anchor = cur + ml;
            if (ip - 2 <= probe_end) put(wide_hash(in + ip - 2, true), ip - 2);
        }
        int content = 0;                            // Block_Content bytes of a compressed block (0: the block goes raw)
        if (fits && nseq > 0) {
            const int tail = bend - anchor;
            if (lit_at + lit + tail + 64 <= cap) {
                wide_copy(in + anchor, out_ + lit_at + lit, tail);
                lit += tail;
                const int sb = zstd_wide_sequences(seq, nseq, rep, T, out, lit_at + lit, imin(cap, op + 3 + bsz));
                if (sb > 0) content = 3 + lit + sb;
            }
        }
        if (content > 0 && content < bsz) {
            zstd_put24(out, op, (last ? 1u : 0u) | (2u << 1) | ((uint32_t)content << 3));      // Compressed_Block
            zstd_put24(out, op + 3, (3u << 2) | ((uint32_t)lit << 4));                          // Raw_Literals_Block, 20-bit size
            op += 3 + content;
            rep = (uint32_t)(seq[nseq - 1] >> 34);
        } else {
            if (op + 3 + bsz > cap) return 0;
            zstd_put24(out, op, (last ? 1u : 0u) | ((uint32_t)bsz << 3));                       // Raw_Block
            wide_copy(in + blk0, out_ + op + 3, bsz);
            op += 3 + bsz;
        }
        if (op >= n) return 0;
    }
    zstd_put_frame_header(out, n);
    return op;
}

// one wave: pulls streams until the counter passes the last one (CODEC_LZ4: cimg_encode_wide, every LZ4 / LZ4HC batch;
// CODEC_ZSTD: cimg_encode_wide_zstd, with z; CODEC_BLOSCLZ: cimg_encode_wide_blosclz)
template <int CODEC>
struct WideEncodeWaveT {
    const WideEncodeArgs& a;
    uint32_t* tab;             // 16 KiB of LDS (zstd: the FSE tables behind it)
    int w;
    const WideZstdEncodeArgs* z = nullptr;

    CIMG_DEV WideEncodeWaveT(const WideEncodeArgs& a_, uint32_t* tab_, int w_) : a(a_), tab(tab_), w(w_) {}
    CIMG_DEV WideEncodeWaveT(const WideZstdEncodeArgs& z_, uint32_t* tab_, int w_) : a(z_.w), tab(tab_), w(w_), z(&z_)
    {
        // the FSE tables of the predefined distributions -> LDS behind the hash table
        const uint32_t* src = reinterpret_cast<const uint32_t*>(z_.tables);
        uint32_t* dst = tab + LZ4_HASH_BYTES / 4;
        const int words = (int)(sizeof(ZstdEncTables) / 4);
        for (int w0 = 0; w0 < words; w0 += 64) { FOR_LANES(l) { if (w0 + l < words) dst[w0 + l] = src[w0 + l]; } }
    }

    CIMG_DEV void run()
    {
        const int items = a.total_blocks * a.p.streams_per_block;
        for (int pops = 0; pops <= items; ++pops) {
            LV<uint32_t> got;
            FOR_LANES(l) { got[l] = 0; }
            FOR_LANES_W(l) { if (l == 0) got[l] = atomic_add_agent(a.queue, 1u); }
            const int item = (int)uni(readlane(got, 0));
            if (item >= items) break;
            run_item(item / a.p.streams_per_block, item % a.p.streams_per_block);
        }
    }

    CIMG_DEV void run_item(int b, int s)
    {
        const int chunk = find_chunk(a.descs, a.nchunks, b, a.uniform_nblocks);
        const ChunkDesc d = uniform_desc(a.descs + chunk);
        if (d.memcpyed) return;
        const int j = b - d.blk0;
        const int ts = a.p.typesize;
        const bool leftover_blk = j == d.nblocks - 1 && d.leftover;
        const int bsize = leftover_blk ? d.leftover : d.blocksize;
        const int ns = (d.split && !leftover_blk) ? ts : 1;
        if (s >= ns) return;
        const int n = bsize / ns;
        const uint8_t* src = a.raw + d.raw_off + (int64_t)j * d.blocksize;
        const uint8_t* in;
        if (a.p.filter == FILTER_SHUFFLE && ts > 1) {
            // stage the stream: byte s of every element (a split plane), or the whole shuffled block
            uint8_t* plane = a.planes + (int64_t)w * a.plane_stride;
            const int ne = bsize / ts;
            if (ns > 1) {
                for (int e0 = 0; e0 < n; e0 += 64) { FOR_LANES(l) { const int e = e0 + l; if (e < n) plane[e] = src[(int64_t)e * ts + s]; } }
            } else {
                for (int o0 = 0; o0 < bsize; o0 += 64) {
                    FOR_LANES(l) {
                        const int o = o0 + l;
                        if (o < bsize) plane[o] = o < ne * ts ? src[(int64_t)(o % ne) * ts + o / ne] : src[o];
                    }
                }
            }
            in = plane;
        } else {
            in = src + (int64_t)s * n;                  // no shuffle: stream s is slice s of the block
        }
        uint8_t* out = a.scratch + (int64_t)b * a.p.slot_bytes + (int64_t)s * n;
        StreamRec r;
        r.kind = REC_RAW; r.value = 0; r.csize = n; r.need = 0;
        uint32_t value;
        if (wide_is_run(in, n, value)) {
            r.kind = REC_RUN; r.value = (int32_t)value; r.csize = 0;
        } else {
            int need = 0;
            int cb;
            if constexpr (CODEC == CODEC_ZSTD) {
                cb = zstd_wide_encode(in, tab, reinterpret_cast<const ZstdEncTables*>(tab + LZ4_HASH_BYTES / 4), n, out, n,
                                      z->seq + (int64_t)w * z->seq_stride);
                need = cb;                                // (a frame fits a budget iff the budget holds its bytes)
            } else if constexpr (CODEC == CODEC_BLOSCLZ) cb = blosclz_wide_encode(in, tab, n, out, n, a.p.clevel, need);
            else cb = lz4_wide_encode(in, tab, n, out, n, a.p.accel, need);
            if (cb > 0 && cb < n) { r.kind = REC_LZ4; r.csize = cb; r.need = need; }
            else wide_copy(in, out, n);
        }
        StreamRec* dst = a.recs + (int64_t)b * a.p.streams_per_block + s;
        FOR_LANES_W(l) { if (l == 0) *dst = r; }
    }
};
using WideEncodeWave = WideEncodeWaveT<CODEC_LZ4>;

// One block of cimg_decode_wide: DecodeBlock (decode_kernel.h) with its "LDS" in a device-memory slot.  The header walk is
// DecodeBlock::phase_a with one difference: every stream is decoded with its own region as the decoder's base.  The wave decoders
// pack LDS offsets into 18 bits (lz4_decode_wave2 / blosclz_decode_wave: "LDS offsets are below 2^18"), which holds for a region
// of up to 256 KiB of output but not for the second plane of a two-plane 256 KiB block seen from the slot's start.
struct WideDecodeBlock : DecodeBlock {
    CIMG_DEV WideDecodeBlock(const DecodeArgs& a_, uint8_t* slot_, int b_) : DecodeBlock(a_, slot_, b_) {}

    CIMG_DEV void phase_a_wide(int wave)
    {
        mode = 3;
        chunk = find_chunk(a.descs, a.nchunks, b, a.uniform_nblocks);
        const ChunkDesc d = uniform_desc(a.descs + chunk);
        j = b - d.blk0;
        c = a.comp + d.comp_off;
        out = a.raw + d.raw_off + (int64_t)j * d.blocksize;
        bsize = (j == d.nblocks - 1 && d.leftover) ? d.leftover : d.blocksize;
        const u128 h0 = ld128u(c), h1 = ld128u(c + 16);
        const uint32_t w0 = uni(h0.x);
        const int flags = (int)((w0 >> 16) & 0xFF);
        ts = (int)(w0 >> 24);
        const int nbytes = (int)uni(h0.y), blocksize = (int)uni(h0.z), cbytes = (int)uni(h0.w);
        const uint32_t f0 = uni(h1.x), f1 = uni(h1.y), b2 = uni(h1.w);
        if ((w0 & 0xFF) > 5) { fail(ERR_VERSION_SUPPORT); return; }
        if (nbytes != d.nbytes || blocksize != d.blocksize || ts == 0 || cbytes < HEADER_LEN) { fail(ERR_INVALID_HEADER); return; }
        if (cbytes > d.destsize) { fail(ERR_READ_BUFFER); return; }
        if ((flags & (FLAG_SHUFFLE | FLAG_BITSHUFFLE)) != (FLAG_SHUFFLE | FLAG_BITSHUFFLE)) { fail(ERR_VERSION_SUPPORT); return; }
        const int special = (int)((b2 >> 28) & 7);
        if (special == SPECIAL_ZERO || special == SPECIAL_UNINIT) { mode = 2; wave_fill_global(out, bsize, 0, wave, 4); return; }
        if (special != 0) { phase_a_special(special, nbytes, blocksize, cbytes, wave); return; }
        if (flags & FLAG_MEMCPYED) {
            if (cbytes != nbytes + HEADER_LEN) { fail(ERR_DATA); return; }
            mode = 1;
            wave_copy_g2g(c + HEADER_LEN + (int64_t)j * blocksize, out, bsize, wave, 4);
            return;
        }
        const int fmt = flags >> 5;
        if (fmt == 4) { fail((flags & FLAG_DONT_SPLIT) || ts <= 1 ? STATUS_ZSTD_PENDING : STATUS_ZSTD_PENDING_SPLIT); return; }   // the zstd read path's (engine.hip)
        if (fmt != 0 && fmt != 1) { fail(ERR_CODEC_SUPPORT); return; }
        filter = (int)((f1 >> 8) & 0xFF);
        if (f0 != 0 || (f1 & 0xFF & ~FILTER_TRUNC_PREC) != 0) { fail(ERR_CODEC_SUPPORT); return; }
        if (filter != FILTER_NONE && filter != FILTER_SHUFFLE && filter != FILTER_BITSHUFFLE) { fail(ERR_CODEC_SUPPORT); return; }
        if (filter == FILTER_BITSHUFFLE && !(flags & FLAG_DONT_SPLIT)) { fail(ERR_CODEC_SUPPORT); return; }
        const bool leftover_blk = bsize != blocksize;
        ns = (!(flags & FLAG_DONT_SPLIT) && !leftover_blk) ? ts : 1;
        neblock = bsize / ns;
        rs = fmt == 0 ? blz_region_stride(neblock) : region_stride(neblock);
        if (ns * rs + 16 > a.lds_bytes) { fail(ERR_FAILURE); return; }
        if (cbytes < HEADER_LEN + 4 * d.nblocks) { fail(ERR_READ_BUFFER); return; }
        const int bstart = ld32s(c + HEADER_LEN + 4 * j);
        if (bstart < HEADER_LEN + 4 * d.nblocks || bstart > cbytes) { fail(ERR_DATA); return; }
        mode = 0;
        int pos = bstart;
        for (int s = 0; s < ns; s++) {
            if (cbytes - pos < 4) { fail(ERR_READ_BUFFER); mode = 3; return; }
            const int cs = ld32s(c + pos);
            pos += 4;
            const int payload = cs > 0 ? cs : (cs < 0 ? 1 : 0);
            if (payload > cbytes - pos) { fail(ERR_READ_BUFFER); mode = 3; return; }
            if ((s & 3) == wave) {
                uint8_t* region = lds + (int64_t)s * rs;                // the decoder's base: offsets inside the region only
                if (cs == 0) {
                    wave_fill_lds(region, 0, neblock, 0);
                } else if (cs < 0) {
                    const int token = c[pos];
                    if (!(token & 1) || cs < -255) { fail(ERR_RUN_LENGTH); }
                    wave_fill_lds(region, 0, neblock, (uint32_t)(-cs) & 0xFF);
                } else if (cs == neblock) {
                    wave_copy_g2l(c + pos, region, 0, neblock);
                } else if (cs > neblock) {
                    fail(ERR_DATA);
                } else {
                    const int park = rs - round16(cs);
                    wave_copy_g2l(c + pos, region, park, cs);
                    const int rc = fmt == 0 ? blosclz_decode_wave(region, 0, neblock, park, cs, rs)
                                            : CIMG_LZ4_DECODE(region, 0, neblock, park, cs, rs);
                    if (rc < 0) fail(rc);
                }
            }
            pos += payload;
        }
    }
};

}  // namespace cimg
