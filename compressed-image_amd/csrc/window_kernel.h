// window_kernel.h -- cimg_decode_window: decode a chosen set of blocks and store only the bytes of a strided 2-D window
// (window_plan.h builds the work items).  One 256-thread workgroup per item (window, batch-wide block): the block is staged
// by DecodeBlock::phase_a (decode_kernel.h) exactly as cimg_decode_blocks stages it, and phase_w then writes, for every
// window row that meets the block, the row's bytes inside the block -- unfiltered straight out of LDS -- to
// out + out_off + r * out_pitch + (column * typesize).  Nothing outside the window is written.  Memcpyed and special chunks
// (zero and uninit: zeros; value and NaN: the pattern at the block's phase, special_plan.h) are cut from the chunk (or from
// nothing) without staging; items of chunks that were decoded whole beforehand
// (zstd, blocks beyond LDS: the batch path into engine scratch) are cut from that copy (`b < 0`).
// cimg_decode_window_strided (below) stages the same way and writes only every col_pitch-th element of each window row.
// cimg_decode_window_grouped runs one workgroup per distinct block and writes every window that meets it.
// cimg_decode_window_typed (at the end) groups the same way and converts each element on its way out of LDS.
#pragma once
#include "decode_kernel.h"

namespace cimg {

struct WindowItem {
    int32_t chunk;        // batch chunk (its status word)
    int32_t b;            // batch-wide block to decode; < 0: copy mode, the chunk lies decoded at whole + src_off
    int32_t r0, r1;       // window rows [r0, r1) that meet the block (or the chunk)
    int64_t p0;           // plane byte offset of the block's (chunk's) first byte
    int64_t len;          // copy mode: bytes of the decoded chunk
    int64_t src_off;      // copy mode: offset of the decoded chunk in `whole`
    int64_t row0;         // plane byte offset of window row 0
    int64_t rpitch;       // plane bytes between the starts of consecutive window rows
    int64_t wbytes;       // bytes of a window row
    int64_t out_off, out_pitch;
};

struct WindowArgs {
    DecodeArgs d;         // descs over the whole batch (raw_off unused), status per chunk, lds_bytes of the launch
    const WindowItem* items;
    const uint8_t* whole; // chunks decoded whole (copy-mode items)
    uint8_t* out;
    int32_t typesize;     // every decoded chunk's header must say this (0: the host has checked the headers)
    int32_t nitems;
};

struct WindowBlock {
    const WindowArgs& a;
    uint8_t* lds;
    WindowItem it;
    DecodeBlock blk;
    int mode = 3;          // 0 staged in LDS, 1 memcpyed chunk, 2 zeros, 3 nothing to write, 4 copy mode, 5 pattern (value / NaN chunk)
    int64_t blen = 0;      // bytes of the block (chunk) the item covers
    const uint8_t* src = nullptr;   // memcpyed / copy mode: the block's first byte; pattern: the chunk's value (null: the NaN)
    int lg = -1;           // log2(typesize) when it is a power of two
    int pts = 1, phase = 0;         // pattern: the typesize, and the element phase of the block's first byte

    CIMG_DEV static WindowItem uniform_item(const WindowItem* p)
    {
        WindowItem t = *p;
        t.chunk = uni(t.chunk); t.b = uni(t.b); t.r0 = uni(t.r0); t.r1 = uni(t.r1);
        t.p0 = uni64(t.p0); t.len = uni64(t.len); t.src_off = uni64(t.src_off); t.row0 = uni64(t.row0);
        t.rpitch = uni64(t.rpitch); t.wbytes = uni64(t.wbytes); t.out_off = uni64(t.out_off); t.out_pitch = uni64(t.out_pitch);
        return t;
    }

    CIMG_DEV WindowBlock(const WindowArgs& a_, uint8_t* lds_, int k)
        : a(a_), lds(lds_), it(uniform_item(a_.items + k)), blk(a_.d, lds_, it.b < 0 ? 0 : it.b) {}
    // (the item handed in, already wave-uniform: the strided kernel keeps its items in a table of its own)
    CIMG_DEV WindowBlock(const WindowArgs& a_, uint8_t* lds_, const WindowItem& t)
        : a(a_), lds(lds_), it(t), blk(a_.d, lds_, it.b < 0 ? 0 : it.b) {}

    CIMG_DEV void fail(int code) { a.d.status[it.chunk] = code; mode = 3; }

    CIMG_DEV void phase_a(int wave)
    {
        mode = 3;
        if (it.b < 0) {
            mode = 4;
            blen = it.len;
            src = a.whole + it.src_off;
            return;
        }
        const ChunkDesc d = uniform_desc(a.d.descs + it.chunk);
        const int j = it.b - d.blk0;
        blen = (j == d.nblocks - 1 && d.leftover) ? d.leftover : d.blocksize;
        const uint8_t* c = a.d.comp + d.comp_off;
        // the header checks of phase_a for the two kinds of chunk it would copy straight to the batch's output
        const u128 h0 = ld128u(c), h1 = ld128u(c + 16);
        const uint32_t w0 = uni(h0.x);
        const int flags = (int)((w0 >> 16) & 0xFF), ts = (int)(w0 >> 24);
        const int nbytes = (int)uni(h0.y), blocksize = (int)uni(h0.z), cbytes = (int)uni(h0.w);
        const uint32_t b2 = uni(h1.w);
        if ((w0 & 0xFF) > 5) { fail(ERR_VERSION_SUPPORT); return; }
        if (nbytes != d.nbytes || blocksize != d.blocksize || (a.typesize && ts != a.typesize) || cbytes < HEADER_LEN) { fail(ERR_INVALID_HEADER); return; }
        if (cbytes > d.destsize) { fail(ERR_READ_BUFFER); return; }
        if ((flags & (FLAG_SHUFFLE | FLAG_BITSHUFFLE)) != (FLAG_SHUFFLE | FLAG_BITSHUFFLE)) { fail(ERR_VERSION_SUPPORT); return; }
        const int special = (int)((b2 >> 28) & 7);
        if (special == SPECIAL_ZERO || special == SPECIAL_UNINIT) { mode = 2; return; }
        if (special != 0) {
            const int rc = special_check(special, ts, nbytes, cbytes);
            if (rc < 0) { fail(rc); return; }
            mode = 5;
            src = special == SPECIAL_VALUE ? c + HEADER_LEN : nullptr;
            pts = ts;
            phase = special_phase(j, blocksize, ts);
            if ((ts & (ts - 1)) == 0) lg = __builtin_ctz((unsigned)ts);
            return;
        }
        if (flags & FLAG_MEMCPYED) {
            if (cbytes != nbytes + HEADER_LEN) { fail(ERR_DATA); return; }
            mode = 1;
            src = c + HEADER_LEN + (int64_t)j * blocksize;
            return;
        }
        blk.phase_a<false>(wave);
        mode = blk.mode == 0 ? 0 : 3;
        if (mode == 0 && (blk.ts & (blk.ts - 1)) == 0) lg = __builtin_ctz((unsigned)blk.ts);
    }

    // unfiltered byte k of the staged block (the inverse filters of DecodeBlock::phase_b, one byte at a time)
    CIMG_DEV uint8_t staged(int k) const
    {
        const int ts = blk.ts;
        if (blk.filter == FILTER_BITSHUFFLE) {
            const int ne8 = (blk.bsize / ts) & ~7, rowbytes = ne8 >> 3;
            if (k >= ne8 * ts) return lds[k];
            const int e = lg >= 0 ? k >> lg : k / ts, jb = lg >= 0 ? k & (ts - 1) : k % ts;
            const int g = e >> 3, i = e & 7;
            uint32_t v = 0;
            for (int bit = 0; bit < 8; bit++) v |= (uint32_t)((lds[(8 * jb + bit) * rowbytes + g] >> i) & 1) << bit;
            return (uint8_t)v;
        }
        if (blk.filter == FILTER_NONE || ts == 1) return lds[blk.ns > 1 ? (k / blk.neblock) * blk.rs + k % blk.neblock : k];
        const int ne = blk.bsize / ts;
        if (k >= ne * ts) return lds[k];
        return lg >= 0 ? lds[blk.plane_base(k & (ts - 1)) + (k >> lg)] : lds[blk.plane_base(k % ts) + k / ts];
    }

    CIMG_DEV uint8_t byte_at(int64_t k) const
    {
        if (mode == 0) return staged((int)k);
        if (mode == 2) return 0;
        if (mode == 5) {
            const int idx = lg >= 0 ? (phase + (int)k) & (pts - 1) : (phase + (int)k) % pts;
            return (uint8_t)SpecialPattern{src, pts}.at(idx);
        }
        return src[k];
    }

    CIMG_DEV void phase_w(int wave)
    {
        if (mode == 3) return;
        const int tid0 = wave * 64;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rs = it.row0 + (int64_t)r * it.rpitch, re = rs + it.wbytes;
            const int64_t s = rs > it.p0 ? rs : it.p0;
            const int64_t e = re < it.p0 + blen ? re : it.p0 + blen;
            if (s >= e) continue;
            uint8_t* dst = a.out + it.out_off + (int64_t)r * it.out_pitch + (s - rs);
            const int64_t n = e - s, k0 = s - it.p0;
            // 4-byte units aligned on the destination: whole units are one dword store, the ragged ends go byte by byte
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += 256) {
                FOR_LANES(l) {
                    const int64_t u = u0 + l;
                    if (u < units) {
                        const int64_t q0 = 4 * u - mis;
                        if (q0 >= 0 && q0 + 4 <= n) {
                            const uint32_t v = (uint32_t)byte_at(k0 + q0) | ((uint32_t)byte_at(k0 + q0 + 1) << 8) |
                                               ((uint32_t)byte_at(k0 + q0 + 2) << 16) | ((uint32_t)byte_at(k0 + q0 + 3) << 24);
                            *reinterpret_cast<uint32_t*>(dst + q0) = v;
                        } else {
                            for (int i = 0; i < 4; i++) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) dst[q] = byte_at(k0 + q);
                            }
                        }
                    }
                }
            }
        }
    }
};

// ---- strided windows: cimg_decode_window_strided -----------------------------------------------------------------------------
// A window whose rows take every col_pitch-th element of the plane.  The block is staged exactly as above (WindowBlock::phase_a);
// only the write phase differs: output byte q of a row is byte q % typesize of element q / typesize, which lies cpitch bytes after
// its neighbour in the plane.  An element that straddles two blocks belongs, byte by byte, to both items.
struct StridedWindowItem : WindowItem {     // wbytes: bytes of an OUTPUT row (width * typesize)
    int64_t cpitch;       // plane bytes between consecutive elements of a window row (col_pitch * typesize)
    int32_t ts;           // the plane's typesize (validated by the planner)
    int32_t pad_;
};

struct StridedWindowArgs {
    WindowArgs w;         // (w.items unused)
    const StridedWindowItem* items;
};

struct StridedWindowBlock {
    WindowBlock wb;
    int64_t cpitch;
    int ts;
    int lg;               // log2(ts) when it is a power of two, else -1

    CIMG_DEV StridedWindowBlock(const StridedWindowArgs& a, uint8_t* lds, int k)
        : wb(a.w, lds, WindowBlock::uniform_item(a.items + k)), cpitch(uni64(a.items[k].cpitch)), ts(uni(a.items[k].ts))
    {
        lg = (ts & (ts - 1)) == 0 ? __builtin_ctz((unsigned)ts) : -1;
    }

    CIMG_DEV void phase_a(int wave) { wb.phase_a(wave); }

    CIMG_DEV void phase_w(int wave)
    {
        if (wb.mode == 3) return;
        const WindowItem& it = wb.it;
        const int64_t blen = wb.blen, width = it.wbytes / ts;
        const int tid0 = wave * 64;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the block
            // elements c_lo .. c_hi of the row have a byte in [0, blen)
            const int64_t lo = -rel - (ts - 1), hi = blen - 1 - rel;
            if (hi < 0) continue;
            const int64_t c_lo = lo <= 0 ? 0 : (lo + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            const int64_t base = rel + c_lo * cpitch;                          // block offset of element c_lo (>= -(ts - 1))
            uint8_t* dst = wb.a.out + it.out_off + (int64_t)r * it.out_pitch + c_lo * ts;
            const int64_t n = (c_hi + 1 - c_lo) * ts;                          // (< 2^32: at most blen / ts + 2 elements)
            // 4-byte units aligned on the destination, as in WindowBlock::phase_w
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += 256) {
                FOR_LANES(l) {
                    const int64_t u = u0 + l;
                    if (u < units) {
                        const int64_t q0 = 4 * u - mis;
                        int64_t k[4];
                        bool all = true;
                        for (int i = 0; i < 4; i++) {
                            const int64_t q = q0 + i;
                            k[i] = -1;
                            if (q >= 0 && q < n) {
                                const uint32_t e = lg >= 0 ? (uint32_t)q >> lg : (uint32_t)q / (uint32_t)ts;
                                const int64_t at = base + (int64_t)e * cpitch + (int64_t)((uint32_t)q - e * (uint32_t)ts);
                                if (at >= 0 && at < blen) k[i] = at;
                            }
                            all = all && k[i] >= 0;
                        }
                        if (all) {
                            const uint32_t v = (uint32_t)wb.byte_at(k[0]) | ((uint32_t)wb.byte_at(k[1]) << 8) |
                                               ((uint32_t)wb.byte_at(k[2]) << 16) | ((uint32_t)wb.byte_at(k[3]) << 24);
                            *reinterpret_cast<uint32_t*>(dst + q0) = v;
                        } else {
                            for (int i = 0; i < 4; i++)
                                if (k[i] >= 0) dst[q0 + i] = wb.byte_at(k[i]);
                        }
                    }
                }
            }
        }
    }
};

// ---- grouped windows: cimg_decode_window_grouped ------------------------------------------------------------------------------
// One workgroup per UNIT: a block with every item that meets it (window_plan.h: group_items), so a block shared by many windows is
// staged once.  The unit's first item stages the block (WindowBlock::phase_a, unchanged); after the barrier every item is written
// with the strided write phase, which only reads LDS -- no barrier between items.  A unit of one item is written by all 256
// threads, as cimg_decode_window_strided writes it; a unit of more deals its items round-robin over the four waves, each wave
// writing its item alone with 64 lanes.  A copy-mode item (b < 0) is a unit of its own.
struct WindowUnit {
    int32_t item0, nitems;     // items [item0, item0 + nitems) of the table, in window order
};

struct GroupedWindowArgs {
    WindowArgs w;              // (w.items unused; w.nitems: items of the table)
    const StridedWindowItem* items;
    const WindowUnit* units;
    int32_t nunits;
};

struct GroupedWindowBlock {
    const GroupedWindowArgs& a;
    WindowUnit u;
    WindowBlock wb;            // the staged block, through the unit's first item

    CIMG_DEV static WindowUnit uniform_unit(const WindowUnit* p)
    {
        WindowUnit t = *p;
        t.item0 = uni(t.item0); t.nitems = uni(t.nitems);
        return t;
    }

    CIMG_DEV GroupedWindowBlock(const GroupedWindowArgs& a_, uint8_t* lds, int k)
        : a(a_), u(uniform_unit(a_.units + k)), wb(a_.w, lds, WindowBlock::uniform_item(a_.items + u.item0)) {}

    CIMG_DEV void phase_a(int wave) { wb.phase_a(wave); }

    // StridedWindowBlock::phase_w for item k of the table over the staged block, by threads tid0 + lane, + stride, ...
    // (p0 is the item's own: windows of two planes that share the chunk see the block at different plane offsets)
    CIMG_DEV void write_item(int k, int tid0, int stride)
    {
        const WindowItem it = WindowBlock::uniform_item(a.items + k);
        const int64_t cpitch = uni64(a.items[k].cpitch);
        const int ts = uni(a.items[k].ts);
        const int lg = (ts & (ts - 1)) == 0 ? __builtin_ctz((unsigned)ts) : -1;
        const int64_t blen = wb.blen, width = it.wbytes / ts;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the block
            // elements c_lo .. c_hi of the row have a byte in [0, blen)
            const int64_t lo = -rel - (ts - 1), hi = blen - 1 - rel;
            if (hi < 0) continue;
            const int64_t c_lo = lo <= 0 ? 0 : (lo + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            const int64_t base = rel + c_lo * cpitch;                          // block offset of element c_lo (>= -(ts - 1))
            uint8_t* dst = a.w.out + it.out_off + (int64_t)r * it.out_pitch + c_lo * ts;
            const int64_t n = (c_hi + 1 - c_lo) * ts;                          // (< 2^32: at most blen / ts + 2 elements)
            // 4-byte units aligned on the destination, as in WindowBlock::phase_w
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += stride) {
                FOR_LANES(l) {
                    const int64_t un = u0 + l;
                    if (un < units) {
                        const int64_t q0 = 4 * un - mis;
                        int64_t at[4];
                        bool all = true;
                        for (int i = 0; i < 4; i++) {
                            const int64_t q = q0 + i;
                            at[i] = -1;
                            if (q >= 0 && q < n) {
                                const uint32_t e = lg >= 0 ? (uint32_t)q >> lg : (uint32_t)q / (uint32_t)ts;
                                const int64_t p = base + (int64_t)e * cpitch + (int64_t)((uint32_t)q - e * (uint32_t)ts);
                                if (p >= 0 && p < blen) at[i] = p;
                            }
                            all = all && at[i] >= 0;
                        }
                        if (all) {
                            const uint32_t v = (uint32_t)wb.byte_at(at[0]) | ((uint32_t)wb.byte_at(at[1]) << 8) |
                                               ((uint32_t)wb.byte_at(at[2]) << 16) | ((uint32_t)wb.byte_at(at[3]) << 24);
                            *reinterpret_cast<uint32_t*>(dst + q0) = v;
                        } else {
                            for (int i = 0; i < 4; i++)
                                if (at[i] >= 0) dst[q0 + i] = wb.byte_at(at[i]);
                        }
                    }
                }
            }
        }
    }

    CIMG_DEV void phase_w(int wave)
    {
        if (wb.mode == 3) return;                                              // (the block failed to stage: nothing for any item)
        if (u.nitems == 1) { write_item(u.item0, wave * 64, 256); return; }
        for (int k = wave; k < u.nitems; k += 4) write_item(u.item0 + k, 0, 64);
    }
};

// ---- typed windows: cimg_decode_window_typed ----------------------------------------------------------------------------------
// The grouped launch with a write phase of its own: the work unit is one output ELEMENT.  A thread gathers the ts bytes of a
// sampled element (WindowBlock::byte_at, every mode), converts the value -- x = (float)v, y = fl32(fl32(x * scale) + offset), two
// roundings and never an FMA, then y itself or y rounded once to float16 -- and stores it with one store of the output's size at
// out + out_off + r * out_pitch + c * epitch.  Bytes between the elements of a row are not written, so the windows of C planes can
// fill the channel slots of pixel-major rows (epitch = C * size of the output type).  An item whose output type is its stored type
// with scale 1 and offset 0 copies the element's bytes unchanged.  The planner (window_plan.h: plan_windows over TypedWindowSpec)
// admits only planes whose blocks hold whole elements, and only naturally aligned outputs.
enum : int { T_U8 = 0, T_I8 = 1, T_U16 = 2, T_I16 = 3, T_U32 = 4, T_I32 = 5, T_F16 = 6, T_F32 = 7, T_F64 = 8, T_COUNT = 9 };   // = CIMG_T_*

CIMG_HD int type_size(int t) { return t < 0 || t >= T_COUNT ? 0 : t < T_U16 ? 1 : t < T_U32 || t == T_F16 ? 2 : t == T_F64 ? 8 : 4; }

struct TypedWindowItem : StridedWindowItem {
    int64_t epitch;       // output bytes between consecutive elements of a row
    int32_t src_type, out_type;     // T_*
    float scale, offset;
};

struct TypedWindowArgs {
    WindowArgs w;              // (w.items unused; w.nitems: items of the table)
    const TypedWindowItem* items;
    const WindowUnit* units;
    int32_t nunits;
};

CIMG_HD uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
CIMG_HD float bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

#ifdef CIMG_EMULATE
// float16 <-> float32 in integer arithmetic (the host compiler need not know a half type): exact one way, round to nearest even
// the other, subnormals kept, overflow to inf
inline float half_to_f32(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u;
    uint32_t m = h & 0x3FFu;
    if (e == 31) return bits_f32(s | 0x7F800000u | (m << 13));
    if (e) return bits_f32(s | ((e + 112) << 23) | (m << 13));
    if (!m) return bits_f32(s);
    const int sh = __builtin_clz(m) - 21;                     // the top bit of m goes to bit 10
    m = (m << sh) & 0x3FFu;
    return bits_f32(s | ((uint32_t)(113 - sh) << 23) | (m << 13));
}
inline uint16_t f32_to_half(float f)
{
    const uint32_t u = f32_bits(f), s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(s | 0x7E00u);      // NaN
    if (a >= 0x477FF000u) return (uint16_t)(s | 0x7C00u);     // >= 65520: inf
    if (a >= 0x38800000u) {                                   // a normal half
        const uint32_t m = a - 0x38000000u, rem = m & 0x1FFFu;
        uint32_t r = m >> 13;
        if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) r++;
        return (uint16_t)(s | r);
    }
    if (a <= 0x33000000u) return (uint16_t)s;                 // <= 2^-25: zero (the tie goes to even)
    const int shift = 126 - (int)(a >> 23);                   // 14 .. 24: units of 2^-24
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    uint32_t r = m >> shift;
    if (rem > half || (rem == half && (r & 1))) r++;
    return (uint16_t)(s | r);
}
#else
CIMG_DEV float half_to_f32(uint16_t h) { _Float16 x; __builtin_memcpy(&x, &h, 2); return (float)x; }
CIMG_DEV uint16_t f32_to_half(float f) { const _Float16 x = (_Float16)f; uint16_t h; __builtin_memcpy(&h, &x, 2); return h; }
#endif

// the stored element `bits` (its ts low bytes) as float32: exact for 8 / 16-bit integers and float16, one rounding for the rest
CIMG_DEV float typed_load(uint64_t bits, int src_type)
{
    switch (src_type) {
    case T_U8: case T_U16: case T_U32: return (float)(uint32_t)bits;
    case T_I8: return (float)(int8_t)bits;
    case T_I16: return (float)(int16_t)bits;
    case T_I32: return (float)(int32_t)bits;
    case T_F16: return half_to_f32((uint16_t)bits);
    case T_F32: return bits_f32((uint32_t)bits);
    default: { double d; __builtin_memcpy(&d, &bits, 8); return (float)d; }
    }
}

// fl32(fl32(x * scale) + offset): the product is rounded before the sum -- no contraction to an FMA here, whatever the build's
// default says (the emulator's translation unit is built with -ffp-contract=off)
CIMG_DEV float typed_scale(float x, float scale, float offset)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = x * scale;
    return p + offset;
}

// ---- the way back (typed window WRITES: update_kernel.h, TypedPatchBlock) ---------------------------------------------------------
// fl32(fl32(y - offset) / scale), the inverse of typed_scale with the same pair: the difference is rounded before the quotient, and
// the quotient is the IEEE correctly rounded division -- not a multiply by a reciprocal, not a fast divide (the product is built
// without fast-math, and HIP's default keeps fp32 division correctly rounded, denormals included)
CIMG_DEV float typed_unscale(float y, float scale, float offset)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = y - offset;
    return d / scale;
}

// the element at m, of memory type mem_type (T_F32 or T_F16), as float32: exact
CIMG_DEV float typed_load_mem(const uint8_t* m, int mem_type)
{
    if (mem_type == T_F16) return half_to_f32(*reinterpret_cast<const uint16_t*>(m));
    return bits_f32(*reinterpret_cast<const uint32_t*>(m));
}

// t as a stored element of dst_type (its low bytes).  Integers: NaN gives 0, otherwise rint (ties to even) saturated to the type's
// range -- the bounds are compared in float32, where 2^31 and 2^32 are exact and every integer-valued float below them converts
// exactly.  float16: one rounding to nearest even, overflow to inf, subnormals kept.  float32: t itself.
CIMG_DEV uint32_t typed_store_bits(float t, int dst_type)
{
    if (dst_type == T_F32) return f32_bits(t);
    if (dst_type == T_F16) return f32_to_half(t);
    if (t != t) return 0;
    const float r = __builtin_rintf(t);
    switch (dst_type) {
    case T_U8: return r <= 0.0f ? 0u : r >= 255.0f ? 255u : (uint32_t)r;
    case T_I8: return (uint32_t)(uint8_t)(int8_t)(r <= -128.0f ? -128 : r >= 127.0f ? 127 : (int32_t)r);
    case T_U16: return r <= 0.0f ? 0u : r >= 65535.0f ? 65535u : (uint32_t)r;
    case T_I16: return (uint32_t)(uint16_t)(int16_t)(r <= -32768.0f ? -32768 : r >= 32767.0f ? 32767 : (int32_t)r);
    case T_U32: return r <= 0.0f ? 0u : r >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)r;
    default: return r <= -2147483648.0f ? 0x80000000u : r >= 2147483648.0f ? 0x7FFFFFFFu : (uint32_t)(int32_t)r;   // T_I32
    }
}

struct TypedWindowBlock {
    const TypedWindowArgs& a;
    WindowUnit u;
    WindowBlock wb;            // the staged block, through the unit's first item

    CIMG_DEV TypedWindowBlock(const TypedWindowArgs& a_, uint8_t* lds, int k)
        : a(a_), u(GroupedWindowBlock::uniform_unit(a_.units + k)), wb(a_.w, lds, WindowBlock::uniform_item(a_.items + u.item0)) {}

    CIMG_DEV void phase_a(int wave) { wb.phase_a(wave); }

    // item k of the table over the staged block, by threads tid0 + lane, + stride, ...: one element a thread
    CIMG_DEV void write_item(int k, int tid0, int stride)
    {
        const WindowItem it = WindowBlock::uniform_item(a.items + k);
        const int64_t cpitch = uni64(a.items[k].cpitch), epitch = uni64(a.items[k].epitch);
        const int ts = uni(a.items[k].ts), src_type = uni(a.items[k].src_type), out_type = uni(a.items[k].out_type);
        const float scale = bits_f32(uni(f32_bits(a.items[k].scale))), offset = bits_f32(uni(f32_bits(a.items[k].offset)));
        const bool identity = out_type == src_type && scale == 1.0f && offset == 0.0f;
        const int osz = identity ? ts : type_size(out_type);
        const int64_t blen = wb.blen, width = it.wbytes / ts;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the block
            // elements c_lo .. c_hi of the row lie inside [0, blen) (whole: the planner admits no element over a block's edge)
            const int64_t hi = blen - ts - rel;
            if (hi < 0) continue;
            const int64_t c_lo = rel >= 0 ? 0 : (-rel + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            const int64_t base = rel + c_lo * cpitch;                          // block offset of element c_lo (>= 0)
            uint8_t* dst = a.w.out + it.out_off + (int64_t)r * it.out_pitch + c_lo * epitch;
            const int64_t n = c_hi + 1 - c_lo;                                 // (< 2^31: at most blen / ts elements)
            for (int64_t e0 = tid0; e0 < n; e0 += stride) {
                FOR_LANES(l) {
                    const int64_t e = e0 + l;
                    if (e < n) {
                        const int64_t at = base + e * cpitch;
                        uint64_t v = 0;
                        for (int j = 0; j < ts; j++) v |= (uint64_t)wb.byte_at(at + j) << (8 * j);
                        if (!identity) {
                            const float y = typed_scale(typed_load(v, src_type), scale, offset);
                            v = out_type == T_F16 ? (uint64_t)f32_to_half(y) : (uint64_t)f32_bits(y);
                        }
                        uint8_t* q = dst + e * epitch;
                        if (osz == 1) *q = (uint8_t)v;
                        else if (osz == 2) *reinterpret_cast<uint16_t*>(q) = (uint16_t)v;
                        else if (osz == 4) *reinterpret_cast<uint32_t*>(q) = (uint32_t)v;
                        else *reinterpret_cast<uint64_t*>(q) = v;
                    }
                }
            }
        }
    }

    CIMG_DEV void phase_w(int wave)
    {
        if (wb.mode == 3) return;                                              // (the block failed to stage: nothing for any item)
        if (u.nitems == 1) { write_item(u.item0, wave * 64, 256); return; }
        for (int k = wave; k < u.nitems; k += 4) write_item(u.item0 + k, 0, 64);
    }
};

}  // namespace cimg
