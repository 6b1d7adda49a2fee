// update_kernel.h -- window writes (update_plan.h plans them): the kernels that turn old chunks plus window bytes into the chunks a
// from-scratch compress of the edited pixels gives.
//
//   cimg_update_patch   one 256-thread workgroup per unit.  A unit is one block of a spliced chunk -- staged by
//                       DecodeBlock::phase_a through WindowBlock exactly as cimg_decode_window stages it, written UNFILTERED to its
//                       slot of the patch buffer -- or one chunk the batch path decoded whole.  Then the window rows that meet the
//                       unit are copied over it from the source, one window after the other in call order (a later window wins).  A
//                       block the windows cover completely is not staged: only the source bytes are copied.
//   cimg_update_patch_strided
//                       the same for windows with a col_pitch (StridedPatchBlock, below): same staging, its own overlay and schedule.
//   cimg_update_patch_typed
//                       the same for typed windows (TypedPatchBlock, below): every written element is loaded as float32 / float16,
//                       unscaled, rounded and stored as the plane's type on its way into the unit.
//   cimg_update_patch_masked
//                       the same for masked and constant windows (MaskedPatchBlock, below): an element is written only where the
//                       window's mask byte is not 0, and a constant window writes one value and reads no source.
//   cimg_update_layout  one wave per spliced chunk.  Lane j takes block j: a touched block's size comes from the stream records the
//                       encode launch left for it; an untouched block's streams are harvested from the old chunk (a negative csize
//                       word is a run, csize == neblock raw, anything else a coded stream whose payload stays where it is).  A wave
//                       prefix sum gives the new bstarts; blosc2's running-destsize rule, special-zero and the header are re-applied
//                       as LayoutChunk applies them.  A chunk that would not fit, or whose running total enters the clipped regime
//                       at a harvested coded stream (its LZ4 `need` is not known), is handed back to the whole route.
//   cimg_update_emit    one 256-thread workgroup per block of a spliced chunk: an untouched block is one contiguous copy from the old
//                       chunk (its csize words and payloads are the bytes a fresh encode writes); a touched block gets its csize
//                       words and payloads from the encode launch's scratch slot, as EmitBlock writes them.
//
// Why splicing is exact: a stream's bytes depend only on the stream, never on the capacity left in the chunk; a clipped budget can only
// turn "coded" into "does not fit", which makes the whole chunk memcpyed.  So old streams of untouched blocks are what a fresh encode
// would write, and only the chunk-level rules need re-applying.
#pragma once
#include "window_kernel.h"
#include "assemble_kernel.h"

namespace cimg {

// ---- patch ----------------------------------------------------------------------------------------------------------------------
struct PatchUnit {
    int32_t chunk;        // batch chunk (its status word)
    int32_t stage;        // 1: stage the block first (WindowArgs::items[k] names it); 0: the unit's bytes are there already, or
                          //    every byte of it comes from the windows
    int32_t item0, nitems;// overlays of the unit: PatchArgs::items[item0 .. item0 + nitems), in call order (an item's p0 is the
                          //    unit's first byte in that item's plane)
    int64_t len;          // bytes of the unit
    int64_t dst_off;      // the unit's bytes in PatchArgs::dst
};

struct PatchArgs {
    WindowArgs w;            // w.d: descs over the batch, status per chunk, lds_bytes; w.items[k]: chunk and block of unit k
    const PatchUnit* units;
    const WindowItem* items; // overlays: rows r0 .. r1 of a window (out_off / out_pitch locate the SOURCE rows)
    const uint8_t* src;      // the windows' bytes
    uint8_t* dst;            // patch buffer
    int32_t nunits;
};

struct PatchBlock {
    const PatchArgs& a;
    PatchUnit u;
    WindowBlock wb;

    CIMG_DEV static PatchUnit uniform_unit(const PatchUnit* p)
    {
        PatchUnit t = *p;
        t.chunk = uni(t.chunk); t.stage = uni(t.stage); t.item0 = uni(t.item0); t.nitems = uni(t.nitems);
        t.len = uni64(t.len); t.dst_off = uni64(t.dst_off);
        return t;
    }

    CIMG_DEV PatchBlock(const PatchArgs& a_, uint8_t* lds, int k) : a(a_), u(uniform_unit(a_.units + k)), wb(a_.w, lds, k) {}
    // (the unit handed in, already wave-uniform: the strided kernel keeps its units in a table of its own)
    CIMG_DEV PatchBlock(const PatchArgs& a_, uint8_t* lds, int k, const PatchUnit& t) : a(a_), u(t), wb(a_.w, lds, k) {}

    CIMG_DEV void phase_a(int wave) { if (u.stage) wb.phase_a(wave); }

    // the staged block, unfiltered, into its slot (a block that failed to stage has its status word set and is left alone)
    CIMG_DEV void phase_base(int wave)
    {
        if (!u.stage || wb.mode == 3) return;
        uint8_t* dst = a.dst + u.dst_off;
        const int64_t units = u.len >> 2;
        for (int64_t u0 = wave * 64; u0 < units; u0 += 256) {
            FOR_LANES(l) {
                const int64_t q = u0 + l;
                if (q < units) {
                    const int64_t k = 4 * q;
                    const uint32_t v = (uint32_t)wb.byte_at(k) | ((uint32_t)wb.byte_at(k + 1) << 8) |
                                       ((uint32_t)wb.byte_at(k + 2) << 16) | ((uint32_t)wb.byte_at(k + 3) << 24);
                    *reinterpret_cast<uint32_t*>(dst + k) = v;
                }
            }
        }
        if (wave == 0) {
            FOR_LANES(l) { const int64_t k = 4 * units + l; if (k < u.len) dst[k] = wb.byte_at(k); }
        }
    }

    // overlay k of the unit: the rows of one window that meet it
    // (StridedPatchBlock::overlay below keeps a copy of this row loop with tid0 and the stride as parameters: change them together)
    CIMG_DEV void overlay(int wave, int k)
    {
        const WindowItem it = WindowBlock::uniform_item(a.items + u.item0 + k);
        const int tid0 = wave * 64;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rs = it.row0 + (int64_t)r * it.rpitch, re = rs + it.wbytes;
            const int64_t s = rs > it.p0 ? rs : it.p0;
            const int64_t e = re < it.p0 + u.len ? re : it.p0 + u.len;
            if (s >= e) continue;
            const uint8_t* src = a.src + it.out_off + (int64_t)r * it.out_pitch + (s - rs);
            uint8_t* dst = a.dst + u.dst_off + (s - it.p0);
            const int64_t n = e - s;
            // 4-byte units aligned on the destination: whole units are one dword store, the ragged ends go byte by byte
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += 256) {
                FOR_LANES(l) {
                    const int64_t q0 = 4 * (u0 + l) - mis;
                    if (u0 + l < units) {
                        if (q0 >= 0 && q0 + 4 <= n) {
                            const uint32_t v = (uint32_t)src[q0] | ((uint32_t)src[q0 + 1] << 8) | ((uint32_t)src[q0 + 2] << 16) |
                                               ((uint32_t)src[q0 + 3] << 24);
                            *reinterpret_cast<uint32_t*>(dst + q0) = v;
                        } else {
                            for (int i = 0; i < 4; i++) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) dst[q] = src[q];
                            }
                        }
                    }
                }
            }
        }
    }
};

// ---- strided patch: cimg_update_patch_strided -------------------------------------------------------------------------------------
// The patch kernel of the strided write calls.  Units are staged exactly as above (PatchBlock::phase_a and phase_base, every
// staging mode theirs); only the overlay differs: element c of window row r goes to plane byte row0 + r * rpitch + c * cpitch.  For
// every row that meets the unit only the elements with a byte inside it are visited (c_lo .. c_hi, from the unit's place in the
// plane), one lane an element, so the work follows the samples in the unit and not the row's width.  An element that straddles the
// unit's end is written byte by byte by the units that hold its bytes.  Items with cpitch == typesize are dense rows and are copied in
// dword units as PatchBlock::overlay copies them.  The host decides each unit's schedule (update_plan.h: items_disjoint): ordered,
// item after item with a barrier between (a later window wins); or disjoint, the items dealt round-robin over the four waves, each
// writing its item alone with 64 lanes and no barrier, as cimg_decode_window_grouped reads.
struct StridedPatchUnit {
    PatchUnit u;
    int32_t disjoint;     // 1: no two items of the unit write a common byte
    int32_t pad_;
};

struct StridedPatchArgs {
    PatchArgs p;                      // (p.units and p.items unused)
    const StridedPatchUnit* units;
    const StridedWindowItem* items;   // overlays, in call order inside a unit
};

struct StridedPatchBlock {
    const StridedPatchArgs& a;
    PatchBlock pb;
    int disjoint;

    CIMG_DEV StridedPatchBlock(const StridedPatchArgs& a_, uint8_t* lds, int k)
        : a(a_), pb(a_.p, lds, k, PatchBlock::uniform_unit(&a_.units[k].u)), disjoint(uni(a_.units[k].disjoint)) {}

    // overlay k of the unit by threads tid0 + lane, + stride, ...
    CIMG_DEV void overlay(int k, int tid0, int stride)
    {
        const StridedWindowItem* ip = a.items + pb.u.item0 + k;
        const WindowItem it = WindowBlock::uniform_item(ip);
        const int64_t cpitch = uni64(ip->cpitch);
        const int ts = uni(ip->ts);
        const int64_t len = pb.u.len;
        uint8_t* const unit = a.p.dst + pb.u.dst_off;
        // dense rows: a copy of PatchBlock::overlay's row loop with tid0 and the stride as parameters (that kernel must not change
        // here; keep the two in step by hand until both can share one helper)
        if (cpitch == ts) {
            for (int r = it.r0; r < it.r1; r++) {
                const int64_t rs = it.row0 + (int64_t)r * it.rpitch, re = rs + it.wbytes;
                const int64_t s = rs > it.p0 ? rs : it.p0;
                const int64_t e = re < it.p0 + len ? re : it.p0 + len;
                if (s >= e) continue;
                const uint8_t* src = a.p.src + it.out_off + (int64_t)r * it.out_pitch + (s - rs);
                uint8_t* dst = unit + (s - it.p0);
                const int64_t n = e - s;
                const int64_t mis = (int64_t)((uintptr_t)dst & 3);
                const int64_t units = (mis + n + 3) >> 2;
                for (int64_t u0 = tid0; u0 < units; u0 += stride) {
                    FOR_LANES(l) {
                        const int64_t q0 = 4 * (u0 + l) - mis;
                        if (u0 + l < units) {
                            if (q0 >= 0 && q0 + 4 <= n) {
                                const uint32_t v = (uint32_t)src[q0] | ((uint32_t)src[q0 + 1] << 8) | ((uint32_t)src[q0 + 2] << 16) |
                                                   ((uint32_t)src[q0 + 3] << 24);
                                *reinterpret_cast<uint32_t*>(dst + q0) = v;
                            } else {
                                for (int i = 0; i < 4; i++) {
                                    const int64_t q = q0 + i;
                                    if (q >= 0 && q < n) dst[q] = src[q];
                                }
                            }
                        }
                    }
                }
            }
            return;
        }
        const int64_t width = it.wbytes / ts;
        const bool dwords = ts == 4 || ts == 8;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the unit
            // elements c_lo .. c_hi of the row have a byte in [0, len)
            const int64_t lo = -rel - (ts - 1), hi = len - 1 - rel;
            if (hi < 0) continue;
            const int64_t c_lo = lo <= 0 ? 0 : (lo + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            const int64_t base = rel + c_lo * cpitch;                          // unit offset of element c_lo (>= -(ts - 1))
            const uint8_t* src = a.p.src + it.out_off + (int64_t)r * it.out_pitch + c_lo * ts;
            const int64_t ne = c_hi + 1 - c_lo;
            for (int64_t e0 = tid0; e0 < ne; e0 += stride) {
                FOR_LANES(l) {
                    const int64_t e = e0 + l;
                    if (e < ne) {
                        const int64_t at = base + e * cpitch;                  // the element's bytes: [at, at + ts) of the unit
                        const uint8_t* s = src + e * ts;
                        uint8_t* d = unit + at;
                        if (dwords && at >= 0 && at + ts <= len && ((uintptr_t)d & 3) == 0) {
                            for (int i = 0; i < ts; i += 4) {
                                const uint32_t v = (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16) |
                                                   ((uint32_t)s[i + 3] << 24);
                                *reinterpret_cast<uint32_t*>(d + i) = v;
                            }
                        } else {
                            for (int i = 0; i < ts; i++)
                                if (at + i >= 0 && at + i < len) d[i] = s[i];
                        }
                    }
                }
            }
        }
    }
};

// ---- typed patch: cimg_update_patch_typed -----------------------------------------------------------------------------------------
// The patch kernel of the typed write call, the inverse of cimg_decode_window_typed.  Units, staging and the two schedules are those
// of the strided patch kernel; the overlay always walks elements, one lane an element: element c of window row r is loaded from
// src + out_off + r * out_pitch + c * epitch as out_type (one naturally aligned load), converted -- typed_unscale, then
// typed_store_bits for the plane's src_type -- and stored at plane byte row0 + r * rpitch + c * cpitch.  An item whose out_type is
// its src_type with scale 1 and offset 0 copies the element's bytes unchanged.  The planner admits only planes whose blocks hold
// whole elements of 1, 2, 4 or 8 bytes, and units start on multiples of 64 in their buffers: every element lies inside one unit
// and its store is one aligned store of its size -- there is no byte-wise tail here.  Identity items with dense rows on both sides
// (epitch == cpitch == typesize) are copied in dword units.
struct TypedPatchArgs {
    PatchArgs p;                      // (p.units and p.items unused)
    const StridedPatchUnit* units;
    const TypedWindowItem* items;     // overlays, in call order inside a unit (out_off / out_pitch / epitch locate the SOURCE elements)
};

struct TypedPatchBlock {
    const TypedPatchArgs& a;
    PatchBlock pb;
    int disjoint;

    CIMG_DEV TypedPatchBlock(const TypedPatchArgs& a_, uint8_t* lds, int k)
        : a(a_), pb(a_.p, lds, k, PatchBlock::uniform_unit(&a_.units[k].u)), disjoint(uni(a_.units[k].disjoint)) {}

    // rows r0 .. r1 of a dense item, copied unchanged in dword units aligned on the destination (the row loop of PatchBlock::overlay
    // with tid0 and the stride as parameters)
    CIMG_DEV void dense_rows(const WindowItem& it, int tid0, int stride)
    {
        const int64_t len = pb.u.len;
        uint8_t* const unit = a.p.dst + pb.u.dst_off;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rs = it.row0 + (int64_t)r * it.rpitch, re = rs + it.wbytes;
            const int64_t s = rs > it.p0 ? rs : it.p0;
            const int64_t e = re < it.p0 + len ? re : it.p0 + len;
            if (s >= e) continue;
            const uint8_t* src = a.p.src + it.out_off + (int64_t)r * it.out_pitch + (s - rs);
            uint8_t* dst = unit + (s - it.p0);
            const int64_t n = e - s;
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += stride) {
                FOR_LANES(l) {
                    const int64_t q0 = 4 * (u0 + l) - mis;
                    if (u0 + l < units) {
                        if (q0 >= 0 && q0 + 4 <= n) {
                            const uint32_t v = (uint32_t)src[q0] | ((uint32_t)src[q0 + 1] << 8) | ((uint32_t)src[q0 + 2] << 16) |
                                               ((uint32_t)src[q0 + 3] << 24);
                            *reinterpret_cast<uint32_t*>(dst + q0) = v;
                        } else {
                            for (int i = 0; i < 4; i++) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) dst[q] = src[q];
                            }
                        }
                    }
                }
            }
        }
    }

    // overlay k of the unit by threads tid0 + lane, + stride, ...
    CIMG_DEV void overlay(int k, int tid0, int stride)
    {
        const TypedWindowItem* ip = a.items + pb.u.item0 + k;
        const WindowItem it = WindowBlock::uniform_item(ip);
        const int64_t cpitch = uni64(ip->cpitch), epitch = uni64(ip->epitch);
        const int ts = uni(ip->ts), src_type = uni(ip->src_type), out_type = uni(ip->out_type);
        const float scale = bits_f32(uni(f32_bits(ip->scale))), offset = bits_f32(uni(f32_bits(ip->offset)));
        const bool identity = out_type == src_type && scale == 1.0f && offset == 0.0f;
        if (identity && cpitch == ts && epitch == ts) { dense_rows(it, tid0, stride); return; }
        const int64_t len = pb.u.len, width = it.wbytes / ts;
        uint8_t* const unit = a.p.dst + pb.u.dst_off;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the unit
            // elements c_lo .. c_hi of the row lie inside [0, len) (whole: the planner admits no element over a unit's edge)
            const int64_t hi = len - ts - rel;
            if (hi < 0) continue;
            const int64_t c_lo = rel >= 0 ? 0 : (-rel + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            uint8_t* dst = unit + rel + c_lo * cpitch;                         // element c_lo (>= the unit's first byte)
            const uint8_t* src = a.p.src + it.out_off + (int64_t)r * it.out_pitch + c_lo * epitch;
            const int64_t ne = c_hi + 1 - c_lo;
            for (int64_t e0 = tid0; e0 < ne; e0 += stride) {
                FOR_LANES(l) {
                    const int64_t e = e0 + l;
                    if (e < ne) {
                        const uint8_t* s = src + e * epitch;
                        uint8_t* d = dst + e * cpitch;
                        if (identity) {
                            if (ts == 1) *d = *s;
                            else if (ts == 2) *reinterpret_cast<uint16_t*>(d) = *reinterpret_cast<const uint16_t*>(s);
                            else if (ts == 4) *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
                            else *reinterpret_cast<uint64_t*>(d) = *reinterpret_cast<const uint64_t*>(s);
                        } else {
                            const uint32_t v = typed_store_bits(typed_unscale(typed_load_mem(s, out_type), scale, offset), src_type);
                            if (ts == 1) *d = (uint8_t)v;
                            else if (ts == 2) *reinterpret_cast<uint16_t*>(d) = (uint16_t)v;
                            else *reinterpret_cast<uint32_t*>(d) = v;
                        }
                    }
                }
            }
        }
    }
};

// ---- masked patch: cimg_update_patch_masked ---------------------------------------------------------------------------------------
// The patch kernel of the masked / constant write calls.  Units, staging (PatchBlock::phase_a and phase_base) and the two schedules
// are those of the strided patch kernel; an item carries flags (WM_CONST: the written bytes are `value`, no source is read; WM_MASK:
// element c of window row r is written only if mask[mask_off + r * mask_pitch + c] != 0).  Three overlay paths:
//   dense_rows   items with cpitch == typesize that are unmasked, or masked with typesize 1 or 2 and elements that sit whole and
//                aligned in the unit: one lane a destination dword.  Unmasked: a whole dword is one store (of source bytes, or of the
//                value replicated at the dword's phase -- the fill reads no source at all), the ragged ends go byte by byte.  Masked:
//                the lane looks at the mask bytes of the dword's 4 or 2 elements; all set: one dword store, else one store per
//                written element.
//   elements     everything else (strided items, typesize 3 and other odd sizes, typesize 4 and 8 under a mask, elements over the
//                unit's edge): the strided overlay's walk c_lo .. c_hi, one lane an element, the element's mask byte in front of
//                its stores; a straddling element is written byte by byte by the units that hold its bytes, each consulting the
//                same mask byte.
// NO READ-MODIFY-WRITE: every store writes new bytes only -- a whole dword of them, or single elements / bytes.  Old and new bytes
// are never merged into a word that is then stored: under the disjoint schedule four waves write one unit with no barrier, and
// lanes of one wave write neighbouring bytes of one dword; byte-level disjointness protects byte stores, not a dword RMW.  (The
// host emulator runs waves one after the other and cannot show such a race: this is kept by construction.)
enum : int { WM_CONST = 1, WM_MASK = 2 };

struct MaskedWindowItem : StridedWindowItem {
    int64_t mask_off, mask_pitch;     // WM_MASK: the mask byte of element c of window row r is mask[mask_off + r * mask_pitch + c]
    uint64_t value;                   // WM_CONST: the element's bytes, byte i at bits 8 i
    int32_t flags;                    // WM_*
    int32_t pad2_;
};

struct MaskedPatchArgs {
    PatchArgs p;                      // (p.units and p.items unused; p.src may be null when every item is constant)
    const StridedPatchUnit* units;
    const MaskedWindowItem* items;    // overlays, in call order inside a unit
    const uint8_t* mask;              // (may be null when no item is masked)
};

struct MaskedPatchBlock {
    const MaskedPatchArgs& a;
    PatchBlock pb;
    int disjoint;

    CIMG_DEV MaskedPatchBlock(const MaskedPatchArgs& a_, uint8_t* lds, int k)
        : a(a_), pb(a_.p, lds, k, PatchBlock::uniform_unit(&a_.units[k].u)), disjoint(uni(a_.units[k].disjoint)) {}

    CIMG_DEV static uint32_t value_byte(uint64_t v, int i) { return (uint32_t)(v >> (8 * i)) & 0xFFu; }

    // rows r0 .. r1 of a dense item in dword units aligned on the destination.  masked: ts is 1 or 2 and every element of the rows
    // lies whole and ts-aligned in the unit (the caller checked)
    CIMG_DEV void dense_rows(const WindowItem& it, int ts, bool constant, bool masked, uint64_t value, int64_t mask_off, int64_t mask_pitch,
                             int tid0, int stride)
    {
        const int64_t len = pb.u.len;
        uint8_t* const unit = a.p.dst + pb.u.dst_off;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rs = it.row0 + (int64_t)r * it.rpitch, re = rs + it.wbytes;
            const int64_t s = rs > it.p0 ? rs : it.p0;
            const int64_t e = re < it.p0 + len ? re : it.p0 + len;
            if (s >= e) continue;
            const int64_t rb = s - rs;                                         // row byte of the first byte written here
            const uint8_t* src = constant ? nullptr : a.p.src + it.out_off + (int64_t)r * it.out_pitch + rb;
            const uint8_t* mrow = masked ? a.mask + mask_off + (int64_t)r * mask_pitch : nullptr;
            uint8_t* dst = unit + (s - it.p0);
            const int64_t n = e - s;
            const int64_t mis = (int64_t)((uintptr_t)dst & 3);
            const int64_t units = (mis + n + 3) >> 2;
            for (int64_t u0 = tid0; u0 < units; u0 += stride) {
                FOR_LANES(l) {
                    const int64_t q0 = 4 * (u0 + l) - mis;
                    if (u0 + l < units) {
                        const bool full = q0 >= 0 && q0 + 4 <= n;
                        // the four new bytes (those inside the row)
                        uint32_t b[4] = {0, 0, 0, 0};
                        if (constant) {
                            int ph = (int)((rb + (q0 < 0 ? 0 : q0)) % ts);             // element byte of the first byte inside
                            for (int i = 0; i < 4; i++) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) { b[i] = value_byte(value, ph); ph = ph + 1 == ts ? 0 : ph + 1; }
                            }
                        } else {
                            for (int i = 0; i < 4; i++) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) b[i] = src[q];
                            }
                        }
                        const uint32_t v = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
                        if (!masked) {
                            if (full) *reinterpret_cast<uint32_t*>(dst + q0) = v;
                            else
                                for (int i = 0; i < 4; i++) {
                                    const int64_t q = q0 + i;
                                    if (q >= 0 && q < n) dst[q] = (uint8_t)b[i];
                                }
                        } else {
                            // the mask bytes of the dword's elements (element of row byte x: x / ts)
                            bool w[4] = {false, false, false, false};
                            bool all = full;
                            for (int i = 0; i < 4; i += ts) {
                                const int64_t q = q0 + i;
                                if (q >= 0 && q < n) w[i] = mrow[(rb + q) / ts] != 0;
                                all = all && w[i];
                            }
                            if (all) *reinterpret_cast<uint32_t*>(dst + q0) = v;
                            else if (ts == 1) { for (int i = 0; i < 4; i++) if (w[i]) dst[q0 + i] = (uint8_t)b[i]; }
                            else { for (int i = 0; i < 4; i += 2) if (w[i]) *reinterpret_cast<uint16_t*>(dst + q0 + i) = (uint16_t)(b[i] | (b[i + 1] << 8)); }
                        }
                    }
                }
            }
        }
    }

    // overlay k of the unit by threads tid0 + lane, + stride, ...
    CIMG_DEV void overlay(int k, int tid0, int stride)
    {
        const MaskedWindowItem* ip = a.items + pb.u.item0 + k;
        const WindowItem it = WindowBlock::uniform_item(ip);
        const int64_t cpitch = uni64(ip->cpitch), mask_off = uni64(ip->mask_off), mask_pitch = uni64(ip->mask_pitch);
        const uint64_t value = (uint64_t)uni64((int64_t)ip->value);
        const int ts = uni(ip->ts), flags = uni(ip->flags);
        const bool constant = (flags & WM_CONST) != 0, masked = (flags & WM_MASK) != 0;
        const int64_t len = pb.u.len;
        uint8_t* const unit = a.p.dst + pb.u.dst_off;
        if (cpitch == ts && (!masked || ts == 1 || (ts == 2 && ((it.p0 | len | (int64_t)(uintptr_t)unit) & 1) == 0))) {
            dense_rows(it, ts, constant, masked, value, mask_off, mask_pitch, tid0, stride);
            return;
        }
        const int64_t width = it.wbytes / ts;
        const bool dwords = ts == 4 || ts == 8;
        for (int r = it.r0; r < it.r1; r++) {
            const int64_t rel = it.row0 + (int64_t)r * it.rpitch - it.p0;      // the row's first byte, seen from the unit
            // elements c_lo .. c_hi of the row have a byte in [0, len)
            const int64_t lo = -rel - (ts - 1), hi = len - 1 - rel;
            if (hi < 0) continue;
            const int64_t c_lo = lo <= 0 ? 0 : (lo + cpitch - 1) / cpitch;
            int64_t c_hi = hi / cpitch;
            if (c_hi > width - 1) c_hi = width - 1;
            if (c_lo > c_hi) continue;
            const int64_t base = rel + c_lo * cpitch;                          // unit offset of element c_lo (>= -(ts - 1))
            const uint8_t* src = constant ? nullptr : a.p.src + it.out_off + (int64_t)r * it.out_pitch + c_lo * ts;
            const uint8_t* m = masked ? a.mask + mask_off + (int64_t)r * mask_pitch + c_lo : nullptr;
            const int64_t ne = c_hi + 1 - c_lo;
            for (int64_t e0 = tid0; e0 < ne; e0 += stride) {
                FOR_LANES(l) {
                    const int64_t e = e0 + l;
                    if (e < ne && (!masked || m[e] != 0)) {
                        const int64_t at = base + e * cpitch;                  // the element's bytes: [at, at + ts) of the unit
                        const uint8_t* s = constant ? nullptr : src + e * ts;
                        uint8_t* d = unit + at;
                        if (dwords && at >= 0 && at + ts <= len && ((uintptr_t)d & 3) == 0) {
                            for (int i = 0; i < ts; i += 4) {
                                const uint32_t v = constant ? (uint32_t)(value >> (8 * i))
                                                            : (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 24);
                                *reinterpret_cast<uint32_t*>(d + i) = v;
                            }
                        } else {
                            for (int i = 0; i < ts; i++)
                                if (at + i >= 0 && at + i < len) d[i] = constant ? (uint8_t)value_byte(value, i) : s[i];
                        }
                    }
                }
            }
        }
    }
};

// ---- splice ---------------------------------------------------------------------------------------------------------------------
enum : int { SPLICE_REGULAR = 0, SPLICE_ZERO = 2, SPLICE_WHOLE = 4, SPLICE_DAMAGED = 5 };

struct SpliceChunk {
    int64_t old_off;      // the old chunk at old_comp + old_off
    int64_t new_off;      // its new form at new_comp + new_off
    int32_t old_cbytes;   // bytes of the old chunk (its header's cbytes, checked against what the buffer holds)
    int32_t destsize;     // capacity of the new chunk (the running-destsize rule)
    int32_t nbytes, blocksize, nblocks, leftover;
    int32_t split;        // 1: full blocks are cut into typesize streams
    int32_t flags;        // header flags byte of the new chunk
    int32_t blk0;         // its first entry in SpliceArgs::blocks
    int32_t nstreams;     // streams of the chunk
};

struct SpliceBlock {
    int32_t chunk;        // SpliceArgs::chunks index
    int32_t j;            // block of the chunk
    int32_t unit;         // >= 0: re-encoded (its records and slot are those of encode-plan block `unit`); -1: harvested
    int32_t new_pos;      // layout: where the block starts in the new chunk
    int32_t old_pos;      // layout: where it starts in the old chunk
    int32_t len;          // layout: its bytes (csize words and payloads)
};

struct SpliceArgs {
    const SpliceChunk* chunks;
    int32_t nchunks;
    int32_t nblocks;
    SpliceBlock* blocks;
    CodecParams p;            // the encode plan's
    const uint8_t* old_comp;
    uint8_t* new_comp;
    const uint8_t* scratch;   // payloads of re-encoded streams: block `unit`'s slot, stream s at s * neblock
    const StreamRec* recs;
    ChunkLayout* layout;      // per chunk: cbytes (SPLICE_DAMAGED: the error code) and mode (SPLICE_*)
};

CIMG_DEV SpliceChunk uniform_splice_chunk(const SpliceChunk* p)
{
    SpliceChunk c = *p;
    c.old_off = uni64(c.old_off); c.new_off = uni64(c.new_off);
    c.old_cbytes = uni(c.old_cbytes); c.destsize = uni(c.destsize); c.nbytes = uni(c.nbytes); c.blocksize = uni(c.blocksize);
    c.nblocks = uni(c.nblocks); c.leftover = uni(c.leftover); c.split = uni(c.split); c.flags = uni(c.flags); c.blk0 = uni(c.blk0);
    c.nstreams = uni(c.nstreams);
    return c;
}

struct SpliceLayout {
    const SpliceArgs& a;
    int chunk;
    CIMG_DEV SpliceLayout(const SpliceArgs& a_, int chunk_) : a(a_), chunk(chunk_) {}

    // stream s of lane's block: csize word (harvested) or record (re-encoded) -> payload bytes, and whether the block is damaged
    CIMG_DEV void run()
    {
        const SpliceChunk d = uniform_splice_chunk(a.chunks + chunk);
        const uint8_t* o = a.old_comp + d.old_off;
        uint8_t* c = a.new_comp + d.new_off;
        const int ts = a.p.typesize;
        int nt = HEADER_LEN + 4 * d.nblocks;
        int mode = SPLICE_REGULAR, code = 0;
        if (nt > d.destsize) mode = SPLICE_WHOLE;
        if (d.old_cbytes < nt) { mode = SPLICE_DAMAGED; code = ERR_READ_BUFFER; }
        for (int j0 = 0; j0 < d.nblocks && mode == SPLICE_REGULAR; j0 += 64) {
            LV<int> sz, pre, opos, unit;
            LV<bool> bad, hand;
            FOR_LANES(l) {
                const int j = j0 + l;
                sz[l] = 0; opos[l] = 0; unit[l] = -1; bad[l] = false; hand[l] = false;
                if (j < d.nblocks) {
                    const SpliceBlock& sb = a.blocks[d.blk0 + j];
                    const bool lb = j == d.nblocks - 1 && d.leftover;
                    const int bsize = lb ? d.leftover : d.blocksize;
                    const int ns = (d.split && !lb) ? ts : 1;
                    const int neblock = bsize / ns;
                    unit[l] = sb.unit;
                    if (sb.unit >= 0) {
                        for (int s = 0; s < ns; s++) sz[l] += 4 + rec_payload(a.recs[(int64_t)sb.unit * a.p.streams_per_block + s]);
                    } else {
                        const int b0 = ld32s(o + HEADER_LEN + 4 * j);
                        opos[l] = b0;
                        if (b0 < HEADER_LEN + 4 * d.nblocks || b0 > d.old_cbytes) { bad[l] = true; }
                        else {
                            int pos = b0;
                            for (int s = 0; s < ns; s++) {
                                if (d.old_cbytes - pos < 4) { bad[l] = true; break; }
                                const int cs = ld32s(o + pos);
                                pos += 4;
                                const int payload = cs > 0 ? cs : (cs < 0 ? 1 : 0);
                                if (cs > neblock || cs < -255 || payload > d.old_cbytes - pos) { bad[l] = true; break; }
                                pos += payload;
                            }
                            sz[l] = pos - b0;
                        }
                    }
                }
            }
            if (ballot(bad)) { mode = SPLICE_DAMAGED; code = ERR_DATA; break; }
            int tile_total;
            wave_exscan(sz, pre, tile_total);
            FOR_LANES(l) {
                const int j = j0 + l;
                if (j < d.nblocks) {
                    SpliceBlock& sb = a.blocks[d.blk0 + j];
                    const bool lb = j == d.nblocks - 1 && d.leftover;
                    const int bsize = lb ? d.leftover : d.blocksize;
                    const int ns = (d.split && !lb) ? ts : 1;
                    const int neblock = bsize / ns;
                    sb.new_pos = nt + pre[l]; sb.old_pos = opos[l]; sb.len = sz[l];
                    st32(c + HEADER_LEN + 4 * j, nt + pre[l]);
                    // LayoutChunk's running-destsize rule, stream by stream
                    int pos = nt + pre[l], hp = opos[l];
                    bool f = false;
                    for (int s = 0; s < ns; s++) {
                        const int N = pos + 4;
                        int kind, value, csize, need = 0;
                        bool known = true;
                        if (unit[l] >= 0) {
                            const StreamRec r = a.recs[(int64_t)unit[l] * a.p.streams_per_block + s];
                            kind = r.kind; value = r.value; csize = r.csize; need = r.need;
                        } else {
                            const int cs = ld32s(o + hp);
                            kind = cs <= 0 ? REC_RUN : cs == neblock ? REC_RAW : REC_LZ4;
                            value = cs < 0 ? -cs : 0; csize = cs > 0 ? cs : 0;
                            known = kind != REC_LZ4;
                            hp += 4 + (cs > 0 ? cs : (cs < 0 ? 1 : 0));
                        }
                        if (kind == REC_RUN) {
                            f |= N > d.destsize || (value > 0 && N + 1 > d.destsize);
                            pos += 4 + (value > 0 ? 1 : 0);
                        } else {
                            int maxout = neblock;
                            if (N + maxout > d.destsize) {
                                if (!known) hand[l] = true;
                                maxout = d.destsize - N;
                                if (maxout <= 0) f = true;
                            }
                            if (!f && known) {
                                if (kind == REC_LZ4) { if (need > maxout) f = true; }
                                else if (N + neblock > d.destsize) f = true;
                            }
                            pos += 4 + csize;
                        }
                    }
                    hand[l] = hand[l] || f;
                }
            }
            if (ballot(hand)) mode = SPLICE_WHOLE;
            nt += tile_total;
        }
        int cbytes = 0;
        if (mode == SPLICE_REGULAR) {
            AssembleArgs aa{};
            aa.p = a.p;
            LayoutChunk lc(aa, 0);
            ChunkDesc hd{};
            hd.nbytes = d.nbytes; hd.blocksize = d.blocksize;
            if (nt == HEADER_LEN + 4 * d.nblocks + 4 * d.nstreams) {
                mode = SPLICE_ZERO; cbytes = HEADER_LEN;
                lc.write_header(hd, c, d.flags, HEADER_LEN, SPECIAL_ZERO << 4);
            } else {
                cbytes = nt;
                lc.write_header(hd, c, d.flags, nt, 0);
            }
        }
        if (mode == SPLICE_DAMAGED) cbytes = code;
        FOR_LANES_W(l) { if (l == 0) { a.layout[chunk].cbytes = cbytes; a.layout[chunk].mode = mode; } }
    }
};

struct SpliceEmit {
    const SpliceArgs& a;
    int k;
    CIMG_DEV SpliceEmit(const SpliceArgs& a_, int k_) : a(a_), k(k_) {}

    CIMG_DEV void run(int wave, int nwaves = 4)
    {
        const SpliceBlock* bp = a.blocks + k;
        const int chunk = uni(bp->chunk), j = uni(bp->j), unit = uni(bp->unit);
        const int new_pos = uni(bp->new_pos), old_pos = uni(bp->old_pos), len = uni(bp->len);
        if (uni(a.layout[chunk].mode) != SPLICE_REGULAR) return;
        const SpliceChunk d = uniform_splice_chunk(a.chunks + chunk);
        uint8_t* c = a.new_comp + d.new_off;
        if (unit < 0) { wave_copy_g2g(a.old_comp + d.old_off + old_pos, c + new_pos, len, wave, nwaves); return; }
        const bool lb = j == d.nblocks - 1 && d.leftover;
        const int bsize = lb ? d.leftover : d.blocksize;
        const int ns = (d.split && !lb) ? a.p.typesize : 1;
        const int neblock = bsize / ns;
        const uint8_t* slot = a.scratch + (int64_t)unit * a.p.slot_bytes;
        const StreamRec* rp = a.recs + (int64_t)unit * a.p.streams_per_block;
        int pos = new_pos;
        for (int s = 0; s < ns; s++) {
            StreamRec r;
            r.kind = uni(rp[s].kind); r.value = uni(rp[s].value); r.csize = uni(rp[s].csize); r.need = 0;
            if (wave == 0) {
                const int word = r.kind == REC_RUN ? -r.value : r.csize;
                FOR_LANES(l) {
                    if (l < 4) c[pos + l] = (uint8_t)(((uint32_t)word >> (8 * l)) & 0xFF);
                    if (l == 4 && r.kind == REC_RUN && r.value > 0) c[pos + 4] = 0x01;
                }
            }
            pos += 4;
            if (r.kind != REC_RUN) wave_copy_g2g(slot + (int64_t)s * neblock, c + pos, r.csize, wave, nwaves);
            pos += rec_payload(r);
        }
    }
};

}  // namespace cimg
