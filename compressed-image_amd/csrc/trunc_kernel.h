// trunc_kernel.h -- blosc2's trunc-prec filter as a masked batched copy: many pieces (the chunks of a compress call), each from its own
// address to its own address -- or onto itself -- with the low mantissa bits of every whole element cleared on the way (trunc_plan.h
// has the rules and the mask).  The shape is pack_kernel.h's: tiles of PACK_TILE bytes of a piece's DESTINATION-aligned middle, one
// wave per tile, found by binary search over the pieces' first tiles; aligned 16-byte stores, 16-byte loads at whatever alignment the
// source has, byte-wise head and tail.
//
// The mask goes by byte phase relative to the PIECE START: byte k of a piece is ANDed with byte k % typesize of the element mask, so a
// piece at an address that is no multiple of the typesize is masked like any other.  The bytes behind the last whole element
// (bytes % typesize of them) are copied as they are.  dst == src is allowed: every byte is read once and written once by the same lane,
// and a lane's loads of a round all come before its stores.  Nothing outside [dst, dst + bytes) is written.
#pragma once
#include "pack_kernel.h"
#include "trunc_plan.h"

namespace cimg {

struct TruncArgs {
    const PackPiece* pieces;                 // ordered by tile0
    int32_t npieces;
    int32_t ntiles;
    uint64_t mask64;                         // trunc_mask64: the element mask replicated over eight bytes
    int32_t typesize;                        // 2, 4 or 8
    int32_t pad_;
};

// the middle ends with the last whole element: what lies behind it rides on the tail, byte by byte
CIMG_HD int trunc_mid_bytes(uintptr_t dst, int bytes, int typesize)
{
    const int whole = bytes - bytes % typesize;
    const int head = pack_head_bytes(dst, bytes);
    return whole > head ? (whole - head) & ~15 : 0;
}
CIMG_HD int trunc_tiles_of(uintptr_t dst, int bytes, int typesize)
{
    const int t = (trunc_mid_bytes(dst, bytes, typesize) + PACK_TILE - 1) / PACK_TILE;
    return t > 0 ? t : 1;
}

CIMG_DEV u128 trunc_and(const u128& v, uint32_t lo, uint32_t hi)
{
    u128 r;
    r.x = v.x & lo; r.y = v.y & hi; r.z = v.z & lo; r.w = v.w & hi;
    return r;
}

CIMG_DEV void trunc_wave(const TruncArgs& a, int tile)
{
    int lo = 0, hi = a.npieces - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (uni(a.pieces[mid].tile0) <= tile) lo = mid; else hi = mid - 1;
    }
    const PackPiece* pp = a.pieces + lo;
    const uint8_t* src = (const uint8_t*)(uintptr_t)uni64((int64_t)(uintptr_t)pp->src);
    uint8_t* dst = (uint8_t*)(uintptr_t)uni64((int64_t)(uintptr_t)pp->dst);
    const int bytes = uni(pp->bytes);
    const int t = tile - uni(pp->tile0);
    const int ts = a.typesize;
    const uint64_t m64 = a.mask64;
    const int whole = bytes - bytes % ts;                                     // bytes in whole elements: the masked part
    const int head = pack_head_bytes((uintptr_t)dst, bytes);
    const int mid = trunc_mid_bytes((uintptr_t)dst, bytes, ts);
    const int ntiles = trunc_tiles_of((uintptr_t)dst, bytes, ts);
    // byte k of the piece: masked by byte k % typesize of the element mask (the typesize divides 8), kept whole behind the last element
    if (t == 0) {
        FOR_LANES_W(l) {
            if (l < head) dst[l] = (uint8_t)(src[l] & (l < whole ? (uint32_t)(m64 >> (8 * (l & 7))) : 0xFFu));
        }
    }
    // ---- the tile's share of the middle: 16-byte units that all start at the same phase of an element ------------------------
    const int phase = head & (ts - 1);
    const uint64_t rot = phase ? (m64 >> (8 * phase)) | (m64 << (64 - 8 * phase)) : m64;
    const uint32_t mlo = (uint32_t)rot, mhi = (uint32_t)(rot >> 32);
    const int m0 = t * PACK_TILE;
    const int mlen = mid - m0 < PACK_TILE ? mid - m0 : PACK_TILE;            // <= 0: a piece without a middle
    const uint8_t* s = src + head + m0;
    uint8_t* d = dst + head + m0;                                             // 16-byte aligned
    const int units = mlen > 0 ? mlen >> 4 : 0;
    constexpr int DEPTH = 8;
    int u0 = 0;
    for (; u0 + 64 * DEPTH <= units; u0 += 64 * DEPTH) {
        LV<u128> r[DEPTH];
        CIMG_UNROLL
        for (int k = 0; k < DEPTH; k++) { FOR_LANES(l) { r[k][l] = pack_ld(s + 16 * (size_t)(u0 + 64 * k + l)); } }
        CIMG_UNROLL
        for (int k = 0; k < DEPTH; k++) { FOR_LANES_W(l) { pack_st(d + 16 * (size_t)(u0 + 64 * k + l), trunc_and(r[k][l], mlo, mhi)); } }
    }
    for (; u0 < units; u0 += 64) {
        LV<u128> r;
        FOR_LANES(l) { if (u0 + l < units) r[l] = pack_ld(s + 16 * (size_t)(u0 + l)); }
        FOR_LANES_W(l) { if (u0 + l < units) pack_st(d + 16 * (size_t)(u0 + l), trunc_and(r[l], mlo, mhi)); }
    }
    // ---- tail: up to 15 bytes of whole elements and up to typesize - 1 behind them (at most 22: one round of lanes) ---------
    if (t == ntiles - 1) {
        const int done = head + mid;
        FOR_LANES_W(l) {
            const int k = done + l;
            if (k < bytes) dst[k] = (uint8_t)(src[k] & (k < whole ? (uint32_t)(m64 >> (8 * (k & 7))) : 0xFFu));
        }
    }
}

// ---- host side: the piece table of one pass ----------------------------------------------------------------------------
// Piece i goes from src[i] to dst[i] (the same address: in place).  Empty pieces are dropped.  Returns 0, -1 for a negative size or a
// typesize the filter does not know, -3 for more tiles than a launch has workgroups.  The caller answers for the ranges: the pieces of
// a call are the chunks of one compress batch, which the engine lays out itself.
inline int trunc_plan_pieces(int n, const void* const* src, void* const* dst, const int32_t* bytes, int typesize,
                             std::vector<PackPiece>& pieces, int64_t* ntiles)
{
    pieces.clear();
    if (trunc_mantissa_width(typesize) == 0) return -1;
    int64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        if (bytes[i] < 0) return -1;
        if (bytes[i] == 0) continue;
        if (tiles > 0x7fffffff) return -3;
        pieces.push_back(PackPiece{(const uint8_t*)src[i], (uint8_t*)dst[i], bytes[i], (int32_t)tiles});
        tiles += trunc_tiles_of((uintptr_t)dst[i], bytes[i], typesize);
    }
    if (tiles > 0x7fffffff) return -3;
    *ntiles = tiles;
    return 0;
}

}  // namespace cimg
