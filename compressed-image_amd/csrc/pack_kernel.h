// pack_kernel.h -- a batched gather copy: many pieces of very different sizes, each from its own address to its own address.
//
// What it is for: compressed chunks leave the encode launch at destsize-spaced offsets (every chunk has room for its nominal
// size + overhead), and an object that keeps an image compressed in HBM wants them back to back at their real sizes
// (cimg_compress_batch_device_packed_fetch, cimg_pack_chunks_device, the repack behind a window write).  Pieces run from a
// 32-byte header-only chunk to 4 MiB + overhead, tens of thousands of them in a call.
//
// Work is cut into tiles of PACK_TILE bytes of a piece's DESTINATION-aligned middle, one wave per tile, so the time of a call
// follows its total bytes: a 4 MiB piece is 256 tiles, a 40-byte piece one.  A piece is
//     head   0..15 bytes up to the first 16-byte boundary of the destination      (its first tile, byte stores)
//     middle whole 16-byte units: aligned 16-byte stores, 16-byte loads at whatever alignment the source has there
//     tail   0..15 bytes                                                            (its last tile, byte stores)
// The host lists the pieces with the index of their first tile (ascending); a wave finds its piece by binary search (wave-uniform:
// scalar loads), so the table that crosses PCIe has one entry per piece, not per tile.  Every byte is read once and written once;
// nothing outside [dst, dst + bytes) is written.
#pragma once
#include "decode_kernel.h"   // u128 helpers, uni64
#include <algorithm>
#include <vector>

namespace cimg {

constexpr int PACK_TILE = 16384;            // bytes of a piece's middle per wave: 16 loads of 16 bytes per lane, 8 in flight

struct PackPiece {
    const uint8_t* src;
    uint8_t* dst;
    int32_t bytes;                           // > 0 (the host drops empty pieces)
    int32_t tile0;                           // index of the piece's first tile in the launch
};

struct PackArgs {
    const PackPiece* pieces;                 // ordered by tile0
    int32_t npieces;
    int32_t ntiles;
};

// 16-byte loads at any alignment / aligned 16-byte stores through pointers the compiler knows to be global memory (the addresses come
// out of the piece table, where it cannot see that: it would emit flat instructions)
#if defined(CIMG_EMULATE) || !defined(__HIP_DEVICE_COMPILE__)      // (the emulator; hipcc's host pass, which only parses the kernels)
CIMG_DEV u128 pack_ld(const uint8_t* p) { return ld128u(p); }
CIMG_DEV void pack_st(uint8_t* p, const u128& v) { st128a(p, v); }
#else
typedef u128 __attribute__((aligned(1))) pack_u128_any;
CIMG_DEV u128 pack_ld(const uint8_t* p) { return *(const __attribute__((address_space(1))) pack_u128_any*)(uintptr_t)p; }
CIMG_DEV void pack_st(uint8_t* p, const u128& v) { *(__attribute__((address_space(1))) u128*)(uintptr_t)p = v; }
#endif

// bytes in front of the destination's first 16-byte boundary (the whole piece if it ends before that)
CIMG_HD int pack_head_bytes(uintptr_t dst, int bytes)
{
    const int h = (int)((16 - (dst & 15)) & 15);
    return h < bytes ? h : bytes;
}
// tiles of one piece: its middle in PACK_TILE steps, at least one (head and tail ride on the first and the last)
CIMG_HD int pack_tiles_of(uintptr_t dst, int bytes)
{
    const int mid = (bytes - pack_head_bytes(dst, bytes)) & ~15;
    const int t = (mid + PACK_TILE - 1) / PACK_TILE;
    return t > 0 ? t : 1;
}

CIMG_DEV void pack_wave(const PackArgs& a, int tile)
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
    const int head = pack_head_bytes((uintptr_t)dst, bytes);
    const int mid = (bytes - head) & ~15;
    const int ntiles = pack_tiles_of((uintptr_t)dst, bytes);
    if (t == 0) { FOR_LANES_W(l) { if (l < head) dst[l] = src[l]; } }
    // ---- the tile's share of the middle ---------------------------------------------------------------------------
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
        for (int k = 0; k < DEPTH; k++) { FOR_LANES_W(l) { pack_st(d + 16 * (size_t)(u0 + 64 * k + l), r[k][l]); } }
    }
    for (; u0 < units; u0 += 64) {
        LV<u128> r;
        FOR_LANES(l) { if (u0 + l < units) r[l] = pack_ld(s + 16 * (size_t)(u0 + l)); }
        FOR_LANES_W(l) { if (u0 + l < units) pack_st(d + 16 * (size_t)(u0 + l), r[l]); }
    }
    if (t == ntiles - 1) {
        const int done = head + mid;
        FOR_LANES_W(l) { if (done + l < bytes) dst[done + l] = src[done + l]; }
    }
}

// ---- host side: the piece table of one call -------------------------------------------------------------------------
// Empty pieces are dropped.  Returns 0, or -1 for a negative size, -2 if a destination range overlaps another destination or any
// source range of the call (sources may overlap each other: they are only read), -3 for more tiles than a launch has workgroups.
inline int pack_plan(int n, const void* const* src, const int32_t* bytes, uint8_t* dst, const int64_t* dst_off,
                     std::vector<PackPiece>& pieces, int64_t* ntiles)
{
    pieces.clear();
    int64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        if (bytes[i] < 0) return -1;
        if (bytes[i] == 0) continue;
        if (tiles > 0x7fffffff) return -3;
        uint8_t* d = dst + dst_off[i];
        pieces.push_back(PackPiece{(const uint8_t*)src[i], d, bytes[i], (int32_t)tiles});
        tiles += pack_tiles_of((uintptr_t)d, bytes[i]);
    }
    if (tiles > 0x7fffffff) return -3;
    *ntiles = tiles;
    struct Range { uintptr_t a, b; bool is_dst; };
    std::vector<Range> r;
    r.reserve(2 * pieces.size());
    for (const PackPiece& p : pieces) {
        r.push_back(Range{(uintptr_t)p.src, (uintptr_t)p.src + (uintptr_t)p.bytes, false});
        r.push_back(Range{(uintptr_t)p.dst, (uintptr_t)p.dst + (uintptr_t)p.bytes, true});
    }
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.a < y.a; });
    uintptr_t src_end = 0, dst_end = 0;                           // furthest end of the ranges of each kind that start earlier
    for (const Range& x : r) {
        if (x.a < dst_end || (x.is_dst && x.a < src_end)) return -2;
        if (x.is_dst) dst_end = std::max(dst_end, x.b); else src_end = std::max(src_end, x.b);
    }
    return 0;
}

}  // namespace cimg
