// interleave_kernel.h -- one plane per channel -> interleaved pixels (R G B A R G B A ...), on the device: the inverse of
// deinterleave_kernel.h, with the same argument meaning and the same tiles.
//
// What it is for: a window decoded from a compressed image comes out as one plane per channel (C, h, w); a consumer that wants
// (h, w, C) gets it here without a trip through the host (cimg_interleave_device).
//
// One wave per tile of deinterleave_tile_pixels() pixels.  The tile's piece of every plane is staged into LDS with 16-byte
// coalesced loads (plane c at c * interleave_plane_lds()), then each lane gathers the 16 / typesize elements of 16 consecutive
// OUTPUT bytes from LDS -- element e of the tile is channel e % nch of pixel e / nch -- and stores them with one 16-byte coalesced
// store.  HBM traffic is the algorithmic minimum: every byte read once, written once.
#pragma once
#include "deinterleave_kernel.h"

namespace cimg {

struct InterleaveArgs {
    const uint8_t* src;       // plane c starts at src + c * plane_stride
    uint8_t* dst;             // npixels * nch elements of ts bytes, interleaved
    int64_t plane_stride;     // bytes, a multiple of 16
    int64_t npixels;
    int32_t nch, ts;          // channels, bytes per element (1, 2, 4 or 8)
    int32_t tile_pixels;      // deinterleave_tile_pixels(nch, ts)
    int32_t lds_bytes;
};

// LDS bytes between the staged pieces of two planes: a tile's piece, a multiple of 16, plus one unit so that the channels of a
// pixel do not all fall on one bank
CIMG_HD int interleave_plane_lds(int nch, int ts) { return ((deinterleave_tile_pixels(nch, ts) * ts + 15) & ~15) + 16; }
CIMG_HD int interleave_lds_bytes(int nch, int ts) { return nch * interleave_plane_lds(nch, ts) + 16; }

template <int TS> CIMG_DEV void interleave_tile(const InterleaveArgs& a, uint8_t* lds, int64_t tile)
{
    constexpr int G = 16 / TS;                                  // elements in 16 output bytes
    const int nch = a.nch;
    const int pl = interleave_plane_lds(nch, TS);
    const int64_t p0 = tile * a.tile_pixels;
    const int np = (int)(a.npixels - p0 < a.tile_pixels ? a.npixels - p0 : a.tile_pixels);
    const int pbytes = np * TS;
    // ---- stage the tile's piece of every plane -------------------------------------------------------------------
    for (int c = 0; c < nch; c++) {
        const uint8_t* src = a.src + (int64_t)c * a.plane_stride + p0 * TS;          // 16-byte aligned: p0 is a multiple of 16
        wave_copy_g2l(src, lds, c * pl, pbytes & ~15);
        const int t = pbytes & ~15;
        FOR_LANES_W(l) { if (t + l < pbytes) lds[c * pl + t + l] = src[t + l]; }
    }
    // ---- 16 output bytes per lane -----------------------------------------------------------------------------------
    const int bytes = np * nch * TS;
    const int units = bytes >> 4;
    uint8_t* out = a.dst + p0 * nch * TS;                                             // 16-byte aligned
    for (int u0 = 0; u0 < units; u0 += 64) {
        LV<u128> o;
        FOR_LANES(l) {
            const int u = u0 + l < units ? u0 + l : 0;
            int px = (u * G) / nch, ch = (u * G) - px * nch;
            uint32_t w[4] = {0, 0, 0, 0};
            CIMG_UNROLL
            for (int k = 0; k < G; k++) {
                const uint64_t e = lds_element<TS>(lds, ch * pl + px * TS);
                if constexpr (TS == 8) { w[2 * k] = (uint32_t)e; w[2 * k + 1] = (uint32_t)(e >> 32); }
                else w[(k * TS) >> 2] |= (uint32_t)e << (8 * ((k * TS) & 3));
                if (++ch == nch) { ch = 0; px++; }
            }
            o[l].x = w[0]; o[l].y = w[1]; o[l].z = w[2]; o[l].w = w[3];
        }
        FOR_LANES_W(l) { if (u0 + l < units) st128a(out + 16 * (size_t)(u0 + l), o[l]); }
    }
    // the bytes of a last, short tile that do not fill 16
    const int done = units << 4;
    FOR_LANES_W(l) {
        if (done + l < bytes) {
            const int e = (done + l) / TS;
            out[done + l] = lds[(e % nch) * pl + (e / nch) * TS + (done + l) % TS];
        }
    }
}

CIMG_DEV void interleave_wave(const InterleaveArgs& a, uint8_t* lds, int64_t tile)
{
    switch (a.ts) {
    case 1: interleave_tile<1>(a, lds, tile); break;
    case 2: interleave_tile<2>(a, lds, tile); break;
    case 4: interleave_tile<4>(a, lds, tile); break;
    default: interleave_tile<8>(a, lds, tile); break;
    }
}

}  // namespace cimg
