// tests/emu/pack_emu.cpp -- TEST INFRASTRUCTURE: the pack and interleave kernels on the host lane emulator, as a library of their own
// (tests/test_emu_pack.py and tests/test_interleave.py compile it into a pytest temp directory; the sanitizer build links
// pack_asan_main.cpp beside it).
#define CIMG_EMULATE 1
#include "pack_env.h"

namespace cimg { int g_emu_write_order = 0; }
using namespace cimg;

extern "C" {

void pkemu_write_order(int order) { g_emu_write_order = order; }

int pkemu_pack(int n, const void* const* src, const int32_t* bytes, uint8_t* dst, const int64_t* dst_off)
{
    return emu_pack_chunks(n, src, bytes, dst, dst_off);
}

// tiles a call is cut into (the time of a launch follows this, not the piece count or the largest piece)
int64_t pkemu_tiles(int n, const void* const* src, const int32_t* bytes, uint8_t* dst, const int64_t* dst_off)
{
    std::vector<PackPiece> pieces;
    int64_t ntiles = 0;
    const int rc = pack_plan(n, src, bytes, dst, dst_off, pieces, &ntiles);
    return rc ? rc : ntiles;
}

int pkemu_interleave(const uint8_t* src, int64_t plane_stride, int nch, int ts, int64_t npixels, uint8_t* dst)
{
    return emu_interleave(src, plane_stride, nch, ts, npixels, dst);
}

// the product's deinterleave body, for interleave(deinterleave(x)) == x
int pkemu_deinterleave(const uint8_t* src, int nch, int ts, int64_t npixels, uint8_t* dst, int64_t plane_stride)
{
    if (nch < 1 || (ts != 1 && ts != 2 && ts != 4 && ts != 8) || (plane_stride & 15) || plane_stride < npixels * ts || nch * ts * 16 > 16384) return -12;
    const int tile = deinterleave_tile_pixels(nch, ts), lds_bytes = deinterleave_lds_bytes(nch, ts);
    DeinterleaveArgs a{src, dst, plane_stride, npixels, nch, ts, tile, lds_bytes};
    for (int64_t t = 0; t * tile < npixels; t++) {
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK, 0xCD);
        deinterleave_wave(a, lds.data(), t);
    }
    return 0;
}

}  // extern "C"
