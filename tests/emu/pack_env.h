// tests/emu/pack_env.h -- TEST INFRASTRUCTURE: the pack kernel (csrc/pack_kernel.h) and the interleave kernel
// (csrc/interleave_kernel.h) on the host lane emulator, tile by tile as a launch would run them.  Shared by pack_emu.cpp (the kernel
// tests) and mock_device.cpp (the mock C ABI).  Include with CIMG_EMULATE defined.
#pragma once
#include "wave.h"
#include "pack_kernel.h"
#include "blosclz_kernel.h"   // (decode_kernel.h declares its decoder)
#include "interleave_kernel.h"
#include <vector>

#ifndef EMU_LDS_SLACK
#define EMU_LDS_SLACK 64
#endif

namespace cimg {

// = cimg_pack_chunks_device: 0, or -12 (BLOSC2_ERROR_INVALID_PARAM) where the engine refuses the call
inline int emu_pack_chunks(int n, const void* const* src, const int32_t* bytes, uint8_t* dst, const int64_t* dst_off)
{
    if (n < 0 || (n > 0 && (!src || !bytes || !dst || !dst_off))) return -12;
    std::vector<PackPiece> pieces;
    int64_t ntiles = 0;
    if (pack_plan(n, src, bytes, dst, dst_off, pieces, &ntiles)) return -12;
    for (const PackPiece& p : pieces) if (!p.src) return -12;
    if (pieces.empty()) return 0;
    PackArgs a{pieces.data(), (int32_t)pieces.size(), (int32_t)ntiles};
    for (int64_t t = 0; t < ntiles; t++) pack_wave(a, (int)t);
    return 0;
}

// = cimg_interleave_device (LDS of exactly the launch size)
inline int emu_interleave(const uint8_t* src, int64_t plane_stride, int nch, int ts, int64_t npixels, uint8_t* dst)
{
    if (nch < 1 || nch > 4096 || (ts != 1 && ts != 2 && ts != 4 && ts != 8) || npixels < 0 || (plane_stride & 15) || plane_stride < npixels * ts ||
        nch * ts * 16 > 16384 || !src || !dst)
        return -12;
    const int tile = deinterleave_tile_pixels(nch, ts), lds_bytes = interleave_lds_bytes(nch, ts);
    InterleaveArgs a{src, dst, plane_stride, npixels, nch, ts, tile, lds_bytes};
    for (int64_t t = 0; t * tile < npixels; t++) {
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK, 0xCD);
        interleave_wave(a, lds.data(), t);
    }
    return 0;
}

}  // namespace cimg
