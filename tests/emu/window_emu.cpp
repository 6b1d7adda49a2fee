// tests/emu/window_emu.cpp -- TEST INFRASTRUCTURE: window calls (csrc/window_plan.h, csrc/window_kernel.h) on the host lane
// emulator.  Linked with emu.cpp and wide_emu.cpp (tests/test_emu_windows.py builds the three into one library): chunks decoded
// whole go through wemu_decompress_batch, which routes them the way engine.hip does (normal blocks and zstd: emu.cpp; blocks beyond
// LDS: the wide kernel).
#define CIMG_EMULATE 1
#include "window_env.h"

using namespace cimg;

extern "C" {

int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);

static WindowStats g_wnemu_stats;

// = cimg_decompress_windows_device
int wnemu_windows_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                         const int32_t* blocksize, int typesize, int nwindows, const WindowSpec* w, uint8_t* out, int32_t* status)
{
    return emu_windows_device(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w, out,
                              status, &g_wnemu_stats);
}

// = cimg_decompress_windows_host
int wnemu_windows_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                       const WindowSpec* w, uint8_t* out, int32_t* status)
{
    return emu_windows_host(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nwindows, w, out, status, &g_wnemu_stats);
}

// = cimg_engine_window_stats
void wnemu_window_stats(int64_t* out)
{
    out[0] = g_wnemu_stats.blocks_decoded; out[1] = g_wnemu_stats.chunks_whole; out[2] = g_wnemu_stats.comp_bytes_uploaded;
}

}  // extern "C"
