// tests/emu/mock_window.cpp -- TEST INFRASTRUCTURE: the window entry points of include/cimg_hip.h (cimg_decompress_windows_device /
// _host, cimg_engine_window_stats) on the host lane emulator, for the mock build of the Python module
// (compressed-image_amd/python/Makefile, `mock`): the planner and the window kernel's body of csrc/, chunks decoded whole through
// emu.cpp's batch function (which libcimg_hip_mock.so exports).  Device pointers are host pointers here, as in mock_cabi.cpp.
#define CIMG_EMULATE 1
#include "window_env.h"
#include "../../include/cimg_hip.h"

using namespace cimg;

extern "C" int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes,
                                    const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);

// mock_cabi.cpp: a host-resident window call goes through the engine's staging area, so a batch staged there by a compress _begin is
// void after it (include/cimg_hip.h); the host calls of this file and of the files that include it say so through this
extern "C" void cimg_mock_void_staged(cimg_engine* e);

namespace {

WindowStats g_stats;

int whole(int n, const uint8_t* comp, const int64_t* comp_off, const int32_t*, const int32_t* nbytes, const int32_t* blocksize, uint8_t* raw,
          const int64_t* raw_off, int32_t* status)
{
    return emu_decompress_batch(n, comp, comp_off, nbytes, blocksize, raw, raw_off, status);
}

}  // namespace

extern "C" {

int cimg_decompress_windows_device(cimg_engine*, int32_t nchunks, const void* d_comp, const int64_t* comp_off, const int32_t* comp_size,
                                   const int32_t* nbytes, const int32_t* blocksize, int32_t typesize, int32_t nwindows, const cimg_window* w,
                                   void* d_out, int32_t* status)
{
    static_assert(sizeof(cimg_window) == sizeof(WindowSpec), "cimg_window != WindowSpec");
    return emu_windows_device(whole, nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows,
                              reinterpret_cast<const WindowSpec*>(w), (uint8_t*)d_out, status, &g_stats);
}

int cimg_decompress_windows_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off, const int32_t* comp_size,
                                 int32_t nwindows, const cimg_window* w, void* h_out, int32_t* status)
{
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    return emu_windows_host(whole, nchunks, (const uint8_t*)h_comp, comp_off, comp_size, nwindows, reinterpret_cast<const WindowSpec*>(w),
                            (uint8_t*)h_out, status, &g_stats);
}

void cimg_engine_window_stats(cimg_engine*, int64_t* blocks_decoded, int64_t* chunks_whole, int64_t* comp_bytes_uploaded)
{
    if (blocks_decoded) *blocks_decoded = g_stats.blocks_decoded;
    if (chunks_whole) *chunks_whole = g_stats.chunks_whole;
    if (comp_bytes_uploaded) *comp_bytes_uploaded = g_stats.comp_bytes_uploaded;
}

}  // extern "C"
