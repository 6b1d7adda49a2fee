// tests/emu/mock_window_typed.cpp -- TEST INFRASTRUCTURE: the typed window entry point of include/cimg_hip.h
// (cimg_decompress_windows_typed_device) on the host lane emulator, for the mock build of the Python module and the mirror tests.
// This file INCLUDES mock_window_grouped.cpp (which includes the strided and the plain mocks) -- one translation unit, so that the
// typed call fills the stats its cimg_engine_window_stats reports and counts among its window calls -- and is compiled in its place
// (compressed-image_amd/python/Makefile, `mock`), with -ffp-contract=off.  mock_typed_window_calls() is the number of typed calls.
#include "mock_window_grouped.cpp"
#include "window_typed_env.h"

namespace {
int64_t g_typed_calls = 0;
}

extern "C" {

MOCK_EXPORT int cimg_decompress_windows_typed_device(cimg_engine*, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                                     const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                                     int32_t typesize, int32_t nwindows, const cimg_window_typed* w, void* d_out,
                                                     int32_t* status)
{
    static_assert(sizeof(cimg_window_typed) == sizeof(TypedWindowSpec), "cimg_window_typed != TypedWindowSpec");
    g_window_calls++;
    g_typed_calls++;
    return emu_windows_typed_device(whole, nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows,
                                    reinterpret_cast<const TypedWindowSpec*>(w), (uint8_t*)d_out, status, &g_stats);
}

MOCK_EXPORT int64_t mock_typed_window_calls(void) { return g_typed_calls; }

}  // extern "C"
