// tests/emu/mock_window_strided.cpp -- TEST INFRASTRUCTURE: the strided window entry points of include/cimg_hip.h
// (cimg_decompress_windows_strided_device / _host) on the host lane emulator, for the mock build of the Python module.  This file
// INCLUDES mock_window.cpp -- one translation unit, so that the strided calls fill the stats its cimg_engine_window_stats reports
// -- and is compiled in its place (compressed-image_amd/python/Makefile, `mock`).
#include "mock_window.cpp"
#include "window_strided_env.h"

extern "C" {

int cimg_decompress_windows_strided_device(cimg_engine*, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                           const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, int32_t typesize,
                                           int32_t nwindows, const cimg_window_strided* w, void* d_out, int32_t* status)
{
    static_assert(sizeof(cimg_window_strided) == sizeof(StridedWindowSpec), "cimg_window_strided != StridedWindowSpec");
    return emu_windows_strided_device(whole, nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows,
                                      reinterpret_cast<const StridedWindowSpec*>(w), (uint8_t*)d_out, status, &g_stats);
}

int cimg_decompress_windows_strided_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                         const int32_t* comp_size, int32_t nwindows, const cimg_window_strided* w, void* h_out,
                                         int32_t* status)
{
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    return emu_windows_strided_host(whole, nchunks, (const uint8_t*)h_comp, comp_off, comp_size, nwindows,
                                    reinterpret_cast<const StridedWindowSpec*>(w), (uint8_t*)h_out, status, &g_stats);
}

}  // extern "C"
