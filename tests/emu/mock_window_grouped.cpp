// tests/emu/mock_window_grouped.cpp -- TEST INFRASTRUCTURE: the grouped window entry points of include/cimg_hip.h
// (cimg_decompress_windows_grouped_device / _host) on the host lane emulator, for the mock build of the Python module.  This file
// INCLUDES mock_window_strided.cpp (which includes mock_window.cpp) -- one translation unit, so that the grouped calls fill the
// stats its cimg_engine_window_stats reports -- and is compiled in its place (compressed-image_amd/python/Makefile, `mock`).
// It also counts the window read calls, for the tests that pin "one engine call per get_regions": mock_window_calls() is the number
// of calls of all six read entry points, mock_grouped_window_calls() that of the two grouped ones, so a get_regions that made one
// grouped call and a plain or strided call beside it would be seen.  The four entry points of the two included files are compiled
// under other names (the macros below) and exported here as wrappers that count.
#define cimg_decompress_windows_device mock_plain_windows_device
#define cimg_decompress_windows_host mock_plain_windows_host
#define cimg_decompress_windows_strided_device mock_strided_windows_device
#define cimg_decompress_windows_strided_host mock_strided_windows_host
#include "mock_window_strided.cpp"
#undef cimg_decompress_windows_device
#undef cimg_decompress_windows_host
#undef cimg_decompress_windows_strided_device
#undef cimg_decompress_windows_strided_host
#include "window_grouped_env.h"

#define MOCK_EXPORT __attribute__((visibility("default")))

namespace {
int64_t g_window_calls = 0, g_grouped_calls = 0;
}

extern "C" {

MOCK_EXPORT int cimg_decompress_windows_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                               const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, int32_t typesize,
                                               int32_t nwindows, const cimg_window* w, void* d_out, int32_t* status)
{
    g_window_calls++;
    return mock_plain_windows_device(e, nchunks, d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w, d_out, status);
}

MOCK_EXPORT int cimg_decompress_windows_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                             const int32_t* comp_size, int32_t nwindows, const cimg_window* w, void* h_out, int32_t* status)
{
    g_window_calls++;
    return mock_plain_windows_host(e, nchunks, h_comp, comp_off, comp_size, nwindows, w, h_out, status);
}

MOCK_EXPORT int cimg_decompress_windows_strided_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                                       const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                                       int32_t typesize, int32_t nwindows, const cimg_window_strided* w, void* d_out,
                                                       int32_t* status)
{
    g_window_calls++;
    return mock_strided_windows_device(e, nchunks, d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w, d_out, status);
}

MOCK_EXPORT int cimg_decompress_windows_strided_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                                     const int32_t* comp_size, int32_t nwindows, const cimg_window_strided* w, void* h_out,
                                                     int32_t* status)
{
    g_window_calls++;
    return mock_strided_windows_host(e, nchunks, h_comp, comp_off, comp_size, nwindows, w, h_out, status);
}

MOCK_EXPORT int cimg_decompress_windows_grouped_device(cimg_engine*, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                                       const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                                       int32_t typesize, int32_t nwindows, const cimg_window_strided* w, void* d_out,
                                                       int32_t* status)
{
    g_window_calls++;
    g_grouped_calls++;
    return emu_windows_grouped_device(whole, nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows,
                                      reinterpret_cast<const StridedWindowSpec*>(w), (uint8_t*)d_out, status, &g_stats);
}

MOCK_EXPORT int cimg_decompress_windows_grouped_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                                     const int32_t* comp_size, int32_t nwindows, const cimg_window_strided* w, void* h_out,
                                                     int32_t* status)
{
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    g_window_calls++;
    g_grouped_calls++;
    return emu_windows_grouped_host(whole, nchunks, (const uint8_t*)h_comp, comp_off, comp_size, nwindows,
                                    reinterpret_cast<const StridedWindowSpec*>(w), (uint8_t*)h_out, status, &g_stats);
}

// window read calls of every kind, and the grouped ones among them, since the library was loaded: exported symbols, which the
// tests look up in the loaded mock module themselves (the module has no hook for them)
MOCK_EXPORT int64_t mock_window_calls(void) { return g_window_calls; }
MOCK_EXPORT int64_t mock_grouped_window_calls(void) { return g_grouped_calls; }

}  // extern "C"
