// tests/emu/mock_window_write_typed.cpp -- TEST INFRASTRUCTURE: the typed window-write entry point of include/cimg_hip.h
// (cimg_update_windows_typed_device) on the host lane emulator, for the mock build of the Python module and the mirror tests.  This
// file INCLUDES mock_window_write_strided.cpp (which includes the plain write mock) -- one translation unit, so that the typed call
// fills the stats its cimg_engine_update_stats reports -- and is compiled in its place (compressed-image_amd/python/Makefile, `mock`),
// with -ffp-contract=off.  mock_typed_update_calls() is the number of typed write calls.
#include "mock_window_write_strided.cpp"
#include "window_write_typed_env.h"

namespace {
int64_t g_typed_update_calls = 0;
}

extern "C" {

int cimg_update_windows_typed_device(cimg_engine*, const cimg_cparams* p, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                     const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize,
                                     int32_t nwindows, const cimg_window_typed* w, const void* d_src, void* d_new,
                                     const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    g_typed_update_calls++;
    return emu_update_typed_device(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes,
                                   blocksize, destsize, nwindows, reinterpret_cast<const TypedWindowSpec*>(w), (const uint8_t*)d_src,
                                   (uint8_t*)d_new, new_off, new_cbytes, status, &g_stats);
}

__attribute__((visibility("default"))) int64_t mock_typed_update_calls(void) { return g_typed_update_calls; }

}  // extern "C"
