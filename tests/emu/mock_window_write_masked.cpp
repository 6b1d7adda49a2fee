// tests/emu/mock_window_write_masked.cpp -- TEST INFRASTRUCTURE: the masked / constant window-write entry points of
// include/cimg_hip.h (cimg_update_windows_masked_device / _host) on the host lane emulator, for the mock build of the Python module
// and the mirror tests.  This file INCLUDES mock_window_write_typed.cpp (which includes the strided and the plain write mocks) -- one
// translation unit, so that the masked calls fill the stats its cimg_engine_update_stats reports -- and is compiled in its place
// (compressed-image_amd/python/Makefile, `mock`): the outermost write mock.  mock_masked_update_calls() is the number of masked
// write calls.
#include "mock_window_write_typed.cpp"
#include "window_write_masked_env.h"

namespace {
int64_t g_masked_update_calls = 0;
}

extern "C" {

int cimg_update_windows_masked_device(cimg_engine*, const cimg_cparams* p, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                      const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize,
                                      int32_t nwindows, const cimg_window_masked* w, const void* d_src, const void* d_mask, void* d_new,
                                      const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    g_masked_update_calls++;
    return emu_update_masked_device(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes,
                                    blocksize, destsize, nwindows, reinterpret_cast<const MaskedWindowSpec*>(w), (const uint8_t*)d_src,
                                    (const uint8_t*)d_mask, (uint8_t*)d_new, new_off, new_cbytes, status, &g_stats);
}

int cimg_update_windows_masked_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                    const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window_masked* w,
                                    const void* h_src, const void* h_mask, cimg_alloc_fn alloc, void* user, void** new_chunks,
                                    int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    g_masked_update_calls++;
    return emu_update_masked_host(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)h_comp, comp_off, comp_size, destsize,
                                  nwindows, reinterpret_cast<const MaskedWindowSpec*>(w), (const uint8_t*)h_src, (const uint8_t*)h_mask, alloc,
                                  user, new_chunks, new_cbytes, status, &g_stats);
}

__attribute__((visibility("default"))) int64_t mock_masked_update_calls(void) { return g_masked_update_calls; }

}  // extern "C"
