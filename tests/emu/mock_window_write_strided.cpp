// tests/emu/mock_window_write_strided.cpp -- TEST INFRASTRUCTURE: the strided window-write entry points of include/cimg_hip.h
// (cimg_update_windows_strided_device / _host) on the host lane emulator, for the mock build of the Python module.  This file
// INCLUDES mock_window_write.cpp -- one translation unit, so that the strided calls fill the stats its cimg_engine_update_stats
// reports -- and is compiled in its place (compressed-image_amd/python/Makefile, `mock`).
#include "mock_window_write.cpp"
#include "window_write_strided_env.h"

extern "C" {

int cimg_update_windows_strided_device(cimg_engine*, const cimg_cparams* p, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                       const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize,
                                       int32_t nwindows, const cimg_window_strided* w, const void* d_src, void* d_new,
                                       const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    return emu_update_strided_device(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes,
                                     blocksize, destsize, nwindows, reinterpret_cast<const StridedWindowSpec*>(w), (const uint8_t*)d_src,
                                     (uint8_t*)d_new, new_off, new_cbytes, status, &g_stats);
}

int cimg_update_windows_strided_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                     const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window_strided* w,
                                     const void* h_src, cimg_alloc_fn alloc, void* user, void** new_chunks, int32_t* new_cbytes,
                                     int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    return emu_update_strided_host(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)h_comp, comp_off, comp_size, destsize,
                                   nwindows, reinterpret_cast<const StridedWindowSpec*>(w), (const uint8_t*)h_src, alloc, user, new_chunks,
                                   new_cbytes, status, &g_stats);
}

}  // extern "C"
