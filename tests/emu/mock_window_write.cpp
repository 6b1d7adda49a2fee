// tests/emu/mock_window_write.cpp -- TEST INFRASTRUCTURE: the window-write entry points of include/cimg_hip.h
// (cimg_update_windows_device / _host, cimg_engine_update_stats) on the host lane emulator, for the mock build of the Python module
// (compressed-image_amd/python/Makefile, `mock`): the planner and kernel bodies of csrc/, chunks decoded and compressed whole through
// emu.cpp's batch functions (which libcimg_hip_mock.so exports).  Device pointers are host pointers here, as in mock_cabi.cpp.
#define CIMG_EMULATE 1
#include "window_write_env.h"
#include "../../include/cimg_hip.h"

using namespace cimg;

extern "C" int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes,
                                    const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
extern "C" int emu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                                  uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);

// mock_cabi.cpp: a host-resident window write goes through the engine's staging area, so a batch staged there by a compress _begin is
// void after it (include/cimg_hip.h); the host calls of this file and of the files that include it say so through this
extern "C" void cimg_mock_void_staged(cimg_engine* e);

namespace {

UpdateStats g_stats;

int whole(int n, const uint8_t* comp, const int64_t* comp_off, const int32_t*, const int32_t* nbytes, const int32_t* blocksize, uint8_t* raw,
          const int64_t* raw_off, int32_t* status)
{
    return emu_decompress_batch(n, comp, comp_off, nbytes, blocksize, raw, raw_off, status);
}

HostCParams host_params(const cimg_cparams* p)
{
    static_assert(sizeof(cimg_cparams) == sizeof(HostCParams), "cimg_cparams != HostCParams");
    HostCParams h;
    memcpy(&h, p, sizeof h);
    return h;
}

}  // namespace

extern "C" {

int cimg_update_windows_device(cimg_engine*, const cimg_cparams* p, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                               const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize,
                               int32_t nwindows, const cimg_window* w, const void* d_src, void* d_new, const int64_t* new_off,
                               int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    return emu_update_device(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)d_comp, comp_off, comp_size, nbytes,
                             blocksize, destsize, nwindows, reinterpret_cast<const WindowSpec*>(w), (const uint8_t*)d_src,
                             (uint8_t*)d_new, new_off, new_cbytes, status, &g_stats);
}

int cimg_update_windows_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                             const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window* w,
                             const void* h_src, cimg_alloc_fn alloc, void* user, void** new_chunks, int32_t* new_cbytes, int32_t* status)
{
    if (!p) return ERR_INVALID_PARAM;
    if (nchunks > 0 && nwindows > 0) cimg_mock_void_staged(e);
    return emu_update_host(whole, emu_compress_batch, host_params(p), nchunks, (const uint8_t*)h_comp, comp_off, comp_size, destsize,
                           nwindows, reinterpret_cast<const WindowSpec*>(w), (const uint8_t*)h_src, alloc, user, new_chunks, new_cbytes,
                           status, &g_stats);
}

void cimg_engine_update_stats(cimg_engine*, int64_t* blocks_decoded, int64_t* blocks_encoded, int64_t* chunks_whole, int64_t* bytes_uploaded)
{
    if (blocks_decoded) *blocks_decoded = g_stats.blocks_decoded;
    if (blocks_encoded) *blocks_encoded = g_stats.blocks_encoded;
    if (chunks_whole) *chunks_whole = g_stats.chunks_whole;
    if (bytes_uploaded) *bytes_uploaded = g_stats.bytes_uploaded;
}

}  // extern "C"
