// tests/emu/window_write_emu.cpp -- TEST INFRASTRUCTURE: window writes (csrc/update_plan.h, csrc/update_kernel.h) on the host lane
// emulator.  Linked with emu.cpp and wide_emu.cpp (tests/test_emu_window_writes.py builds the three into one library): chunks decoded
// whole go through wemu_decompress_batch and chunks compressed whole through wemu_compress_batch, which route them the way engine.hip
// does (normal blocks: emu.cpp; blocks beyond LDS: the wide kernels).
#define CIMG_EMULATE 1
#include "window_write_env.h"

using namespace cimg;

extern "C" {

int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
int wemu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                        const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);

static UpdateStats g_wwemu_stats;

static HostCParams host_params(const void* p)
{
    HostCParams h;
    static_assert(sizeof(HostCParams) == 32, "HostCParams != cimg_cparams");
    memcpy(&h, p, sizeof h);
    return h;
}

// = cimg_update_windows_device
int wwemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                        const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const WindowSpec* w,
                        const uint8_t* src, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    return emu_update_device(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, nbytes,
                             blocksize, destsize, nwindows, w, src, newbuf, new_off, new_cbytes, status, &g_wwemu_stats);
}

// = cimg_update_windows_host (alloc: malloc; the caller frees with wwemu_free)
static void* wwemu_alloc(void*, size_t n) { return malloc(n); }
int wwemu_update_host(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                      const int32_t* destsize, int nwindows, const WindowSpec* w, const uint8_t* src, void** new_chunks,
                      int32_t* new_cbytes, int32_t* status)
{
    return emu_update_host(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, destsize,
                           nwindows, w, src, wwemu_alloc, nullptr, new_chunks, new_cbytes, status, &g_wwemu_stats);
}
void wwemu_free(void* m) { free(m); }

// = cimg_engine_update_stats
void wwemu_update_stats(int64_t* out)
{
    out[0] = g_wwemu_stats.blocks_decoded; out[1] = g_wwemu_stats.blocks_encoded; out[2] = g_wwemu_stats.chunks_whole;
    out[3] = g_wwemu_stats.bytes_uploaded;
}

}  // extern "C"
