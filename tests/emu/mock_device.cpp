// tests/emu/mock_device.cpp -- TEST INFRASTRUCTURE: the device-resident entry points of include/cimg_hip.h that the device objects
// (compressed/device_channel.h, device_image.h) need and libcimg_hip_mock.so lacks, on the host lane emulator: device memory is
// host memory (as in mock_cabi.cpp), the pack and interleave launches are the kernel bodies of csrc/ run tile by tile
// (pack_env.h), compress / decode go through emu.cpp's batch functions.  Compiled beside mock_window.cpp / mock_window_write.cpp
// into the mock build of the Python module (compressed-image_amd/python/Makefile, `mock`) and into the C++ test of the device objects.
#define CIMG_EMULATE 1
#include "pack_env.h"
#include "../../include/cimg_hip.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cimg;

extern "C" int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes,
                                    const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);

// mock_cabi.cpp: the sizes of the batch staged by the last _begin -- of the host kind or of the packed kind, which share the staging
// area as they do in the engine -- or -12 where none of n chunks is waiting
extern "C" int cimg_mock_staged_sizes(cimg_engine* e, int32_t n, int32_t* len);

extern "C" {

void* cimg_device_malloc(cimg_engine*, size_t bytes) { return malloc(bytes ? bytes : 16); }
void cimg_device_free(cimg_engine*, void* p) { free(p); }
int cimg_memcpy_h2d(cimg_engine*, void* d, const void* h, size_t n) { if (n) memcpy(d, h, n); return 0; }
int cimg_memcpy_d2h(cimg_engine*, void* h, const void* d, size_t n) { if (n) memcpy(h, d, n); return 0; }
int cimg_engine_wait_stream(cimg_engine*, void*) { return 0; }
// (no way to tell here whose memory an address is: only what cannot be any memory is refused)
int cimg_device_range_check(cimg_engine*, const void* p, size_t bytes) { return p && (uintptr_t)p + bytes >= (uintptr_t)p ? 0 : -12; }

int cimg_decompress_batch_device_sized(cimg_engine*, int32_t n, const void* d_comp, const int64_t* comp_off, const int32_t* comp_size,
                                       const int32_t* nbytes, const int32_t* blocksize, void* d_raw, const int64_t* raw_off, int32_t* status)
{
    if (n <= 0) return 0;
    if (comp_size)
        for (int i = 0; i < n; i++) {
            int32_t cb = 0;
            if (comp_size[i] >= 16) memcpy(&cb, (const uint8_t*)d_comp + comp_off[i] + 12, 4);
            if (comp_size[i] < 32 || cb > comp_size[i]) { if (status) status[i] = -5; return -5; }
        }
    const int rc = emu_decompress_batch(n, (const uint8_t*)d_comp, comp_off, nbytes, blocksize, (uint8_t*)d_raw, raw_off, status);
    if (rc < 0) return rc;
    for (int i = 0; i < n; i++) if (status[i] < 0) return status[i];
    return 0;
}
int cimg_decompress_batch_device(cimg_engine* e, int32_t n, const void* d_comp, const int64_t* comp_off, const int32_t* nbytes,
                                 const int32_t* blocksize, void* d_raw, const int64_t* raw_off, int32_t* status)
{
    return cimg_decompress_batch_device_sized(e, n, d_comp, comp_off, nullptr, nbytes, blocksize, d_raw, raw_off, status);
}

int cimg_compress_batch_device_packed_begin(cimg_engine* e, const cimg_cparams* p, int32_t n, const void* d_raw, const int64_t* raw_off,
                                            const int32_t* nbytes, const int32_t* destsize, int32_t* cbytes)
{
    // (device memory is host memory: the host _begin stages the batch, and its bookkeeping says when a pending fetch has been voided)
    return cimg_compress_batch_host_begin(e, p, n, d_raw, raw_off, nbytes, destsize, cbytes);
}

int cimg_pack_chunks_device(cimg_engine*, int32_t n, const void* const* d_src, const int32_t* bytes, void* d_dst, const int64_t* dst_off)
{
    return emu_pack_chunks(n, d_src, bytes, (uint8_t*)d_dst, dst_off);
}

int cimg_compress_batch_device_packed_fetch(cimg_engine* e, int32_t n, void* d_dst, const int64_t* dst_off)
{
    if (n <= 0) return 0;
    std::vector<int32_t> len((size_t)n);
    if (cimg_mock_staged_sizes(e, n, len.data())) return -12;
    // out of the staging area (an error if another batch call has reused it since _begin), then through the pack kernel's body
    std::vector<int64_t> off((size_t)n);
    int64_t total = 0;
    for (int i = 0; i < n; i++) { if (len[(size_t)i] < 0) len[(size_t)i] = 0; off[(size_t)i] = total; total += ((int64_t)len[(size_t)i] + 63) & ~63ll; }
    std::vector<uint8_t> tmp((size_t)total + 64);
    const int rc = cimg_compress_batch_host_fetch(e, n, tmp.data(), off.data());
    if (rc) return rc;
    std::vector<const void*> src((size_t)n);
    for (int i = 0; i < n; i++) src[(size_t)i] = tmp.data() + off[(size_t)i];
    return emu_pack_chunks(n, src.data(), len.data(), (uint8_t*)d_dst, dst_off);
}

int cimg_interleave_device(cimg_engine*, const void* d_planar, int64_t plane_stride, int32_t nch, int32_t ts, int64_t npixels, void* d_interleaved)
{
    if ((((uintptr_t)d_planar) | ((uintptr_t)d_interleaved)) & 15) return -12;
    return emu_interleave((const uint8_t*)d_planar, plane_stride, nch, ts, npixels, (uint8_t*)d_interleaved);
}

}  // extern "C"
