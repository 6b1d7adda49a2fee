// blosc2_getitem.cpp -- blosc2_getitem_ctx (include/blosc2.h): items [start, start + nitems) of one chunk through the engine's window
// call, which decodes only the blocks that hold them.  Kept apart from blosc2_shim.cpp because that file is also linked into the
// emulator-backed mock library, which has no window entry points; this one goes into libcimg_hip.so only.
#include <cstdint>

#include "../../include/blosc2.h"
#include "../../include/cimg_hip.h"
#include "blosc2_context.h"

extern "C" int blosc2_getitem_ctx(blosc2_context* context, const void* src, int32_t srcsize, int start, int nitems, void* dest,
                                  int32_t destsize)
{
    if (!context || !src || !dest) return BLOSC2_ERROR_NULL_POINTER;
    if (context->compress) return BLOSC2_ERROR_INVALID_PARAM;
    if (context->unsupported_params) return BLOSC2_ERROR_CODEC_SUPPORT;
    if (srcsize < BLOSC_MIN_HEADER_LENGTH) return BLOSC2_ERROR_READ_BUFFER;
    int32_t nbytes, cbytes, blocksize;
    int rc = blosc2_cbuffer_sizes(src, &nbytes, &cbytes, &blocksize);
    if (rc < 0) return rc;
    if (cbytes > srcsize) return BLOSC2_ERROR_READ_BUFFER;
    const int64_t ts = static_cast<const uint8_t*>(src)[3];
    if (ts == 0) return BLOSC2_ERROR_INVALID_HEADER;
    if (start < 0 || nitems < 0 || ((int64_t)start + nitems) * ts > nbytes) return BLOSC2_ERROR_INVALID_PARAM;
    if ((int64_t)nitems * ts > destsize) return BLOSC2_ERROR_WRITE_BUFFER;
    if (nitems == 0) return 0;
    cimg_engine* e = cimg_shared_engine();
    if (!e) return BLOSC2_ERROR_FAILURE;
    const int64_t zero = 0;
    cimg_window w = {0, 1, start, nitems, nitems, 1, 0, (int64_t)nitems * ts};
    int32_t status = 0;
    rc = cimg_decompress_windows_host(e, 1, src, &zero, &srcsize, 1, &w, dest, &status);
    return rc < 0 ? rc : (int)(nitems * ts);
}
