// chunk_plan.h -- host-side chunk geometry: what blosc2_compress_ctx derives from (cparams, srcsize)
// before it touches a byte (oracle/chunk.c: orc_chunk_geometry is the
// checker's copy of the same rules).  Pure C++ with no kernel header behind it: the engine and the emulator reach it through
// plan.h, the blosc2 shim and special_plan.h (which write headers on the host) include it directly.
#pragma once
#include "codec_types.h"
#include "trunc_plan.h"
#include <stdint.h>
#include <vector>

namespace cimg {

struct HostCParams {
    int32_t typesize = 1;
    int32_t clevel = 9;
    int32_t blocksize = 32768;                 // constants.h:11 default
    int32_t compcode = CODEC_LZ4;              // channel.h:101 default
    int32_t splitmode = SPLIT_AUTO;            // wrapper.h:328,353
    uint8_t filters[6] = {0, 0, 0, 0, 0, FILTER_SHUFFLE};   // BLOSC2_CPARAMS_DEFAULTS
    uint8_t filters_meta[6] = {0, 0, 0, 0, 0, 0};
};

inline int compformat_of(int compcode)
{
    switch (compcode) {
    case CODEC_BLOSCLZ: return 0;
    case CODEC_LZ4: case CODEC_LZ4HC: return 1;
    case CODEC_ZLIB: return 3;
    case CODEC_ZSTD: return 4;
    default: return -1;
    }
}

// the single filter the kernels implement: one of none/shuffle/bitshuffle, in the last pipeline slot
inline int single_filter(const HostCParams& p, int* filter)
{
    for (int i = 0; i < 5; i++) if (p.filters[i] != 0) return ERR_CODEC_SUPPORT;
    if (p.filters[5] > FILTER_BITSHUFFLE) return ERR_CODEC_SUPPORT;
    *filter = p.filters[5];
    return 0;
}

// trunc-prec in slot 4 (trunc_plan.h).  The planners below plan for pixels as they ARE: parameters that name the filter are refused
// like any filter in slots 0 .. 4 unless the caller says the pass has run over the pixels (`truncated`); then the batch is planned as
// for the same parameters without slot 4, and *trunc carries the two header bytes (CodecParams::trunc).
inline int strip_trunc(const HostCParams& p, bool truncated, HostCParams* q, int32_t* trunc)
{
    *q = p;
    *trunc = 0;
    if (!truncated || !trunc_named(p.filters)) return 0;
    int zeroed = 0;
    const int rc = trunc_zeroed_bits(p.typesize, p.filters_meta[4], &zeroed);
    if (rc < 0) return rc;
    q->filters[4] = 0;
    *trunc = FILTER_TRUNC_PREC | ((int32_t)p.filters_meta[4] << 8);
    return 0;
}

inline bool wants_split(const HostCParams& p, int typesize, int blocksize)
{
    if (p.splitmode == SPLIT_ALWAYS) return true;
    if (p.splitmode == SPLIT_NEVER) return false;
    const bool fast = p.compcode == CODEC_BLOSCLZ || p.compcode == CODEC_LZ4 || (p.compcode == CODEC_ZSTD && p.clevel <= 5);
    bool shuffle = false;
    for (int i = 0; i < 6; i++) shuffle |= p.filters[i] == FILTER_SHUFFLE;
    return fast && shuffle && typesize <= MAX_STREAMS && blocksize / typesize >= MIN_BUFFERSIZE;
}

// fills everything in `d` except raw_off / comp_off / blk0; returns 0 or a blosc2 error code
inline int plan_chunk(const HostCParams& p, int32_t nbytes, int32_t destsize, ChunkDesc* d)
{
    *d = ChunkDesc{};
    if (nbytes < 0) return ERR_MAX_BUFSIZE;
    if (destsize < HEADER_LEN) return ERR_MAX_BUFSIZE;
    if (p.clevel < 0 || p.clevel > 9) return ERR_CODEC_PARAM;
    if (compformat_of(p.compcode) < 0) return ERR_CODEC_SUPPORT;
    int ts = p.typesize;
    if (ts <= 0) return ERR_INVALID_PARAM;
    if (ts > 255) ts = 1;
    int bs;
    if (nbytes < ts) {
        bs = 1;
    } else {
        if (p.blocksize <= 0) return ERR_INVALID_PARAM;     // automatic block size is not on the path
        bs = p.blocksize;
        if (bs < MIN_BUFFERSIZE) bs = MIN_BUFFERSIZE;       // a forced block size below 32 bytes is raised to 32 (upstream compute_blocksize, recalled)
        if (bs > nbytes) bs = nbytes;
        if (bs > ts) bs = bs / ts * ts;
    }
    d->nbytes = nbytes;
    d->destsize = destsize;
    d->blocksize = bs;
    d->nblocks = nbytes / bs;
    d->leftover = nbytes % bs;
    if (d->leftover) d->nblocks++;
    d->memcpyed = (p.clevel == 0 || nbytes < MIN_BUFFERSIZE) ? 1 : 0;
    d->flags = FLAG_SHUFFLE | FLAG_BITSHUFFLE;
    // one rule for the header's flags byte: the dont-split bit and the codec format are set whether or not the chunk is
    // memcpyed up front (oracle/chunk.c: orc_chunk_geometry says where that comes from)
    const bool split = wants_split(p, ts, bs);
    if (!split) d->flags |= FLAG_DONT_SPLIT;
    d->flags |= compformat_of(p.compcode) << 5;
    if (d->memcpyed) d->flags |= FLAG_MEMCPYED;
    else d->split = split ? 1 : 0;
    if (d->split) d->nstreams = d->leftover ? (d->nblocks - 1) * ts + 1 : d->nblocks * ts;
    else d->nstreams = d->nblocks;
    return 0;
}

}  // namespace cimg
