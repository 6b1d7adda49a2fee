// special_plan.h -- blosc2's special-value chunks: the chunks that hold a header and no pixel stream.  One set of rules for the
// kernels (decode_kernel.h, wide_kernel.h, window_kernel.h), the blosc2 shim (blosc2_chunk_zeros / _nans / _repeatval / _uninit)
// and the emulator, as trunc_plan.h is for trunc-prec.
//
// [UPSTREAM-RECALL] (c-blosc2 blosc2.c: blosc2_chunk_zeros & co., the special-value branch of blosc_run_decompression_with_context;
// DESIGN.md section 2).  Bits 4-6 of header byte 31 (blosc2_flags) name the kind:
//   1 SPECIAL_ZERO    32 bytes            every byte 0
//   2 SPECIAL_NAN     32 bytes            every whole element a quiet NaN: 0x7FC00000 (typesize 4), 0x7FF8000000000000 (typesize 8);
//                                         nbytes % typesize trailing bytes are not written; any other typesize is ERR_DATA
//   3 SPECIAL_VALUE   32 + typesize       byte k of the chunk is value[k % typesize], the value being the typesize bytes behind the
//                                         header; valid iff cbytes >= 32 + typesize and nbytes % typesize == 0, else ERR_DATA
//   4 SPECIAL_UNINIT  32 bytes            values unspecified by the format; THIS library reads them as zeros on every route (a host
//                                         call's destination is filled from engine staging, whose old contents must never show)
//   5 .. 7                                ERR_DATA
// The field is decided behind the version / nbytes / blocksize / cbytes / extended-header checks and BEFORE the memcpyed flag and
// the codec format: a special chunk whose flags name zstd never reaches the zstd launches.
// A block that starts at chunk offset j * blocksize starts at element phase (j * blocksize) % typesize: nonzero only where a
// hand-set block size is no multiple of the typesize.
#pragma once
#include "chunk_plan.h"
#include <stdint.h>
#include <string.h>

#if defined(__HIP__) && !defined(CIMG_EMULATE)
#define CIMG_SPECIAL_FN __host__ __device__ inline
#else
#define CIMG_SPECIAL_FN inline
#endif

namespace cimg {

// what a reader does with the special field of a header that passed the checks in front of it: 0 or ERR_DATA
CIMG_SPECIAL_FN int special_check(int special, int typesize, int nbytes, int cbytes)
{
    if (special == 0 || special == SPECIAL_ZERO || special == SPECIAL_UNINIT) return 0;
    if (typesize <= 0) return ERR_DATA;
    if (special == SPECIAL_VALUE) return (cbytes >= HEADER_LEN + typesize && nbytes % typesize == 0) ? 0 : ERR_DATA;
    if (special == SPECIAL_NAN) return (typesize == 4 || typesize == 8) ? 0 : ERR_DATA;
    return ERR_DATA;
}

// byte idx (0 .. typesize - 1) of the quiet NaN of a 4- or 8-byte float, little-endian
CIMG_SPECIAL_FN uint32_t special_nan_byte(int typesize, int idx)
{
    return idx == typesize - 1 ? 0x7Fu : idx == typesize - 2 ? (typesize == 4 ? 0xC0u : 0xF8u) : 0u;
}

// The repeating pattern of a value or NaN chunk: `value` points at the typesize bytes behind the header, or is null for the NaN.
struct SpecialPattern {
    const uint8_t* value;
    int ts;
    CIMG_SPECIAL_FN uint32_t at(int idx) const { return value ? (uint32_t)value[idx] : special_nan_byte(ts, idx); }
};

// the bytes of a chunk the pattern covers (a NaN chunk leaves nbytes % typesize trailing bytes alone)
CIMG_SPECIAL_FN int special_covered(int nbytes, int typesize) { return nbytes - nbytes % typesize; }

// element phase of the block that starts at chunk offset j * blocksize
CIMG_SPECIAL_FN int special_phase(int j, int blocksize, int typesize) { return (int)(((int64_t)j * blocksize) % typesize); }

// ---- writers (host only) ----------------------------------------------------------------------------------------------------------
// The header LayoutChunk::write_header (assemble_kernel.h) writes for a special-zero chunk of the same cparams, with the special field
// `code`, cbytes = 32 (+ typesize for a value chunk, whose value follows the header), the block size plan_chunk derives and the
// trunc-prec bytes.  With trunc-prec named, a stored value is the truncated one.  Returns the chunk's size or a negative code:
// ERR_DATA for a destination that cannot hold the chunk and for nbytes that is no multiple of the typesize (c-blosc2's codes, as
// recalled), ERR_INVALID_PARAM / ERR_CODEC_SUPPORT / ERR_CODEC_PARAM for cparams plan_chunk or the filter rules refuse.
inline int special_chunk_write(const HostCParams& p_in, int code, int32_t nbytes, const void* value, void* dest, int32_t destsize)
{
    if (!dest || (code == SPECIAL_VALUE && !value)) return ERR_INVALID_PARAM;
    if (code < SPECIAL_ZERO || code > SPECIAL_UNINIT) return ERR_INVALID_PARAM;
    HostCParams p;
    int32_t trunc = 0;
    int filter = 0;
    int rc = strip_trunc(p_in, true, &p, &trunc);
    if (rc < 0) return rc;
    if ((rc = single_filter(p, &filter)) < 0) return rc;
    if (p.typesize <= 0) return ERR_INVALID_PARAM;
    const int ts = p.typesize > 255 ? 1 : p.typesize;
    const int32_t cbytes = HEADER_LEN + (code == SPECIAL_VALUE ? ts : 0);
    if (destsize < cbytes) return ERR_DATA;
    if (nbytes < 0 || nbytes % ts) return ERR_DATA;
    if (code == SPECIAL_NAN && ts != 4 && ts != 8) return ERR_DATA;
    ChunkDesc d;
    if ((rc = plan_chunk(p, nbytes, destsize, &d)) < 0) return rc;
    uint8_t* c = static_cast<uint8_t*>(dest);
    memset(c, 0, (size_t)HEADER_LEN);
    c[0] = 5;
    c[1] = 1;
    c[OFF_FLAGS] = (uint8_t)(d.flags & ~FLAG_MEMCPYED);
    c[OFF_TYPESIZE] = (uint8_t)ts;
    memcpy(c + OFF_NBYTES, &d.nbytes, 4);
    memcpy(c + OFF_BLOCKSIZE, &d.blocksize, 4);
    memcpy(c + OFF_CBYTES, &cbytes, 4);
    c[OFF_FILTERS + 4] = (uint8_t)(trunc & 0xFF);
    c[OFF_FILTERS_META + 4] = (uint8_t)((trunc >> 8) & 0xFF);
    c[OFF_FILTERS + 5] = (uint8_t)filter;
    c[OFF_COMPCODE] = (uint8_t)p.compcode;
    c[OFF_BLOSC2_FLAGS] = (uint8_t)(code << 4);
    if (code == SPECIAL_VALUE) {
        memcpy(c + HEADER_LEN, value, (size_t)ts);
        uint64_t mask64 = 0;
        if (trunc && trunc_from_cparams(ts, p_in.filters, p_in.filters_meta, &mask64) == 1)
            for (int k = 0; k < ts; k++) c[HEADER_LEN + k] &= (uint8_t)(mask64 >> (8 * k));      // (typesize 2, 4, 8: the mask repeats every typesize bytes)
    }
    return cbytes;
}

}  // namespace cimg
