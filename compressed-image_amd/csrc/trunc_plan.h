// trunc_plan.h -- blosc2's trunc-prec filter (BLOSC_TRUNC_PREC = 4): which cparams name it, which are valid, and the mask it stands for.
// Pure host C++, shared by the engine (engine.hip: the pass in front of every compress) and the emulator (tests/emu/trunc_emu.cpp).
//
// The filter zeroes the low mantissa bits of every float before the other filters and the codec see the pixels; undoing it is a no-op
// (the truncated values ARE the stored values).  [UPSTREAM-RECALL] (c-blosc2 trunc-prec.c):
//   - it sits in filters[4], with filters[0..3] == 0 and filters[5] one of none / shuffle / bitshuffle; filters_meta[4] is an int8 m
//   - mantissa width M: 23 (typesize 4), 52 (typesize 8); typesize 2 is taken as IEEE binary16, M = 10 (an extension on the write side)
//   - zeroed = M - m for m >= 0 (m = mantissa bits KEPT), -m for m < 0 (bits ZEROED); valid iff |m| <= M and zeroed < M
//   - every whole element, as a little-endian unsigned integer, is ANDed with ~((1 << zeroed) - 1); sign and exponent are untouched
// Any other placement of the filter is what plan.h's single_filter says it is (BLOSC2_ERROR_CODEC_SUPPORT).
#pragma once
#include "codec_types.h"
#include <stdint.h>

namespace cimg {

// does slot 4 (and nothing in front of it) name the filter?  (slot 5 is single_filter's business)
inline bool trunc_named(const uint8_t filters[6])
{
    return filters[4] == FILTER_TRUNC_PREC && filters[0] == 0 && filters[1] == 0 && filters[2] == 0 && filters[3] == 0;
}

inline int trunc_mantissa_width(int typesize)
{
    return typesize == 2 ? 10 : typesize == 4 ? 23 : typesize == 8 ? 52 : 0;
}

// 0 and *zeroed (0 .. M - 1), or ERR_INVALID_PARAM
inline int trunc_zeroed_bits(int typesize, int meta, int* zeroed)
{
    const int M = trunc_mantissa_width(typesize);
    if (M == 0) return ERR_INVALID_PARAM;
    const int m = (int)(int8_t)(meta & 0xFF);
    if (m > M || m < -M) return ERR_INVALID_PARAM;
    const int z = m >= 0 ? M - m : -m;
    if (z >= M) return ERR_INVALID_PARAM;
    *zeroed = z;
    return 0;
}

// the element mask, replicated over 64 bits (typesize 2: four times, 4: twice): byte k of a piece is ANDed with byte k % typesize of it
inline uint64_t trunc_mask64(int typesize, int zeroed)
{
    const uint64_t keep = ~((1ull << zeroed) - 1);
    if (typesize == 8) return keep;
    if (typesize == 4) { const uint64_t m = keep & 0xffffffffull; return m | (m << 32); }
    const uint64_t m = keep & 0xffffull;
    return m | (m << 16) | (m << 32) | (m << 48);
}

// what a compress call does about the filter: 0 = the cparams do not name it (nothing changes), 1 = named and valid (*mask64 set),
// < 0 = ERR_INVALID_PARAM.  A misplaced filter is 0 here: single_filter refuses it as it always did.
inline int trunc_from_cparams(int typesize, const uint8_t filters[6], const uint8_t filters_meta[6], uint64_t* mask64)
{
    if (!trunc_named(filters)) return 0;
    if (filters[5] > FILTER_BITSHUFFLE) return 0;            // (refused by single_filter)
    int z = 0;
    const int rc = trunc_zeroed_bits(typesize, filters_meta[4], &z);
    if (rc < 0) return rc;
    *mask64 = trunc_mask64(typesize, z);
    return 1;
}

}  // namespace cimg
