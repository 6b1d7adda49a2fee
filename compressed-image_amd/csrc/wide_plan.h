// wide_plan.h -- the planner of the wide-block kernels (wide_kernel.h).  It is asked only after plan_encode_batch /
// plan_decode_batch (plan.h) refused a batch with ERR_CODEC_SUPPORT, and it takes exactly what those refuse for size alone:
// LZ4 / LZ4HC streams longer than the byU16 encoder's 65 546 bytes, zstd streams longer than ZSTD_ENC_MAX_INPUT, BloscLZ streams
// longer than BLZ_MAX_INPUT (for a caller that has the BloscLZ instance of the wide encoder: `blosclz`), or shuffled blocks whose
// staging exceeds LDS (write), and blocks whose staging exceeds LDS (read; zstd blocks among them go on to the zstd
// read path's walk and cimg_zstd_replay_wide) -- in both cases for blocks up to WIDE_MAX_BLOCK.  Everything else keeps the normal
// planner's answer.  Pure C++, shared by the engine and the emulator tests.
#pragma once
#include "plan.h"
#include "wide_kernel.h"

namespace cimg {

// Write side: the whole batch goes through cimg_encode_wide (every stream, whatever its length) and the two assembly kernels.
// blosclz: the caller launches cimg_encode_wide_blosclz for a BloscLZ plan (the engine does; a caller with the LZ4 instance alone
// leaves it false and BloscLZ stays refused).  Such a batch is planned like an lz4 one: cp.clevel is what the kernel reads.
inline int plan_encode_wide(const HostCParams& p_in, int nchunks, const int64_t* raw_off, const int32_t* nbytes,
                            const int64_t* comp_off, const int32_t* destsize, EncodePlan* plan, bool truncated = false, bool blosclz = false)
{
    plan->descs.resize((size_t)nchunks);
    HostCParams p;
    int filter = 0;
    int rc = strip_trunc(p_in, truncated, &p, &plan->cp.trunc);
    if (rc < 0) return rc;
    rc = single_filter(p, &filter);
    if (rc < 0) return rc;
    if (p.compcode != CODEC_LZ4 && p.compcode != CODEC_LZ4HC && p.compcode != CODEC_ZSTD && !(blosclz && p.compcode == CODEC_BLOSCLZ)) return ERR_CODEC_SUPPORT;   // zlib: not built
    if (filter == FILTER_BITSHUFFLE) return ERR_CODEC_SUPPORT;
    if (p.blocksize <= 0 || p.blocksize > WIDE_MAX_BLOCK) return ERR_CODEC_SUPPORT;      // (automatic block size stays with plan.h)
    CodecParams& cp = plan->cp;
    cp.typesize = p.typesize > 255 ? 1 : p.typesize;
    cp.clevel = p.clevel;
    cp.compcode = p.compcode;
    cp.filter = filter;
    cp.accel = (p.compcode == CODEC_LZ4HC || p.compcode == CODEC_ZSTD) ? 1 : 10 - p.clevel;   // (zstd: zstd_wide_encode has no acceleration)
    cp.max_blocksize = 0;
    cp.streams_per_block = 1;
    int32_t blk = 0;
    plan->lds_split = plan->lds_unsplit = 0;
    for (int i = 0; i < nchunks; i++) {
        ChunkDesc& d = plan->descs[(size_t)i];
        rc = plan_chunk(p, nbytes[i], destsize[i], &d);
        if (rc < 0) return rc;
        if (d.blocksize > WIDE_MAX_BLOCK) return ERR_CODEC_SUPPORT;
        d.raw_off = raw_off[i];
        d.comp_off = comp_off[i];
        d.blk0 = blk;
        d.assemble = 0;                                   // cimg_layout_chunks / cimg_emit_blocks behind the launch
        blk += d.nblocks;
        if (d.blocksize > cp.max_blocksize) cp.max_blocksize = d.blocksize;
        if (d.split) cp.streams_per_block = cp.typesize;
    }
    plan->total_blocks = blk;
    plan->uniform_nblocks = uniform_blocks(plan->descs);
    cp.slot_bytes = (cp.max_blocksize + 63) & ~63;
    return 0;
}

// Read side: chunks whose blocks fit the normal kernels' LDS stay with them (`normal`: their indices, planned by
// plan_decode_batch on that subset); the others (`wide`) are planned here for cimg_decode_wide.  slot_bytes: the
// scratch one workgroup of that launch stages a block in.
struct WideDecodePlan {
    std::vector<int> normal, wide;
    DecodePlan plan;           // over the wide chunks, in the order of `wide`
    int32_t slot_bytes = 0;
};

inline bool decode_is_wide(int blocksize) { return decode_lds_bound(blocksize) > MAX_LDS_BYTES; }

// The batch arrays of the listed chunks, in the order of the list: what a sub-batch is handed to the batch path with.  Without
// comp_size every cs says 0x7fffffff (the caller chooses between that and a null pointer); without raw_off ro stays empty.
struct SubBatch {
    std::vector<int64_t> co, ro;
    std::vector<int32_t> cs, nb, bs;
    SubBatch(const std::vector<int>& list, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
             const int64_t* raw_off = nullptr)
    {
        for (const int i : list) {
            co.push_back(comp_off[i]); cs.push_back(comp_size ? comp_size[i] : 0x7fffffff); nb.push_back(nbytes[i]); bs.push_back(blocksize[i]);
            if (raw_off) ro.push_back(raw_off[i]);
        }
    }
};

// a sub-batch refused before any of its chunks had a status of its own: the refusal is every listed chunk's
inline void spread_refusal(int rc, size_t n, int32_t* st)
{
    if (rc >= 0) return;
    for (size_t k = 0; k < n; k++) if (st[k] != 0) return;
    for (size_t k = 0; k < n; k++) st[k] = rc;
}

inline int plan_decode_wide(int nchunks, const int64_t* comp_off, const int32_t* nbytes, const int32_t* blocksize,
                            const int64_t* raw_off, WideDecodePlan* wp, const int32_t* comp_size = nullptr)
{
    wp->normal.clear(); wp->wide.clear();
    for (int i = 0; i < nchunks; i++) {
        if (nbytes[i] < 0 || blocksize[i] <= 0 || (nbytes[i] > 0 && blocksize[i] > nbytes[i])) return ERR_INVALID_HEADER;
        if (!decode_is_wide(blocksize[i])) { wp->normal.push_back(i); continue; }
        if (blocksize[i] > WIDE_MAX_BLOCK) return ERR_CODEC_SUPPORT;
        wp->wide.push_back(i);
    }
    if (wp->wide.empty()) return ERR_CODEC_SUPPORT;           // nothing here is wide: the normal planner's refusal stands
    const int nw = (int)wp->wide.size();
    DecodePlan& plan = wp->plan;
    plan.descs.resize((size_t)nw);
    int32_t blk = 0, slot = 0;
    for (int k = 0; k < nw; k++) {
        const int i = wp->wide[(size_t)k];
        ChunkDesc& d = plan.descs[(size_t)k];
        d = ChunkDesc{};
        d.raw_off = raw_off[i];
        d.comp_off = comp_off[i];
        d.nbytes = nbytes[i];
        d.destsize = comp_size ? comp_size[i] : 0x7fffffff;
        if (d.destsize < HEADER_LEN) return ERR_READ_BUFFER;
        d.blocksize = blocksize[i];
        d.nblocks = d.nbytes / d.blocksize;
        d.leftover = d.nbytes % d.blocksize;
        if (d.leftover) d.nblocks++;
        d.blk0 = blk;
        blk += d.nblocks;
        slot = imax(slot, decode_lds_bound(d.blocksize));
    }
    plan.total_blocks = blk;
    plan.lds_bytes = slot;
    plan.lds_lean = 0;
    plan.uniform_nblocks = uniform_blocks(plan.descs);
    wp->slot_bytes = (slot + 63) & ~63;
    return 0;
}

// The plans of the wide zstd read path (engine.hip: decompress_finish_wide_zstd): the walk decodes the sequences itself (no lane
// decoders, hence no table area to overflow) and a slot holds records for a sequence per three bytes -- zstd's shortest match --
// and literals for the whole block, so that no valid block is refused for its plan: these blocks have nobody to fall back to.
inline int zstd_wide_plan_cap(int area) { return ((area + area / 3) + 15) & ~15; }

}  // namespace cimg
