// tests/emu/trunc_emu.cpp -- TEST INFRASTRUCTURE: the trunc-prec pass (csrc/trunc_kernel.h, csrc/trunc_plan.h) on the host lane
// emulator, tile by tile as a launch would run it, and behind it the emulated encode launches with the planner told that the pass has
// run (tests/test_trunc_plan.py and tests/test_emu_trunc_prec.py compile it into a pytest temp directory; the sanitizer build links
// trunc_asan_main.cpp beside it).  The encode part follows emu.cpp's emu_compress_batch in its default form.
#define CIMG_EMULATE 1
#include "plan.h"
#include "assemble_kernel.h"
#include "blosclz_kernel.h"
#include "trunc_kernel.h"
#include <cstring>
#include <vector>

#ifndef EMU_LDS_SLACK
#define EMU_LDS_SLACK 64
#endif

namespace cimg {
int g_emu_zstd_take = 1 << 30; long g_emu_zx_batches = 0, g_emu_zx_rounds = 0, g_emu_zx_par = 0, g_emu_zx_serial = 0, g_emu_zx_longlit = 0;
long g_emu_d2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
long g_emu_dec_par = 0, g_emu_dec_serial = 0, g_emu_dec_batches = 0; int g_emu_write_order = 0; long g_emu_windows = 0, g_emu_matches = 0, g_emu_collisions = 0;
}
using namespace cimg;

extern "C" {

struct EmuCParams {
    int32_t typesize, clevel, blocksize, compcode, splitmode;
    uint8_t filters[6], filters_meta[6];
};

static HostCParams to_host(const EmuCParams* p)
{
    HostCParams h;
    h.typesize = p->typesize; h.clevel = p->clevel; h.blocksize = p->blocksize;
    h.compcode = p->compcode; h.splitmode = p->splitmode;
    memcpy(h.filters, p->filters, 6); memcpy(h.filters_meta, p->filters_meta, 6);
    return h;
}

void tremu_write_order(int o) { g_emu_write_order = o; }

// trunc_plan.h: validity of (typesize, meta), and the bits zeroed / the mask over eight bytes where valid
int tremu_check(int typesize, int meta, int* zeroed, uint64_t* mask64)
{
    int z = 0;
    const int rc = trunc_zeroed_bits(typesize, meta, &z);
    if (rc < 0) return rc;
    *zeroed = z;
    *mask64 = trunc_mask64(typesize, z);
    return 0;
}

// what a compress call makes of the cparams: 0 not named, 1 named and valid, < 0 refused
int tremu_from_cparams(const EmuCParams* p)
{
    uint64_t m = 0;
    return trunc_from_cparams(p->typesize, p->filters, p->filters_meta, &m);
}

// the planner's answer for one chunk of nbytes, with and without the caller's word that the pass has run
int tremu_plan_rc(const EmuCParams* p, int32_t nbytes, int truncated)
{
    EncodePlan plan;
    const int64_t zero = 0;
    const int32_t dest = nbytes + 32;
    return plan_encode_batch(to_host(p), 1, &zero, &nbytes, &zero, &dest, &plan, truncated != 0);
}

// = the engine's trunc_launch: piece i from src[i] to dst[i] (the same address: in place)
int tremu_pass(int n, const void* const* src, void* const* dst, const int32_t* bytes, int typesize, int meta)
{
    int z = 0;
    if (trunc_zeroed_bits(typesize, meta, &z) < 0) return ERR_INVALID_PARAM;
    std::vector<PackPiece> pieces;
    int64_t ntiles = 0;
    if (trunc_plan_pieces(n, src, dst, bytes, typesize, pieces, &ntiles)) return ERR_INVALID_PARAM;
    if (pieces.empty()) return 0;
    TruncArgs a{pieces.data(), (int32_t)pieces.size(), (int32_t)ntiles, trunc_mask64(typesize, z), typesize, 0};
    for (int64_t t = 0; t < ntiles; t++) trunc_wave(a, (int)t);
    return 0;
}

int64_t tremu_tiles(int n, const void* const* src, void* const* dst, const int32_t* bytes, int typesize)
{
    std::vector<PackPiece> pieces;
    int64_t ntiles = 0;
    const int rc = trunc_plan_pieces(n, src, dst, bytes, typesize, pieces, &ntiles);
    return rc ? rc : ntiles;
}

// = the engine's compress_launch for pixels it owns: the pass in place over `raw` (the caller's copy), then the encode launches and
// the assembly planned as for the same cparams without slot 4
int tremu_compress_batch(const EmuCParams* p, int nchunks, uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                         const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes)
{
    const HostCParams hp = to_host(p);
    uint64_t mask64 = 0;
    const int trunc = trunc_from_cparams(hp.typesize, hp.filters, hp.filters_meta, &mask64);
    if (trunc < 0) return trunc;
    EncodePlan plan;
    int rc = plan_encode_batch(hp, nchunks, raw_off, nbytes, comp_off, destsize, &plan, trunc != 0);
    if (rc < 0) return rc;
    if (trunc) {
        std::vector<const void*> s((size_t)nchunks);
        std::vector<void*> d((size_t)nchunks);
        for (int i = 0; i < nchunks; i++) s[(size_t)i] = d[(size_t)i] = raw + raw_off[i];
        if ((rc = tremu_pass(nchunks, s.data(), d.data(), nbytes, hp.typesize, hp.filters_meta[4]))) return rc;
    }
    std::vector<uint8_t> scratch((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
    std::vector<StreamRec> recs((size_t)plan.total_blocks * plan.cp.streams_per_block);
    std::vector<ChunkLayout> layout((size_t)nchunks), layout_host((size_t)nchunks + 1);
    bool leftovers = false;
    for (const ChunkDesc& d : plan.descs) if (!d.assemble) leftovers = true;
    std::vector<uint32_t> chunk_count((size_t)nchunks, 0), ready((size_t)nchunks, 3);
    const uint32_t gen = 5;
    for (int split = 1; split >= 0; split--) {
        const int lds_bytes = split ? plan.lds_split : plan.lds_unsplit;
        if (!lds_bytes) continue;
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
        std::vector<uint32_t> queue((size_t)ENC_NQ * ENC_QSTRIDE, 0), queue_next((size_t)ENC_NQ * ENC_QSTRIDE, 77);
        bool block_items = split != 0;
        if (block_items)
            for (const ChunkDesc& d : plan.descs)
                if (!d.memcpyed && d.split && !encode_block_items_ok(plan.cp.typesize, plan.cp.filter, d.blocksize)) { block_items = false; break; }
        const int whole_blocks = block_items ? plan.total_blocks : 0;
        const int zstride = 2 * (plan.cp.max_blocksize / 4 + 64);
        std::vector<uint32_t> zseq((size_t)zstride * 4, 0xA5A5A5A5u);
        static ZstdEncTables ztabs;
        zstd_build_enc_tables(&ztabs);
        const int emu_waves = 3;
        std::vector<int32_t> next_item((size_t)encode_items(plan.total_blocks, plan.cp.streams_per_block, split != 0, whole_blocks) + 1, -7);
        EncodeArgs ea{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), lds_bytes, plan.total_blocks, split, nullptr, queue.data(), plan.uniform_nblocks, whole_blocks,
                      zseq.data(), zstride, &ztabs,
                      queue_next.data(), emu_waves, 1, comp, layout.data(), layout_host.data(), chunk_count.data(), ready.data(), next_item.data(), gen};
        for (int w = emu_waves - 1; w >= 0; w--) {
            memset(lds.data(), 0xCD, lds.size());
            if (plan.cp.compcode == CODEC_BLOSCLZ) { EncodeStream<CODEC_BLOSCLZ> es(&ea, lds.data(), w); es.run(); }
            else if (plan.cp.compcode == CODEC_ZSTD) { EncodeStream<CODEC_ZSTD> es(&ea, lds.data(), w); es.run(); }
            else { EncodeStream<CODEC_LZ4> es(&ea, lds.data(), w); es.run(); }
        }
    }
    if (layout_host[(size_t)nchunks].cbytes < 0) return -1;
    if (leftovers) {
        AssembleArgs aa{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), comp, layout.data(), plan.uniform_nblocks, nullptr, 1};
        for (int c = 0; c < nchunks; c++) { LayoutChunk lc(aa, c); lc.run(); }
        for (int b = 0; b < plan.total_blocks; b++) { EmitBlock eb(aa, b); for (int w = 0; w < 4; w++) eb.run(w); }
    }
    for (int c = 0; c < nchunks; c++) cbytes[c] = layout[(size_t)c].cbytes;
    return 0;
}

}  // extern "C"
