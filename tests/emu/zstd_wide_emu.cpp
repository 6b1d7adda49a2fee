// tests/emu/zstd_wide_emu.cpp -- TEST INFRASTRUCTURE: the wide zstd paths on the host lane emulator, routed the way engine.hip
// routes them.  Linked together with emu.cpp and wide_emu.cpp (tests/test_emu_zstd_wide_blocks.py builds the three into one library):
//   write  a batch the normal planner takes runs through emu.cpp; one it refuses for size goes to wide_plan.h and the zstd or the
//          LZ4 instance of the wide encoder (wide_kernel.h), then the two assembly kernels.  (wide_emu.cpp's wemu_compress_batch
//          runs the LZ4 instance only: it predates zstd on the wide path and is not the route for zstd batches.)
//   read   the normal chunks through emu.cpp, the wide ones through cimg_decode_wide's body; wide blocks it leaves with
//          STATUS_ZSTD_PENDING[_SPLIT] go through the zstd read path's walk (no lane decoders) and the replay out of a slot in
//          "device memory" (zstd_walk_kernel.h: ZstdReplayBlockT<uint8_t*>), as decompress_finish_wide_zstd does.
#define CIMG_EMULATE 1
#include "wide_plan.h"
#include "zstd_walk_kernel.h"
#include <cstring>
#include <vector>

using namespace cimg;

extern "C" {

struct ZwEmuCParams {                   // = emu.cpp's EmuCParams
    int32_t typesize, clevel, blocksize, compcode, splitmode;
    uint8_t filters[6], filters_meta[6];
};

int emu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                       const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);
int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes, const int32_t* blocksize,
                         uint8_t* raw, const int64_t* raw_off, int32_t* status);

static int g_zw_waves = 3;              // persistent waves of the emulated encode launch / replay workgroups
static int g_zw_route = 0;              // the last batch: 0 normal kernels only, 1 wide kernels, 2 wide kernels and the wide zstd read path
static int g_zw_plan_fail = 0;          // 1: the plans' device memory cannot be had (engine.hip: CIMG_ZSTD_PLAN_FAIL)

void zwemu_set_waves(int n) { g_zw_waves = n > 0 ? n : 1; }
int zwemu_last_route(void) { return g_zw_route; }
void zwemu_set_plan_fail(int on) { g_zw_plan_fail = on; }

static const ZstdEncTables* enc_tables()
{
    static ZstdEncTables t;
    static bool built = false;
    if (!built) { zstd_build_enc_tables(&t); built = true; }
    return &t;
}

// zstd_wide_encode alone: one stream -> one frame in dst[0, cap) (0: not smaller than n / does not fit)
int zwemu_zstd_encode(const uint8_t* src, int n, uint8_t* dst, int cap)
{
    std::vector<uint32_t> lds((size_t)WIDE_ZSTD_LDS / 4, 0xCDCDCDCDu);     // (exactly the launch's LDS)
    memcpy(lds.data() + LZ4_HASH_BYTES / 4, enc_tables(), sizeof(ZstdEncTables));
    std::vector<uint64_t> seq((size_t)WIDE_ZSTD_SEQ_STRIDE, 0xA5A5A5A5A5A5A5A5ull);
    return zstd_wide_encode(src, lds.data(), reinterpret_cast<const ZstdEncTables*>(lds.data() + LZ4_HASH_BYTES / 4), n, dst, cap, seq.data());
}

int zwemu_compress_batch(const ZwEmuCParams* ep, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                         uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes)
{
    g_zw_route = 0;
    int rc = emu_compress_batch(ep, nchunks, raw, raw_off, nbytes, comp, comp_off, destsize, cbytes);
    if (rc != ERR_CODEC_SUPPORT) return rc;
    HostCParams p;
    p.typesize = ep->typesize; p.clevel = ep->clevel; p.blocksize = ep->blocksize; p.compcode = ep->compcode; p.splitmode = ep->splitmode;
    memcpy(p.filters, ep->filters, 6); memcpy(p.filters_meta, ep->filters_meta, 6);
    EncodePlan plan;
    if ((rc = plan_encode_wide(p, nchunks, raw_off, nbytes, comp_off, destsize, &plan)) < 0) return rc;
    g_zw_route = 1;
    std::vector<uint8_t> scratch((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
    std::vector<StreamRec> recs((size_t)plan.total_blocks * plan.cp.streams_per_block);
    std::vector<ChunkLayout> layout((size_t)nchunks);
    const int64_t stride = ((int64_t)plan.cp.max_blocksize + 255) & ~(int64_t)255;
    std::vector<uint8_t> planes((size_t)stride * (size_t)g_zw_waves, 0xAB);
    uint32_t queue = 0;
    WideEncodeArgs a{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), plan.total_blocks, plan.uniform_nblocks,
                     planes.data(), stride, &queue};
    std::vector<uint64_t> seq((size_t)WIDE_ZSTD_SEQ_STRIDE * (size_t)g_zw_waves, 0xA5A5A5A5A5A5A5A5ull);
    WideZstdEncodeArgs za{a, seq.data(), WIDE_ZSTD_SEQ_STRIDE, enc_tables()};
    std::vector<uint32_t> lds((size_t)WIDE_ZSTD_LDS / 4);
    for (int w = 0; w < g_zw_waves; w++) {         // (the first wave drains the counter; the others find it dry)
        memset(lds.data(), 0xCD, lds.size() * 4);
        if (plan.cp.compcode == CODEC_ZSTD) { WideEncodeWaveT<CODEC_ZSTD> ww(za, lds.data(), w); ww.run(); }
        else { WideEncodeWave ww(a, lds.data(), w); ww.run(); }
    }
    AssembleArgs aa{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), comp, layout.data(), plan.uniform_nblocks, nullptr, 1};
    for (int c = 0; c < nchunks; c++) { LayoutChunk lc(aa, c); lc.run(); }
    for (int b = 0; b < plan.total_blocks; b++) { EmitBlock eb(aa, b); for (int w = 0; w < 4; w++) eb.run(w); }
    for (int c = 0; c < nchunks; c++) cbytes[c] = layout[(size_t)c].cbytes;
    return 0;
}

// the wide zstd read path over the wide chunks' plan (status: their words; the pending ones have been cleared)
static int zw_read_wide_zstd(const DecodeArgs& base, int max_bs, const std::vector<int>& pending_chunks)
{
    if (g_zw_plan_fail) {
        for (int k : pending_chunks) base.status[k] = -4;      // BLOSC2_ERROR_MEMORY_ALLOC
        return 0;
    }
    const int area = zstd_kernel_area(max_bs), cap = zstd_wide_plan_cap(area);
    const int64_t stride = zstd_plan_stride(cap, false);
    std::vector<uint8_t> zplan((size_t)base.total_blocks * (size_t)stride, 0xCD);
    std::vector<uint32_t> counter(4, 0);
    DecodeArgs zb = base;
    zb.skipped = counter.data();
    zb.zplan = zplan.data(); zb.zplan_stride = stride; zb.zcap = cap; zb.zarea = area; zb.zlanes = 0; zb.zblocks = base.total_blocks;
    zb.blk_first = 0;
    zb.tune = 2;                                                // (a block the walk refuses has nobody to go to)
    DecodeArgs wa = zb;
    wa.lds_bytes = zstd_walk_lds_bytes(2048);                   // (engine.hip: zstd_walk_stage)
    std::vector<uint8_t> wl((size_t)wa.lds_bytes);
    for (int b = 0; b < base.total_blocks; b++) {
        memset(wl.data(), 0xCD, wl.size());
        ZstdWalkBlock blk(wa, wl.data(), b);
        blk.run();
    }
    DecodeArgs ra = zb;
    ra.lds_bytes = zstd_replay_lds_bytes(max_bs);
    std::vector<uint8_t> slots((size_t)ra.lds_bytes * (size_t)g_zw_waves);     // (exactly: the executor's fetches stay inside the slot)
    for (int b = 0; b < base.total_blocks; b++) {               // workgroup k of the persistent launch: blocks k, k + G, ...
        uint8_t* slot = slots.data() + (size_t)(b % g_zw_waves) * (size_t)ra.lds_bytes;
        memset(slot, 0xCD, (size_t)ra.lds_bytes);
        ZstdReplayBlockT<uint8_t*> blk(ra, slot, b);
        blk.run();
    }
    return 0;
}

int zwemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                           const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status)
{
    g_zw_route = 0;
    DecodePlan probe;
    int rc = plan_decode_batch(nchunks, comp_off, nbytes, blocksize, raw_off, &probe, comp_size);
    if (rc == 0 && !comp_size) return emu_decompress_batch(nchunks, comp, comp_off, nbytes, blocksize, raw, raw_off, status);
    if (rc != ERR_CODEC_SUPPORT && rc != 0) return rc;
    WideDecodePlan wp;
    if (rc == ERR_CODEC_SUPPORT) { if ((rc = plan_decode_wide(nchunks, comp_off, nbytes, blocksize, raw_off, &wp, comp_size)) < 0) return rc; }
    else for (int i = 0; i < nchunks; i++) wp.normal.push_back(i);
    memset(status, 0, sizeof(int32_t) * (size_t)nchunks);
    if (!wp.normal.empty()) {
        const size_t nn = wp.normal.size();
        const SubBatch sub(wp.normal, comp_off, nullptr, nbytes, blocksize, raw_off);
        std::vector<int32_t> st(nn, 0);
        if ((rc = emu_decompress_batch((int)nn, comp, sub.co.data(), sub.nb.data(), sub.bs.data(), raw, sub.ro.data(), st.data())) < 0) return rc;
        for (size_t k = 0; k < nn; k++) status[wp.normal[k]] = st[k];
    }
    if (wp.wide.empty()) return 0;
    g_zw_route = 1;
    const DecodePlan& plan = wp.plan;
    std::vector<int32_t> wst(wp.wide.size(), 0);
    std::vector<uint8_t> slot((size_t)wp.slot_bytes + 64);
    WideDecodeArgs a{};
    a.d = DecodeArgs{plan.descs.data(), (int32_t)wp.wide.size(), comp, raw, wst.data(), wp.slot_bytes, nullptr, plan.uniform_nblocks,
                     nullptr, 0, nullptr, plan.total_blocks, 0, 1, 0};
    a.slots = slot.data();
    for (int b = 0; b < plan.total_blocks; b++) {
        memset(slot.data(), 0xCD, slot.size());
        WideDecodeBlock blk(a.d, a.slots, b);
        WideDecodeBlock w0 = blk, w1 = blk, w2 = blk, w3 = blk;   // each wave keeps its own copy of the uniform walk
        WideDecodeBlock* ws[4] = {&w0, &w1, &w2, &w3};
        for (int w = 0; w < 4; w++) ws[w]->phase_a_wide(w);
        for (int w = 0; w < 4; w++) ws[w]->phase_b(w);
    }
    // as decompress_finish does: the chunks cimg_decode_wide left pending go through the wide zstd read path
    std::vector<int> pending;
    for (size_t k = 0; k < wst.size(); k++) if (wst[k] == STATUS_ZSTD_PENDING || wst[k] == STATUS_ZSTD_PENDING_SPLIT) { pending.push_back((int)k); wst[k] = 0; }
    if (!pending.empty()) {
        g_zw_route = 2;
        int max_bs = 0;
        for (const ChunkDesc& d : plan.descs) max_bs = d.blocksize > max_bs ? d.blocksize : max_bs;
        if ((rc = zw_read_wide_zstd(a.d, max_bs, pending)) < 0) return rc;
    }
    for (size_t k = 0; k < wp.wide.size(); k++) status[wp.wide[k]] = wst[k];
    return 0;
}

}  // extern "C"
