// tests/emu/wide_emu.cpp -- TEST INFRASTRUCTURE: the wide-block kernels (csrc/wide_kernel.h) on the host lane emulator,
// routed the way engine.hip routes them.  Linked together with emu.cpp (tests/test_emu_wide_blocks.py builds both into one
// library): a batch the normal planner takes runs through emu.cpp's batch functions, a batch it refuses for size goes to
// wide_plan.h and the wide kernels.
#define CIMG_EMULATE 1
#include "wide_plan.h"
#include <cstring>
#include <vector>

using namespace cimg;

extern "C" {

struct WideEmuCParams {                 // = emu.cpp's EmuCParams
    int32_t typesize, clevel, blocksize, compcode, splitmode;
    uint8_t filters[6], filters_meta[6];
};

int emu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                       const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);
int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes, const int32_t* blocksize,
                         uint8_t* raw, const int64_t* raw_off, int32_t* status);

static int g_wemu_waves = 3;            // persistent waves of the emulated encode launch
static int g_wemu_last_wide = 0;        // 1: the last batch went through the wide kernels

void wemu_set_waves(int n) { g_wemu_waves = n > 0 ? n : 1; }
int wemu_last_wide(void) { return g_wemu_last_wide; }

// lz4_wide_encode alone (the byU16 / byU32 LZ4 encoder of the wide launch)
int wemu_lz4_encode(const uint8_t* src, int n, uint8_t* out, int cap, int accel, int* need)
{
    std::vector<uint32_t> tab(4096 + 16, 0xCDCDCDCDu);
    int nd = 0;
    const int r = lz4_wide_encode(src, tab.data(), n, out, cap, accel, nd);
    *need = nd;
    return r;
}

int wemu_compress_batch(const WideEmuCParams* ep, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                        uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes)
{
    g_wemu_last_wide = 0;
    int rc = emu_compress_batch(ep, nchunks, raw, raw_off, nbytes, comp, comp_off, destsize, cbytes);
    if (rc != ERR_CODEC_SUPPORT) return rc;
    HostCParams p;
    p.typesize = ep->typesize; p.clevel = ep->clevel; p.blocksize = ep->blocksize; p.compcode = ep->compcode; p.splitmode = ep->splitmode;
    memcpy(p.filters, ep->filters, 6); memcpy(p.filters_meta, ep->filters_meta, 6);
    EncodePlan plan;
    if ((rc = plan_encode_wide(p, nchunks, raw_off, nbytes, comp_off, destsize, &plan)) < 0) return rc;
    g_wemu_last_wide = 1;
    std::vector<uint8_t> scratch((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
    std::vector<StreamRec> recs((size_t)plan.total_blocks * plan.cp.streams_per_block);
    std::vector<ChunkLayout> layout((size_t)nchunks);
    const int64_t stride = ((int64_t)plan.cp.max_blocksize + 255) & ~(int64_t)255;
    std::vector<uint8_t> planes((size_t)stride * (size_t)g_wemu_waves, 0xAB);
    uint32_t queue = 0;
    WideEncodeArgs a{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), plan.total_blocks, plan.uniform_nblocks,
                     planes.data(), stride, &queue};
    std::vector<uint32_t> tab(4096 + 16);
    for (int w = 0; w < g_wemu_waves; w++) {       // (the first wave drains the counter; the others find it dry)
        memset(tab.data(), 0xCD, tab.size() * 4);
        WideEncodeWave ww(a, tab.data(), w);
        ww.run();
    }
    AssembleArgs aa{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), comp, layout.data(), plan.uniform_nblocks, nullptr, 1};
    for (int c = 0; c < nchunks; c++) { LayoutChunk lc(aa, c); lc.run(); }
    for (int b = 0; b < plan.total_blocks; b++) { EmitBlock eb(aa, b); for (int w = 0; w < 4; w++) eb.run(w); }
    for (int c = 0; c < nchunks; c++) cbytes[c] = layout[(size_t)c].cbytes;
    return 0;
}

// the wide chunks of a batch through cimg_decode_wide's body; the others through emu_decompress_batch
int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status)
{
    g_wemu_last_wide = 0;
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
    g_wemu_last_wide = 1;
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
    for (size_t k = 0; k < wp.wide.size(); k++) {
        int s = wst[k];
        if (s == STATUS_ZSTD_PENDING || s == STATUS_ZSTD_PENDING_SPLIT) s = ERR_CODEC_SUPPORT;   // (zstd blocks this large: not built)
        status[wp.wide[k]] = s;
    }
    return 0;
}

}  // extern "C"
