// tests/emu/blosclz_wide_emu.cpp -- TEST INFRASTRUCTURE: BloscLZ on the wide write route on the host lane emulator, routed the way
// engine.hip routes it.  Linked together with emu.cpp (tests/test_emu_blosclz_wide.py builds the two into one library):
//   write  a batch the normal planner takes runs through emu.cpp; one it refuses for size goes to plan_encode_wide with the BloscLZ
//          flag set (as the engine sets it) and the BloscLZ or the LZ4 instance of the wide encoder, then the two assembly kernels.
//   read   the normal chunks through emu.cpp, the wide ones through cimg_decode_wide's body (wide_emu.cpp's wemu_decompress_batch,
//          restated: that file is not linked here).
// Every buffer the encoder sees is an allocation of exactly its size (the table: exactly 16 KiB), so that a sanitizer build of
// this file (blosclz_wide_asan_main.cpp) sees any load outside a stream.
#define CIMG_EMULATE 1
#include "wide_plan.h"
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cimg;

extern "C" {

struct BwEmuCParams {                   // = emu.cpp's EmuCParams
    int32_t typesize, clevel, blocksize, compcode, splitmode;
    uint8_t filters[6], filters_meta[6];
};

int emu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                       const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);
int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes, const int32_t* blocksize,
                         uint8_t* raw, const int64_t* raw_off, int32_t* status);

static int g_bw_waves = 3;              // persistent waves of the emulated encode launch
static int g_bw_route = 0;              // the last batch: 0 normal kernels, 1 cimg_encode_wide, 2 cimg_encode_wide_blosclz
static int g_bw_flag = 1;               // what plan_encode_wide is told about the BloscLZ instance (0: a caller without it)

void bwemu_set_waves(int n) { g_bw_waves = n > 0 ? n : 1; }
int bwemu_last_route(void) { return g_bw_route; }
void bwemu_set_blosclz_flag(int on) { g_bw_flag = on; }

// blosclz_wide_encode alone.  in_place = 0: the stream staged at the start of an allocation of n bytes; 1: at the END of a larger
// allocation (a slice of the caller's pixels that ends with them).  Table and output: allocations of exactly 16 KiB / cap bytes.
int bwemu_blosclz_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int clevel, int in_place, int* need)
{
    const size_t lead = in_place ? 4099 : 0;
    uint8_t* in = (uint8_t*)malloc(lead + (size_t)n + (n == 0));
    uint32_t* tab = (uint32_t*)malloc(LZ4_HASH_BYTES);
    uint8_t* out = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1));
    memset(in, 0xEE, lead);
    if (n) memcpy(in + lead, src, (size_t)n);
    memset(tab, 0xCD, LZ4_HASH_BYTES);
    int nd = 0;
    const int r = blosclz_wide_encode(in + lead, tab, n, out, cap, clevel, nd);
    if (r > 0) memcpy(dst, out, (size_t)r);
    if (need) *need = nd;
    free(in); free(tab); free(out);
    return r;
}

int bwemu_compress_batch(const BwEmuCParams* ep, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                         uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes)
{
    g_bw_route = 0;
    int rc = emu_compress_batch(ep, nchunks, raw, raw_off, nbytes, comp, comp_off, destsize, cbytes);
    if (rc != ERR_CODEC_SUPPORT) return rc;
    HostCParams p;
    p.typesize = ep->typesize; p.clevel = ep->clevel; p.blocksize = ep->blocksize; p.compcode = ep->compcode; p.splitmode = ep->splitmode;
    memcpy(p.filters, ep->filters, 6); memcpy(p.filters_meta, ep->filters_meta, 6);
    EncodePlan plan;
    if ((rc = plan_encode_wide(p, nchunks, raw_off, nbytes, comp_off, destsize, &plan, false, g_bw_flag != 0)) < 0) return rc;
    if (plan.cp.compcode == CODEC_ZSTD) return ERR_CODEC_SUPPORT;      // (zstd_wide_emu.cpp's route)
    g_bw_route = plan.cp.compcode == CODEC_BLOSCLZ ? 2 : 1;
    std::vector<uint8_t> scratch((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
    std::vector<StreamRec> recs((size_t)plan.total_blocks * plan.cp.streams_per_block);
    std::vector<ChunkLayout> layout((size_t)nchunks);
    const int64_t stride = ((int64_t)plan.cp.max_blocksize + 255) & ~(int64_t)255;
    std::vector<uint8_t> planes((size_t)stride * (size_t)g_bw_waves, 0xAB);
    uint32_t queue = 0;
    WideEncodeArgs a{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), plan.total_blocks, plan.uniform_nblocks,
                     planes.data(), stride, &queue};
    std::vector<uint32_t> tab(LZ4_HASH_BYTES / 4);                     // (exactly the table)
    for (int w = 0; w < g_bw_waves; w++) {         // (the first wave drains the counter; the others find it dry)
        memset(tab.data(), 0xCD, tab.size() * 4);
        if (plan.cp.compcode == CODEC_BLOSCLZ) { WideEncodeWaveT<CODEC_BLOSCLZ> ww(a, tab.data(), w); ww.run(); }
        else { WideEncodeWave ww(a, tab.data(), w); ww.run(); }
    }
    AssembleArgs aa{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), comp, layout.data(), plan.uniform_nblocks, nullptr, 1};
    for (int c = 0; c < nchunks; c++) { LayoutChunk lc(aa, c); lc.run(); }
    for (int b = 0; b < plan.total_blocks; b++) { EmitBlock eb(aa, b); for (int w = 0; w < 4; w++) eb.run(w); }
    for (int c = 0; c < nchunks; c++) cbytes[c] = layout[(size_t)c].cbytes;
    return 0;
}

// wemu_decompress_batch's twin: the wide chunks of a batch through cimg_decode_wide's body, the others through emu_decompress_batch
int bwemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                           const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status)
{
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
    for (size_t k = 0; k < wp.wide.size(); k++) status[wp.wide[k]] = wst[k];
    return 0;
}

}  // extern "C"
