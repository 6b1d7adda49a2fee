// tests/emu/window_write_env.h -- TEST INFRASTRUCTURE: an update call (csrc/update_plan.h: run_update) with the kernel bodies of
// csrc/update_kernel.h and the batch encoder of csrc/encode_kernel.h on the host lane emulator.  Shared by window_write_emu.cpp
// (tests/test_emu_window_writes.py) and mock_window_write.cpp (the Python module's mock backend); each hands in the batch decoder and
// the batch compressor of its library.
#pragma once
#ifndef CIMG_EMULATE
#define CIMG_EMULATE 1
#endif
#include "update_plan.h"
#include "window_env.h"

namespace cimg {

// the batch compress (cparams laid out as cimg_cparams / HostCParams)
typedef int (*EmuCompressFn)(const void* p, int n, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                             const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);

struct EmuUpdateEnv : EmuChunks {
    EmuCompressFn compress_fn;
    const uint8_t* src;
    uint8_t* newbuf;
    std::vector<uint8_t> patchbuf, scratch;
    std::vector<StreamRec> recs;

    int headers(const std::vector<int>& list, uint8_t* out)
    {
        for (size_t k = 0; k < list.size(); k++) memcpy(out + k * HEADER_LEN, comp + comp_off[list[k]], HEADER_LEN);
        return 0;
    }

    int patch(const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<PatchUnit>& units, const std::vector<WindowItem>& stage,
              const std::vector<WindowItem>& items, int to_whole, int64_t patch_bytes, int32_t* status)
    {
        if (!to_whole) patchbuf.assign((size_t)patch_bytes + 64, 0xEE);
        const int nchunks = (int)descs.size();
        std::vector<int32_t> st((size_t)nchunks, 0);
        PatchArgs pa{};
        pa.w.d = DecodeArgs{descs.data(), nchunks, comp, nullptr, st.data(), lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        pa.w.items = stage.data();
        pa.w.nitems = (int32_t)stage.size();
        pa.units = units.data();
        pa.items = items.data();
        pa.src = src;
        pa.dst = to_whole ? whole.data() : patchbuf.data();
        pa.nunits = (int32_t)units.size();
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)units.size(); k++) {
            memset(lds.data(), 0xCD, lds.size());
            PatchBlock pb(pa, lds.data(), k);
            PatchBlock p0 = pb, p1 = pb, p2 = pb, p3 = pb;       // each wave keeps its own copy of the uniform walk
            PatchBlock* ws[4] = {&p0, &p1, &p2, &p3};
            for (int w = 0; w < 4; w++) ws[w]->phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->phase_base(w);
            for (int i = 0; i < pb.u.nitems; i++)
                for (int w = 0; w < 4; w++) ws[w]->overlay(w, i);
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }

    // the batch encode launch over the patch buffer (engine.hip: encode_launch without assembly), persistent waves one after the other
    int encode(const EncodePlan& plan)
    {
        const int n = (int)plan.descs.size();
        scratch.assign((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
        recs.assign((size_t)plan.total_blocks * plan.cp.streams_per_block, StreamRec{-1, -1, -1, -1});
        std::vector<ChunkLayout> layout((size_t)n), layout_host((size_t)n + 1);
        std::vector<uint32_t> chunk_count((size_t)n, 0), ready((size_t)n, 3);
        static ZstdEncTables ztabs;
        zstd_build_enc_tables(&ztabs);
        for (int split = 1; split >= 0; split--) {
            const int lds_bytes = split ? plan.lds_split : plan.lds_unsplit;
            if (!lds_bytes) continue;
            std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
            std::vector<uint32_t> queue((size_t)ENC_NQ * ENC_QSTRIDE, 0), queue_next((size_t)ENC_NQ * ENC_QSTRIDE, 77);
            const int zstride = 2 * (plan.cp.max_blocksize / 4 + 64);
            std::vector<uint32_t> zseq((size_t)zstride * 4, 0xA5A5A5A5u);
            std::vector<int32_t> next_item((size_t)encode_items(plan.total_blocks, plan.cp.streams_per_block, split != 0, 0) + 1, -7);
            const int nwaves = 3;
            EncodeArgs ea{plan.descs.data(), n, plan.cp, patchbuf.data(), scratch.data(), recs.data(), lds_bytes, plan.total_blocks, split,
                          nullptr, queue.data(), plan.uniform_nblocks, 0, zseq.data(), zstride, &ztabs, queue_next.data(), nwaves, 0, nullptr,
                          layout.data(), layout_host.data(), chunk_count.data(), ready.data(), next_item.data(), 5};
            for (int w = nwaves - 1; w >= 0; w--) {
                memset(lds.data(), 0xCD, lds.size());
                if (plan.cp.compcode == CODEC_BLOSCLZ) { EncodeStream<CODEC_BLOSCLZ> es(&ea, lds.data(), w); es.run(); }
                else { EncodeStream<CODEC_LZ4> es(&ea, lds.data(), w); es.run(); }
            }
        }
        return 0;
    }

    int splice(const CodecParams& cp, const std::vector<SpliceChunk>& chunks, std::vector<SpliceBlock> blocks, std::vector<ChunkLayout>& lay)
    {
        SpliceArgs sa{chunks.data(), (int32_t)chunks.size(), (int32_t)blocks.size(), blocks.data(), cp, comp, newbuf, scratch.data(),
                      recs.data(), lay.data()};
        for (int c = 0; c < (int)chunks.size(); c++) { SpliceLayout sl(sa, c); sl.run(); }
        for (int k = 0; k < (int)blocks.size(); k++) { SpliceEmit se(sa, k); for (int w = 0; w < 4; w++) se.run(w); }
        return 0;
    }

    int compress(const HostCParams& p, const std::vector<int>& list, const std::vector<int64_t>& raw_off, const std::vector<int32_t>& nb,
                 const std::vector<int32_t>& ds, const std::vector<int64_t>& new_off, int32_t* cbytes)
    {
        (void)list;
        return compress_fn(&p, (int)nb.size(), whole.data(), raw_off.data(), nb.data(), newbuf, new_off.data(), ds.data(), cbytes);
    }
};

// = cimg_update_windows_device: sizes from the caller, device pointers are host pointers
inline int emu_update_device(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp, const int64_t* comp_off,
                             const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows,
                             const WindowSpec* w, const uint8_t* src, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes,
                             int32_t* status, UpdateStats* stats)
{
    EmuUpdateEnv env{{wf, comp, comp_off, comp_size, nbytes, blocksize, {}}, cf, src, newbuf, {}, {}, {}};
    return run_update(env, p, nchunks, comp_off, comp_size, nbytes, blocksize, destsize, nwindows, w, new_off, new_cbytes, status, stats);
}

// = cimg_update_windows_host: planned as the engine plans it, staged with memcpy where the engine copies over PCIe -- into buffers that
// end at their last used byte, for the sanitizers; every touched chunk's new form in memory from `alloc`
inline int emu_update_host(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp, const int64_t* comp_off,
                           const int32_t* comp_size, const int32_t* destsize, int nwindows, const WindowSpec* w, const uint8_t* src,
                           void* (*alloc)(void*, size_t), void* user, void** new_chunks, int32_t* new_cbytes, int32_t* status,
                           UpdateStats* stats)
{
    *stats = UpdateStats{};
    int rc = open_update_call(nchunks, nwindows, status, new_cbytes, new_chunks);
    if (rc) return rc > 0 ? 0 : rc;
    if (nchunks == 0 || !alloc) return ERR_INVALID_PARAM;
    UpdateHostPlan hp;
    if ((rc = plan_update_host(p.typesize, nchunks, comp, comp_off, comp_size, destsize, nwindows, w, status, &hp)) < 0) return rc;
    std::vector<uint8_t> sc((size_t)hp.comp_used), ss((size_t)hp.rows_used), newbuf((size_t)hp.new_used, 0);
    for (int i = 0; i < nchunks; i++) if (hp.up[(size_t)i]) memcpy(sc.data() + hp.d_comp_off[(size_t)i], comp + comp_off[i], (size_t)hp.up[(size_t)i]);
    for (int k = 0; k < nwindows; k++) {
        const WindowSpec& d = hp.dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(ss.data() + d.out_off, d.out_pitch, src + w[k].out_off, w[k].out_pitch, d.out_pitch, w[k].height);
    }
    rc = emu_update_device(wf, cf, p, nchunks, sc.data(), hp.d_comp_off.data(), hp.held.data(), hp.nbytes.data(), hp.blocksize.data(), destsize,
                           nwindows, hp.dw.data(), ss.data(), newbuf.data(), hp.new_off.data(), new_cbytes, status, stats);
    stats->bytes_uploaded += hp.bytes_uploaded;
    if (rc == ERR_INVALID_PARAM) return rc;
    for (int i = 0; i < nchunks; i++) {
        if (new_cbytes[i] <= 0) continue;
        void* m = alloc(user, (size_t)new_cbytes[i]);
        if (!m) return -4;
        memcpy(m, newbuf.data() + hp.new_off[(size_t)i], (size_t)new_cbytes[i]);
        new_chunks[i] = m;
    }
    return rc;
}

}  // namespace cimg
