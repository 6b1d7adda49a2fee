// tests/emu/helpers_emu.cpp -- TEST INFRASTRUCTURE: the emulated encode batch of emu.cpp with the waves of a launch stopped between
// their codec phase and their placing phase (EncodeStream::run_codec / run_place), so that a wave with nothing of its own to place
// runs as a HELPER while the chunks' owners have not placed yet (encode_kernel.h: encode_emit_own).  emu_compress_batch runs every
// wave to its end before the next starts: the first drains the queue and places everything, and no helper ever finds work.
// Here wave 1 encodes a budget of items and stops, wave 2 encodes the rest (every chunk is laid out then), and the schedule says who
// places when:
//   0  every wave to its end, one after the other (the order of emu_compress_batch)
//   1  the helper (wave 0, no items) places first, then the owners: they find their blocks marked and skip the stored planes
//   2  the owner places first, then the helpers: nothing is left for them.  (ONE owner, wave 1 with an unlimited budget: of two
//      owners the first to place would, done with its own, help the second.)
//   3  two helpers (waves 0 and 3), the second from a snapshot of the marks taken before the first: it places every block again
//      -- the same bytes --, then the owners
// Counters (emu_helpers_stats): stored streams left for placing, placed in all, placed by their owner, placed by another wave,
// skipped by their owner because marked.  Built by tests/test_emu_helpers_place.py into a library of its own, and with
// helpers_asan_main.cpp into a sanitizer program; never linked into libcimg_hip.so.
#include "emu.cpp"

extern "C" {

void emu_helpers_stats(long* out)
{
    out[0] = cimg::g_emu_src_left; out[1] = cimg::g_emu_src_placed; out[2] = cimg::g_emu_src_by_owner;
    out[3] = cimg::g_emu_src_by_helper; out[4] = cimg::g_emu_src_owner_skipped;
    cimg::g_emu_src_left = cimg::g_emu_src_placed = cimg::g_emu_src_by_owner = cimg::g_emu_src_by_helper = cimg::g_emu_src_owner_skipped = 0;
}

// LZ4 chunks only.  block_items: 0 plane items, 1 whole blocks, 2 the first half of the blocks whole.  helpers: 0 = the switch
// (CIMG_ENC_NO_HELPERS) set: no marks, every wave its own.
int emu_helpers_compress_batch(const EmuCParams* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                               uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes,
                               int schedule, int block_items_mode, int helpers, long* stats)
{
    long drop[5];
    emu_helpers_stats(drop);
    EncodePlan plan;
    int rc = plan_encode_batch(to_host(p), nchunks, raw_off, nbytes, comp_off, destsize, &plan);
    if (rc < 0) return rc;
    if (plan.cp.compcode != CODEC_LZ4) return -12;
    std::vector<uint8_t> scratch((size_t)plan.total_blocks * plan.cp.slot_bytes + 64, 0xEE);
    std::vector<StreamRec> recs((size_t)plan.total_blocks * plan.cp.streams_per_block);
    std::vector<ChunkLayout> layout((size_t)nchunks), layout_host((size_t)nchunks + 1);
    bool leftovers = false;
    for (const ChunkDesc& d : plan.descs) if (!d.assemble) leftovers = true;
    std::vector<uint32_t> chunk_count((size_t)nchunks, 0), ready((size_t)nchunks, 3);
    std::vector<uint32_t> placed((size_t)plan.total_blocks * (size_t)(plan.cp.streams_per_block + 1) + (size_t)nchunks, 3);        // (stale marks of an earlier generation)
    const uint32_t gen = 5;
    for (int split = 1; split >= 0; split--) {
        const int lds_bytes = split ? plan.lds_split : plan.lds_unsplit;
        if (!lds_bytes) continue;
        std::vector<uint32_t> queue((size_t)ENC_NQ * ENC_QSTRIDE, 0), queue_next((size_t)ENC_NQ * ENC_QSTRIDE, 77);
        bool block_items = split && block_items_mode;
        if (block_items)
            for (const ChunkDesc& d : plan.descs)
                if (!d.memcpyed && d.split && !encode_block_items_ok(plan.cp.typesize, plan.cp.filter, d.blocksize)) { block_items = false; break; }
        const int whole_blocks = !block_items ? 0 : (block_items_mode == 2 ? plan.total_blocks / 2 : plan.total_blocks);
        const int items = encode_items(plan.total_blocks, plan.cp.streams_per_block, split != 0, whole_blocks);
        std::vector<int32_t> next_item((size_t)items + 1, -7);
        EncodeArgs ea{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), lds_bytes, plan.total_blocks, split, nullptr, queue.data(), plan.uniform_nblocks, whole_blocks,
                      nullptr, 0, nullptr,
                      queue_next.data(), 4, 1, comp, layout.data(), layout_host.data(), chunk_count.data(), ready.data(), next_item.data(), gen,
                      helpers ? placed.data() : nullptr, helpers ? 1 : 0};
        // four waves, each with LDS of its own (a wave's plane does not outlive its codec phase, but the emulator should not rely on it)
        std::vector<std::vector<uint8_t>> lds(4, std::vector<uint8_t>((size_t)lds_bytes + EMU_LDS_SLACK, 0xCD));
        EncodeStream<CODEC_LZ4> h0(&ea, lds[0].data(), 0), a(&ea, lds[1].data(), 1), b(&ea, lds[2].data(), 2), h3(&ea, lds[3].data(), 3);
        if (schedule == 0) {
            a.run(); b.run(); h3.run(); h0.run();
        } else {
            a.run_codec(schedule == 2 ? 0x7fffffff : (items + 1) / 2);
            b.run_codec(0x7fffffff);
            h0.run_codec(0x7fffffff);                          // (finds the queue dry; wave 0 zeroes the next launch's heads)
            h3.run_codec(0x7fffffff);
            if (schedule == 1) { h0.run_place(); a.run_place(); b.run_place(); h3.run_place(); }
            else if (schedule == 2) { a.run_place(); b.run_place(); h0.run_place(); h3.run_place(); }
            else {
                const std::vector<uint32_t> before = placed;
                h0.run_place();
                const std::vector<uint32_t> after = placed;
                placed = before;
                h3.run_place();
                for (size_t i = 0; i < placed.size(); i++) if (after[i] == gen) placed[i] = gen;
                a.run_place(); b.run_place();
            }
        }
        for (int q = 0; q < ENC_NQ; q++) if (queue_next[(size_t)q * ENC_QSTRIDE] != 0) return -1;   // the next launch's heads were zeroed
    }
    if (layout_host[(size_t)nchunks].cbytes < 0) return -1;                      // a wave waited in vain
    for (int c = 0; c < nchunks; c++) if (chunk_count[(size_t)c] != 0) return -1;
    for (int c = 0; c < nchunks; c++) if (plan.descs[(size_t)c].assemble && ready[(size_t)c] != gen) return -1;
    if (leftovers) {
        AssembleArgs aa{plan.descs.data(), nchunks, plan.cp, raw, scratch.data(), recs.data(), comp, layout.data(), plan.uniform_nblocks, nullptr, 1};
        for (int c = 0; c < nchunks; c++) { LayoutChunk lc(aa, c); lc.run(); }
        for (int b2 = 0; b2 < plan.total_blocks; b2++) { EmitBlock eb(aa, b2); for (int w = 0; w < 4; w++) eb.run(w); }
    }
    for (int c = 0; c < nchunks; c++) cbytes[c] = layout[(size_t)c].cbytes;
    emu_helpers_stats(stats);
    return 0;
}

}
