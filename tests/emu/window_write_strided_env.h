// tests/emu/window_write_strided_env.h -- TEST INFRASTRUCTURE: a strided update call (csrc/update_plan.h: run_update over
// StridedWindowSpec) with the body of cimg_update_patch_strided (csrc/update_kernel.h: StridedPatchBlock) on the host lane emulator,
// over window_write_env.h's encode, splice and compress steps.  Shared by window_write_strided_emu.cpp
// (tests/test_emu_window_writes_strided.py) and mock_window_write_strided.cpp (the Python module's mock backend).  The four waves of a
// workgroup write a DISJOINT unit in a test-selected order (g_emu_write_order), since the kernel lets them run free there; an
// ordered unit runs item after item, as the barrier makes it.
#pragma once
#include "window_write_env.h"
#include "trunc_kernel.h"

namespace cimg {

struct EmuStridedUpdateEnv : EmuUpdateEnv {
    int64_t disjoint_units = 0, ordered_units = 0;     // units of more than one item, by schedule

    int patch_strided(const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<StridedPatchUnit>& units,
                      const std::vector<WindowItem>& stage, const std::vector<StridedWindowItem>& items, int to_whole, int64_t patch_bytes,
                      int32_t* status)
    {
        if (!to_whole) patchbuf.assign((size_t)patch_bytes + 64, 0xEE);
        const int nchunks = (int)descs.size();
        std::vector<int32_t> st((size_t)nchunks, 0);
        // (the tables as exact allocations of their own, for the sanitizers)
        const std::vector<StridedPatchUnit> un(units.begin(), units.end());
        const std::vector<StridedWindowItem> it(items.begin(), items.end());
        const std::vector<WindowItem> sg(stage.begin(), stage.end());
        StridedPatchArgs sa{};
        sa.p.w.d = DecodeArgs{descs.data(), nchunks, comp, nullptr, st.data(), lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        sa.p.w.items = sg.data();
        sa.p.w.nitems = (int32_t)sg.size();
        sa.p.src = src;
        sa.p.dst = to_whole ? whole.data() : patchbuf.data();
        sa.p.nunits = (int32_t)un.size();
        sa.units = un.data();
        sa.items = it.data();
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)un.size(); k++) {
            if (!lds.empty()) memset(lds.data(), 0xCD, lds.size());      // (a launch over chunks decoded whole has no LDS)
            StridedPatchBlock sb(sa, lds.data(), k);
            StridedPatchBlock s0 = sb, s1 = sb, s2 = sb, s3 = sb;       // each wave keeps its own copy of the uniform walk
            StridedPatchBlock* ws[4] = {&s0, &s1, &s2, &s3};
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_base(w);
            const int n = sb.pb.u.nitems;
            if (n == 1) {
                for (int w = 0; w < 4; w++) ws[w]->overlay(0, w * 64, 256);
            } else if (sb.disjoint) {
                disjoint_units++;
                for (int i = 0; i < 4; i++) {
                    const int w = g_emu_write_order == 1 ? 3 - i : g_emu_write_order == 2 ? (i * 3 + 2) & 3 : i;
                    for (int j = w; j < n; j += 4) ws[w]->overlay(j, 0, 64);
                }
            } else {
                ordered_units++;
                for (int j = 0; j < n; j++)
                    for (int w = 0; w < 4; w++) ws[w]->overlay(j, w * 64, 256);
            }
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }

    // trunc-prec over patched slots of the patch buffer, in place, in front of encode() (engine.hip: trunc_launch)
    int trunc(int typesize, uint64_t mask64, const std::vector<int64_t>& off, const std::vector<int32_t>& len)
    {
        std::vector<const void*> s;
        std::vector<void*> d;
        for (const int64_t o : off) { s.push_back(patchbuf.data() + o); d.push_back(patchbuf.data() + o); }
        std::vector<PackPiece> pieces;
        int64_t ntiles = 0;
        if (trunc_plan_pieces((int)len.size(), s.data(), d.data(), len.data(), typesize, pieces, &ntiles)) return ERR_INVALID_PARAM;
        if (pieces.empty()) return 0;
        TruncArgs a{pieces.data(), (int32_t)pieces.size(), (int32_t)ntiles, mask64, typesize, 0};
        for (int64_t t = 0; t < ntiles; t++) trunc_wave(a, (int)t);
        return 0;
    }
};

// units of more than one item the last strided call ran, by schedule
struct EmuScheduleStats { int64_t disjoint_units = 0, ordered_units = 0; };

// = cimg_update_windows_strided_device
inline int emu_update_strided_device(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp,
                                     const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                     const int32_t* destsize, int nwindows, const StridedWindowSpec* w, const uint8_t* src, uint8_t* newbuf,
                                     const int64_t* new_off, int32_t* new_cbytes, int32_t* status, UpdateStats* stats,
                                     EmuScheduleStats* sched = nullptr)
{
    EmuStridedUpdateEnv env{{{wf, comp, comp_off, comp_size, nbytes, blocksize, {}}, cf, src, newbuf, {}, {}, {}}, 0, 0};
    const int rc = run_update(env, p, nchunks, comp_off, comp_size, nbytes, blocksize, destsize, nwindows, w, new_off, new_cbytes, status, stats);
    if (sched) { sched->disjoint_units = env.disjoint_units; sched->ordered_units = env.ordered_units; }
    return rc;
}

// = cimg_update_windows_strided_host: staged into buffers that end at their last used byte, as emu_update_host does
inline int emu_update_strided_host(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp,
                                   const int64_t* comp_off, const int32_t* comp_size, const int32_t* destsize, int nwindows,
                                   const StridedWindowSpec* w, const uint8_t* src, void* (*alloc)(void*, size_t), void* user,
                                   void** new_chunks, int32_t* new_cbytes, int32_t* status, UpdateStats* stats,
                                   EmuScheduleStats* sched = nullptr)
{
    *stats = UpdateStats{};
    int rc = open_update_call(nchunks, nwindows, status, new_cbytes, new_chunks);
    if (rc) return rc > 0 ? 0 : rc;
    if (nchunks == 0 || !alloc) return ERR_INVALID_PARAM;
    UpdateHostPlan hp;
    std::vector<StridedWindowSpec> dw;
    if ((rc = plan_update_host(p.typesize, nchunks, comp, comp_off, comp_size, destsize, nwindows, w, status, &hp, &dw)) < 0) return rc;
    std::vector<uint8_t> sc((size_t)hp.comp_used), ss((size_t)hp.rows_used), newbuf((size_t)hp.new_used, 0);
    for (int i = 0; i < nchunks; i++) if (hp.up[(size_t)i]) memcpy(sc.data() + hp.d_comp_off[(size_t)i], comp + comp_off[i], (size_t)hp.up[(size_t)i]);
    for (int k = 0; k < nwindows; k++) {
        const StridedWindowSpec& d = dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(ss.data() + d.out_off, d.out_pitch, src + w[k].out_off, w[k].out_pitch, d.out_pitch, w[k].height);
    }
    rc = emu_update_strided_device(wf, cf, p, nchunks, sc.data(), hp.d_comp_off.data(), hp.held.data(), hp.nbytes.data(), hp.blocksize.data(),
                                   destsize, nwindows, dw.data(), ss.data(), newbuf.data(), hp.new_off.data(), new_cbytes, status, stats, sched);
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
