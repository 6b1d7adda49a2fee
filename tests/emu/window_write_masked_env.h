// tests/emu/window_write_masked_env.h -- TEST INFRASTRUCTURE: a masked / constant update call (csrc/update_plan.h:
// check_masked_update, then run_update over MaskedWindowSpec; plan_update_host for the host form) with the body of
// cimg_update_patch_masked (csrc/update_kernel.h: MaskedPatchBlock) on the host lane emulator, over window_write_strided_env.h's trunc
// step and window_write_env.h's encode, splice and compress steps.  Shared by window_write_masked_emu.cpp
// (tests/test_emu_window_writes_masked.py) and mock_window_write_masked.cpp (the Python module's mock backend).  Schedules as in
// window_write_strided_env.h: the four waves write a DISJOINT unit in a test-selected order (g_emu_write_order); an ordered unit
// runs item after item.  (Waves run one after the other here: a read-modify-write of unit bytes in an overlay would not show.  The
// kernel has none by construction, and the GPU suite holds the case that would expose one.)
#pragma once
#include "window_write_typed_env.h"

namespace cimg {

struct EmuMaskedUpdateEnv : EmuTypedUpdateEnv {
    const uint8_t* mask;

    int patch_masked(const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<StridedPatchUnit>& units,
                     const std::vector<WindowItem>& stage, const std::vector<MaskedWindowItem>& items, int to_whole, int64_t patch_bytes,
                     int32_t* status)
    {
        if (!to_whole) patchbuf.assign((size_t)patch_bytes + 64, 0xEE);
        const int nchunks = (int)descs.size();
        std::vector<int32_t> st((size_t)nchunks, 0);
        // (the tables as exact allocations of their own, for the sanitizers)
        const std::vector<StridedPatchUnit> un(units.begin(), units.end());
        const std::vector<MaskedWindowItem> it(items.begin(), items.end());
        const std::vector<WindowItem> sg(stage.begin(), stage.end());
        MaskedPatchArgs ma{};
        ma.p.w.d = DecodeArgs{descs.data(), nchunks, comp, nullptr, st.data(), lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        ma.p.w.items = sg.data();
        ma.p.w.nitems = (int32_t)sg.size();
        ma.p.src = src;
        ma.p.dst = to_whole ? whole.data() : patchbuf.data();
        ma.p.nunits = (int32_t)un.size();
        ma.units = un.data();
        ma.items = it.data();
        ma.mask = mask;
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)un.size(); k++) {
            if (!lds.empty()) memset(lds.data(), 0xCD, lds.size());      // (a launch over chunks decoded whole has no LDS)
            MaskedPatchBlock mb(ma, lds.data(), k);
            MaskedPatchBlock m0 = mb, m1 = mb, m2 = mb, m3 = mb;        // each wave keeps its own copy of the uniform walk
            MaskedPatchBlock* ws[4] = {&m0, &m1, &m2, &m3};
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_base(w);
            const int n = mb.pb.u.nitems;
            if (n == 1) {
                for (int w = 0; w < 4; w++) ws[w]->overlay(0, w * 64, 256);
            } else if (mb.disjoint) {
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
};

// = cimg_update_windows_masked_device: the masked checks before status or new_cbytes are touched, then the strided call's course
// (checked: false for the inner call of the host form, whose pointers and windows have been checked and re-packed)
inline int emu_update_masked_device(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp,
                                    const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                    const int32_t* destsize, int nwindows, const MaskedWindowSpec* w, const uint8_t* src, const uint8_t* mask,
                                    uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes, int32_t* status, UpdateStats* stats,
                                    EmuScheduleStats* sched = nullptr, bool checked = true)
{
    if (checked && nwindows > 0 && w && check_masked_update(p.typesize, nwindows, w, src, mask) < 0) {
        *stats = UpdateStats{};
        return ERR_INVALID_PARAM;
    }
    EmuMaskedUpdateEnv env{{{{{wf, comp, comp_off, comp_size, nbytes, blocksize, {}}, cf, src, newbuf, {}, {}, {}}, 0, 0}}, mask};
    const int rc = run_update(env, p, nchunks, comp_off, comp_size, nbytes, blocksize, destsize, nwindows, w, new_off, new_cbytes, status, stats);
    if (sched) { sched->disjoint_units = env.disjoint_units; sched->ordered_units = env.ordered_units; }
    return rc;
}

// = cimg_update_windows_masked_host: staged into buffers that end at their last used byte, as emu_update_host does -- the rows of the
// windows that have a source, the mask rows of the masked ones, nothing for a constant unmasked window
inline int emu_update_masked_host(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp,
                                  const int64_t* comp_off, const int32_t* comp_size, const int32_t* destsize, int nwindows,
                                  const MaskedWindowSpec* w, const uint8_t* src, const uint8_t* mask, void* (*alloc)(void*, size_t), void* user,
                                  void** new_chunks, int32_t* new_cbytes, int32_t* status, UpdateStats* stats,
                                  EmuScheduleStats* sched = nullptr)
{
    *stats = UpdateStats{};
    if (nwindows > 0 && w && check_masked_update(p.typesize, nwindows, w, src, mask) < 0) return ERR_INVALID_PARAM;
    int rc = open_update_call(nchunks, nwindows, status, new_cbytes, new_chunks);
    if (rc) return rc > 0 ? 0 : rc;
    if (nchunks == 0 || !alloc) return ERR_INVALID_PARAM;
    UpdateHostPlan hp;
    std::vector<MaskedWindowSpec> dw;
    if ((rc = plan_update_host(p.typesize, nchunks, comp, comp_off, comp_size, destsize, nwindows, w, status, &hp, &dw)) < 0) return rc;
    std::vector<uint8_t> sc((size_t)hp.comp_used), ss((size_t)hp.rows_used), sm((size_t)hp.mask_used), newbuf((size_t)hp.new_used, 0);
    for (int i = 0; i < nchunks; i++) if (hp.up[(size_t)i]) memcpy(sc.data() + hp.d_comp_off[(size_t)i], comp + comp_off[i], (size_t)hp.up[(size_t)i]);
    for (int k = 0; k < nwindows; k++) {
        const MaskedWindowSpec& d = dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(ss.data() + d.out_off, d.out_pitch, src + w[k].out_off, w[k].out_pitch, d.out_pitch, w[k].height);
        if (hp.mbytes[(size_t)k]) copy_rows(sm.data() + d.mask_off, d.mask_pitch, mask + w[k].mask_off, w[k].mask_pitch, d.mask_pitch, w[k].height);
    }
    rc = emu_update_masked_device(wf, cf, p, nchunks, sc.data(), hp.d_comp_off.data(), hp.held.data(), hp.nbytes.data(), hp.blocksize.data(),
                                  destsize, nwindows, dw.data(), ss.data(), sm.data(), newbuf.data(), hp.new_off.data(), new_cbytes, status, stats,
                                  sched, false);
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
