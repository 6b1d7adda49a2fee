// tests/emu/window_write_typed_env.h -- TEST INFRASTRUCTURE: a typed update call (csrc/update_plan.h: check_typed_update, then
// run_update over TypedWindowSpec) with the body of cimg_update_patch_typed (csrc/update_kernel.h: TypedPatchBlock) on the host lane
// emulator, over window_write_strided_env.h's trunc step and window_write_env.h's encode, splice and compress steps.  Shared by
// window_write_typed_emu.cpp (tests/test_emu_window_writes_typed.py) and mock_window_write_typed.cpp (the Python module's mock
// backend).  Schedules as in window_write_strided_env.h: the four waves write a DISJOINT unit in a test-selected order
// (g_emu_write_order); an ordered unit runs item after item.  The translation unit that includes this is built with
// -ffp-contract=off: the kernel's subtraction and division are two roundings.
#pragma once
#include "window_write_strided_env.h"

namespace cimg {

struct EmuTypedUpdateEnv : EmuStridedUpdateEnv {
    int patch_typed(const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<StridedPatchUnit>& units,
                    const std::vector<WindowItem>& stage, const std::vector<TypedWindowItem>& items, int to_whole, int64_t patch_bytes,
                    int32_t* status)
    {
        if (!to_whole) patchbuf.assign((size_t)patch_bytes + 64, 0xEE);
        const int nchunks = (int)descs.size();
        std::vector<int32_t> st((size_t)nchunks, 0);
        // (the tables as exact allocations of their own, for the sanitizers)
        const std::vector<StridedPatchUnit> un(units.begin(), units.end());
        const std::vector<TypedWindowItem> it(items.begin(), items.end());
        const std::vector<WindowItem> sg(stage.begin(), stage.end());
        TypedPatchArgs ta{};
        ta.p.w.d = DecodeArgs{descs.data(), nchunks, comp, nullptr, st.data(), lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        ta.p.w.items = sg.data();
        ta.p.w.nitems = (int32_t)sg.size();
        ta.p.src = src;
        ta.p.dst = to_whole ? whole.data() : patchbuf.data();
        ta.p.nunits = (int32_t)un.size();
        ta.units = un.data();
        ta.items = it.data();
        std::vector<uint8_t> lds((size_t)lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)un.size(); k++) {
            if (!lds.empty()) memset(lds.data(), 0xCD, lds.size());      // (a launch over chunks decoded whole has no LDS)
            TypedPatchBlock tb(ta, lds.data(), k);
            TypedPatchBlock t0 = tb, t1 = tb, t2 = tb, t3 = tb;         // each wave keeps its own copy of the uniform walk
            TypedPatchBlock* ws[4] = {&t0, &t1, &t2, &t3};
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->pb.phase_base(w);
            const int n = tb.pb.u.nitems;
            if (n == 1) {
                for (int w = 0; w < 4; w++) ws[w]->overlay(0, w * 64, 256);
            } else if (tb.disjoint) {
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

// = cimg_update_windows_typed_device: the typed checks before status or new_cbytes are touched, then the strided call's course
inline int emu_update_typed_device(EmuWholeFn wf, EmuCompressFn cf, const HostCParams& p, int nchunks, const uint8_t* comp,
                                   const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                   const int32_t* destsize, int nwindows, const TypedWindowSpec* w, const uint8_t* src, uint8_t* newbuf,
                                   const int64_t* new_off, int32_t* new_cbytes, int32_t* status, UpdateStats* stats,
                                   EmuScheduleStats* sched = nullptr)
{
    if (nchunks > 0 && nwindows > 0 && w && nbytes && blocksize && check_typed_update(nchunks, nbytes, blocksize, p.typesize, nwindows, w, src) < 0) {
        *stats = UpdateStats{};
        return ERR_INVALID_PARAM;
    }
    EmuTypedUpdateEnv env{{{{wf, comp, comp_off, comp_size, nbytes, blocksize, {}}, cf, src, newbuf, {}, {}, {}}, 0, 0}};
    const int rc = run_update(env, p, nchunks, comp_off, comp_size, nbytes, blocksize, destsize, nwindows, w, new_off, new_cbytes, status, stats);
    if (sched) { sched->disjoint_units = env.disjoint_units; sched->ordered_units = env.ordered_units; }
    return rc;
}

}  // namespace cimg
