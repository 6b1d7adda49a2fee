// tests/emu/window_grouped_env.h -- TEST INFRASTRUCTURE: a grouped window call (csrc/window_plan.h: run_windows_grouped) with the
// grouped window kernel's body (csrc/window_kernel.h: GroupedWindowBlock) on the host lane emulator.  Shared by
// window_grouped_emu.cpp (tests/test_emu_windows_grouped.py) and mock_window_grouped.cpp (the Python module's mock backend), over
// window_env.h's chunk handling.  The four waves of a workgroup write in a test-selected order (g_emu_write_order), since the
// kernel lets them run free after its one barrier.
#pragma once
#include "window_strided_env.h"

namespace cimg {

struct EmuGroupedWindowEnv : EmuChunks {
    uint8_t* out;
    int32_t typesize;

    int run_units(const StridedWindowPlan& plan, const std::vector<StridedWindowItem>& items, const std::vector<int32_t>& order,
                  const std::vector<WindowUnit>& units, int32_t* status)
    {
        const int nchunks = (int)plan.descs.size();
        std::vector<ChunkDesc> descs = plan.descs;
        for (int i = 0; i < nchunks; i++) {
            descs[(size_t)i].comp_off = plan.touched[(size_t)i] ? comp_off[i] : 0;
            descs[(size_t)i].destsize = comp_size ? comp_size[i] : 0x7fffffff;
        }
        std::vector<int32_t> st((size_t)nchunks, 0);
        // (the tables as exact allocations of their own, for the sanitizers)
        std::vector<StridedWindowItem> it;
        it.reserve(items.size());
        for (const int32_t k : order) it.push_back(items[(size_t)k]);
        const std::vector<WindowUnit> un(units.begin(), units.end());
        GroupedWindowArgs ga{};
        ga.w.d = DecodeArgs{descs.data(), nchunks, comp, out, st.data(), plan.lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        ga.w.whole = whole.data();
        ga.w.out = out;
        ga.w.typesize = typesize;
        ga.w.nitems = (int32_t)it.size();
        ga.items = it.data();
        ga.units = un.data();
        ga.nunits = (int32_t)un.size();
        std::vector<uint8_t> lds((size_t)plan.lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < ga.nunits; k++) {
            memset(lds.data(), 0xCD, lds.size());
            GroupedWindowBlock gb(ga, lds.data(), k);
            GroupedWindowBlock g0 = gb, g1 = gb, g2 = gb, g3 = gb;       // each wave keeps its own copy of the uniform walk
            GroupedWindowBlock* gs[4] = {&g0, &g1, &g2, &g3};
            for (int w = 0; w < 4; w++) gs[w]->phase_a(w);
            for (int i = 0; i < 4; i++) {
                const int w = g_emu_write_order == 1 ? 3 - i : g_emu_write_order == 2 ? (i * 3 + 2) & 3 : i;
                gs[w]->phase_w(w);
            }
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }
};

// cimg_decompress_windows_grouped_device
inline int emu_windows_grouped_device(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                                      const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows,
                                      const StridedWindowSpec* w, uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    const int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    if (typesize <= 0 || typesize > 255) return ERR_INVALID_PARAM;
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    EmuGroupedWindowEnv env{{fn, comp, comp_off, comp_size, nbytes, blocksize, {}}, out, typesize};
    return run_windows_grouped(env, nchunks, nbytes, blocksize, ts.data(), nwindows, w, {}, status, stats);
}

// cimg_decompress_windows_grouped_host: staged into buffers that end at their last used byte, as emu_windows_host does
inline int emu_windows_grouped_host(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                                    int nwindows, const StridedWindowSpec* w, uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    WindowHostPlan hp;
    std::vector<StridedWindowSpec> dw;
    if ((rc = plan_windows_host(nchunks, comp, comp_off, comp_size, nwindows, w, status, &hp, &dw)) < 0) return rc;
    std::vector<uint8_t> sc((size_t)hp.comp_used), so((size_t)hp.rows_used, 0);
    for (int i = 0; i < nchunks; i++) if (hp.up[(size_t)i]) memcpy(sc.data() + hp.d_comp_off[(size_t)i], comp + comp_off[i], (size_t)hp.up[(size_t)i]);
    EmuGroupedWindowEnv env{{fn, sc.data(), hp.d_comp_off.data(), hp.cbytes.data(), hp.nbytes.data(), hp.blocksize.data(), {}}, so.data(), 0};
    rc = run_windows_grouped(env, nchunks, hp.nbytes.data(), hp.blocksize.data(), hp.typesize.data(), nwindows, dw.data(), hp.hint, status, stats);
    stats->comp_bytes_uploaded = hp.comp_bytes_uploaded;
    if (rc == ERR_INVALID_PARAM) return rc;
    for (int k = 0; k < nwindows; k++) {
        const StridedWindowSpec& d = dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(out + w[k].out_off, w[k].out_pitch, so.data() + d.out_off, d.out_pitch, d.out_pitch, w[k].height);
    }
    return rc;
}

}  // namespace cimg
