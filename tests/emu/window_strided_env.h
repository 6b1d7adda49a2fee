// tests/emu/window_strided_env.h -- TEST INFRASTRUCTURE: a strided window call (csrc/window_plan.h: run_windows over
// StridedWindowSpec) with the strided window kernel's body (csrc/window_kernel.h: StridedWindowBlock) on the host lane emulator.
// Shared by window_strided_emu.cpp (tests/test_emu_windows_strided.py) and mock_window_strided.cpp (the Python module's mock
// backend), over window_env.h's chunk handling.
#pragma once
#include "window_env.h"

namespace cimg {

struct EmuStridedWindowEnv : EmuChunks {
    uint8_t* out;
    int32_t typesize;

    int run_items(const StridedWindowPlan& plan, const std::vector<StridedWindowItem>& items, int32_t* status)
    {
        const int nchunks = (int)plan.descs.size();
        std::vector<ChunkDesc> descs = plan.descs;
        for (int i = 0; i < nchunks; i++) {
            descs[(size_t)i].comp_off = plan.touched[(size_t)i] ? comp_off[i] : 0;
            descs[(size_t)i].destsize = comp_size ? comp_size[i] : 0x7fffffff;
        }
        std::vector<int32_t> st((size_t)nchunks, 0);
        StridedWindowArgs sa{};
        sa.w.d = DecodeArgs{descs.data(), nchunks, comp, out, st.data(), plan.lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        sa.w.whole = whole.data();
        sa.w.out = out;
        sa.w.typesize = typesize;
        sa.w.nitems = (int32_t)items.size();
        sa.items = items.data();
        std::vector<uint8_t> lds((size_t)plan.lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)items.size(); k++) {
            memset(lds.data(), 0xCD, lds.size());
            StridedWindowBlock wb(sa, lds.data(), k);
            StridedWindowBlock w0 = wb, w1 = wb, w2 = wb, w3 = wb;       // each wave keeps its own copy of the uniform walk
            StridedWindowBlock* ws[4] = {&w0, &w1, &w2, &w3};
            for (int w = 0; w < 4; w++) ws[w]->phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->phase_w(w);
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }
};

// cimg_decompress_windows_strided_device
inline int emu_windows_strided_device(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                                      const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows,
                                      const StridedWindowSpec* w, uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    const int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    if (typesize <= 0 || typesize > 255) return ERR_INVALID_PARAM;
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    EmuStridedWindowEnv env{{fn, comp, comp_off, comp_size, nbytes, blocksize, {}}, out, typesize};
    return run_windows(env, nchunks, nbytes, blocksize, ts.data(), nwindows, w, {}, status, stats);
}

// cimg_decompress_windows_strided_host: staged into buffers that end at their last used byte, as emu_windows_host does
inline int emu_windows_strided_host(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
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
    EmuStridedWindowEnv env{{fn, sc.data(), hp.d_comp_off.data(), hp.cbytes.data(), hp.nbytes.data(), hp.blocksize.data(), {}}, so.data(), 0};
    rc = run_windows(env, nchunks, hp.nbytes.data(), hp.blocksize.data(), hp.typesize.data(), nwindows, dw.data(), hp.hint, status, stats);
    stats->comp_bytes_uploaded = hp.comp_bytes_uploaded;
    if (rc == ERR_INVALID_PARAM) return rc;
    for (int k = 0; k < nwindows; k++) {
        const StridedWindowSpec& d = dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(out + w[k].out_off, w[k].out_pitch, so.data() + d.out_off, d.out_pitch, d.out_pitch, w[k].height);
    }
    return rc;
}

}  // namespace cimg
