// tests/emu/window_env.h -- TEST INFRASTRUCTURE: a window call (csrc/window_plan.h: run_windows) with the window kernel's body
// (csrc/window_kernel.h) on the host lane emulator.  Shared by window_emu.cpp (tests/test_emu_windows.py) and mock_window.cpp (the
// Python module's mock backend); each hands in the batch decoder that takes the chunks decoded whole.
#pragma once
#ifndef CIMG_EMULATE
#define CIMG_EMULATE 1
#endif
#include "window_plan.h"

#ifndef EMU_LDS_SLACK
#define EMU_LDS_SLACK 64
#endif

namespace cimg {

// the batch path over some chunks (comp_size may be null): what the engine's decode_whole calls
typedef int (*EmuWholeFn)(int n, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);

// the batch a window call runs on, and the step run_windows and run_update share (engine.hip: EngineChunks)
struct EmuChunks {
    EmuWholeFn whole_fn;
    const uint8_t* comp;
    const int64_t* comp_off;
    const int32_t* comp_size;
    const int32_t* nbytes;
    const int32_t* blocksize;
    std::vector<uint8_t> whole;

    int decode_whole(const std::vector<int>& list, const std::vector<int64_t>& dst_off, int64_t total, int32_t* st)
    {
        whole.assign((size_t)total + 64, 0xEE);
        const SubBatch sub(list, comp_off, comp_size, nbytes, blocksize);
        const int rc = whole_fn((int)list.size(), comp, sub.co.data(), comp_size ? sub.cs.data() : nullptr, sub.nb.data(), sub.bs.data(), whole.data(),
                                dst_off.data(), st);
        spread_refusal(rc, list.size(), st);
        return 0;
    }
};

// rows of `row` bytes from one pitch to another: what the engine's host calls do with (2-D) copies over PCIe
inline void copy_rows(uint8_t* dst, int64_t dst_pitch, const uint8_t* src, int64_t src_pitch, int64_t row, int height)
{
    for (int r = 0; r < height; r++) memcpy(dst + r * dst_pitch, src + r * src_pitch, (size_t)row);
}

struct EmuWindowEnv : EmuChunks {
    uint8_t* out;
    int32_t typesize;

    int run_items(const WindowPlan& plan, const std::vector<WindowItem>& items, int32_t* status)
    {
        const int nchunks = (int)plan.descs.size();
        std::vector<ChunkDesc> descs = plan.descs;
        for (int i = 0; i < nchunks; i++) {
            descs[(size_t)i].comp_off = plan.touched[(size_t)i] ? comp_off[i] : 0;
            descs[(size_t)i].destsize = comp_size ? comp_size[i] : 0x7fffffff;
        }
        std::vector<int32_t> st((size_t)nchunks, 0);
        WindowArgs wa{};
        wa.d = DecodeArgs{descs.data(), nchunks, comp, out, st.data(), plan.lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        wa.items = items.data();
        wa.whole = whole.data();
        wa.out = out;
        wa.typesize = typesize;
        wa.nitems = (int32_t)items.size();
        std::vector<uint8_t> lds((size_t)plan.lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < (int)items.size(); k++) {
            memset(lds.data(), 0xCD, lds.size());
            WindowBlock wb(wa, lds.data(), k);
            WindowBlock w0 = wb, w1 = wb, w2 = wb, w3 = wb;       // each wave keeps its own copy of the uniform walk
            WindowBlock* ws[4] = {&w0, &w1, &w2, &w3};
            for (int w = 0; w < 4; w++) ws[w]->phase_a(w);
            for (int w = 0; w < 4; w++) ws[w]->phase_w(w);
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }
};

// cimg_decompress_windows_device: sizes from the caller, every chunk must say `typesize`
inline int emu_windows_device(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                              const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows, const WindowSpec* w,
                              uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    const int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    if (typesize <= 0 || typesize > 255) return ERR_INVALID_PARAM;
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    EmuWindowEnv env{{fn, comp, comp_off, comp_size, nbytes, blocksize, {}}, out, typesize};
    return run_windows(env, nchunks, nbytes, blocksize, ts.data(), nwindows, w, {}, status, stats);
}

// cimg_decompress_windows_host: planned as the engine plans it, staged with memcpy where the engine copies over PCIe -- into buffers
// that end at their last used byte, for the sanitizers
inline int emu_windows_host(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                            int nwindows, const WindowSpec* w, uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    WindowHostPlan hp;
    if ((rc = plan_windows_host(nchunks, comp, comp_off, comp_size, nwindows, w, status, &hp)) < 0) return rc;
    std::vector<uint8_t> sc((size_t)hp.comp_used), so((size_t)hp.rows_used, 0);
    for (int i = 0; i < nchunks; i++) if (hp.up[(size_t)i]) memcpy(sc.data() + hp.d_comp_off[(size_t)i], comp + comp_off[i], (size_t)hp.up[(size_t)i]);
    EmuWindowEnv env{{fn, sc.data(), hp.d_comp_off.data(), hp.cbytes.data(), hp.nbytes.data(), hp.blocksize.data(), {}}, so.data(), 0};
    rc = run_windows(env, nchunks, hp.nbytes.data(), hp.blocksize.data(), hp.typesize.data(), nwindows, hp.dw.data(), hp.hint, status, stats);
    stats->comp_bytes_uploaded = hp.comp_bytes_uploaded;
    if (rc == ERR_INVALID_PARAM) return rc;
    for (int k = 0; k < nwindows; k++) {
        const WindowSpec& d = hp.dw[(size_t)k];
        if (hp.wbytes[(size_t)k]) copy_rows(out + w[k].out_off, w[k].out_pitch, so.data() + d.out_off, d.out_pitch, d.out_pitch, w[k].height);
    }
    return rc;
}

}  // namespace cimg
