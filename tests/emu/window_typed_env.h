// tests/emu/window_typed_env.h -- TEST INFRASTRUCTURE: a typed window call (csrc/window_plan.h: run_windows_typed) with the typed
// window kernel's body (csrc/window_kernel.h: TypedWindowBlock) on the host lane emulator.  Shared by window_typed_emu.cpp
// (tests/test_emu_windows_typed.py) and mock_window_typed.cpp (the Python module's mock backend), over window_env.h's chunk
// handling.  The four waves of a workgroup write in a test-selected order (g_emu_write_order), as in window_grouped_env.h.  The
// translation unit that includes this is built with -ffp-contract=off: the kernel's multiply and add are two roundings.
#pragma once
#include "window_grouped_env.h"

namespace cimg {

struct EmuTypedWindowEnv : EmuChunks {
    uint8_t* out;
    int32_t typesize;

    int run_typed_units(const TypedWindowPlan& plan, const std::vector<TypedWindowItem>& items, const std::vector<int32_t>& order,
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
        std::vector<TypedWindowItem> it;
        it.reserve(items.size());
        for (const int32_t k : order) it.push_back(items[(size_t)k]);
        const std::vector<WindowUnit> un(units.begin(), units.end());
        TypedWindowArgs ta{};
        ta.w.d = DecodeArgs{descs.data(), nchunks, comp, out, st.data(), plan.lds_bytes, nullptr, 0, nullptr, 0, nullptr, 0, 0, 1, 0};
        ta.w.whole = whole.data();
        ta.w.out = out;
        ta.w.typesize = typesize;
        ta.w.nitems = (int32_t)it.size();
        ta.items = it.data();
        ta.units = un.data();
        ta.nunits = (int32_t)un.size();
        std::vector<uint8_t> lds((size_t)plan.lds_bytes + EMU_LDS_SLACK);
        for (int k = 0; k < ta.nunits; k++) {
            memset(lds.data(), 0xCD, lds.size());
            TypedWindowBlock tb(ta, lds.data(), k);
            TypedWindowBlock t0 = tb, t1 = tb, t2 = tb, t3 = tb;         // each wave keeps its own copy of the uniform walk
            TypedWindowBlock* ts[4] = {&t0, &t1, &t2, &t3};
            for (int w = 0; w < 4; w++) ts[w]->phase_a(w);
            for (int i = 0; i < 4; i++) {
                const int w = g_emu_write_order == 1 ? 3 - i : g_emu_write_order == 2 ? (i * 3 + 2) & 3 : i;
                ts[w]->phase_w(w);
            }
        }
        for (int i = 0; i < nchunks; i++) if (st[(size_t)i] != 0 && status[i] == 0) status[i] = st[(size_t)i];
        return 0;
    }
};

// cimg_decompress_windows_typed_device (the engine also asks that `out` itself is a multiple of every output size)
inline int emu_windows_typed_device(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                                    const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows, const TypedWindowSpec* w,
                                    uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    const int rc = open_window_call(nchunks, nwindows, status);
    if (rc) return rc > 0 ? 0 : rc;
    if (typesize <= 0 || typesize > 255) return ERR_INVALID_PARAM;
    for (int k = 0; k < nwindows; k++)
        if (type_size(w[k].out_type) && (uintptr_t)out % (uintptr_t)type_size(w[k].out_type)) return ERR_INVALID_PARAM;
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    EmuTypedWindowEnv env{{fn, comp, comp_off, comp_size, nbytes, blocksize, {}}, out, typesize};
    return run_windows_typed(env, nchunks, nbytes, blocksize, ts.data(), nwindows, w, {}, status, stats);
}

}  // namespace cimg
