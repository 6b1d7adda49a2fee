// tests/emu/window_typed_emu.cpp -- TEST INFRASTRUCTURE: typed window calls (csrc/window_plan.h: run_windows_typed;
// csrc/window_kernel.h: TypedWindowBlock) on the host lane emulator.  This file INCLUDES window_grouped_emu.cpp (which includes the
// strided and the plain window emulators) -- one translation unit, so that the typed calls fill the stats wnemu_window_stats
// reports and the grouped call is at hand to compare with -- and is linked with emu.cpp and wide_emu.cpp in its place
// (tests/_windows_typed.py builds the three into one library, this file with -ffp-contract=off).
#include "window_grouped_emu.cpp"
#include "window_typed_env.h"

extern "C" {

// = cimg_decompress_windows_typed_device
int wnemu_windows_typed_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                               const int32_t* blocksize, int typesize, int nwindows, const TypedWindowSpec* w, uint8_t* out, int32_t* status)
{
    return emu_windows_typed_device(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w, out,
                                    status, &g_wnemu_stats);
}

// the order of a typed launch's units on its own: the decode units' first output addresses, in launch order; returns their count
int wnemu_typed_unit_order(int nchunks, const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows, const TypedWindowSpec* w,
                           int64_t* first_out, int max_units)
{
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    TypedWindowPlan plan;
    const int rc = plan_windows(nchunks, nbytes, blocksize, ts.data(), nwindows, w, nullptr, &plan);
    if (rc < 0) return rc;
    std::vector<int32_t> order;
    std::vector<WindowUnit> units;
    group_items(plan.items, &order, &units);
    order_units_by_output(plan.items, order, &units);
    int n = 0;
    for (const WindowUnit& u : units) {
        const TypedWindowItem& t = plan.items[(size_t)order[(size_t)u.item0]];
        if (t.b < 0 || n >= max_units) break;
        const int64_t rel = t.row0 + (int64_t)t.r0 * t.rpitch - t.p0;
        first_out[n++] = t.out_off + (int64_t)t.r0 * t.out_pitch + (rel >= 0 ? 0 : (-rel + t.cpitch - 1) / t.cpitch) * t.epitch;
    }
    return n;
}

}  // extern "C"
