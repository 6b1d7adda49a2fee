// tests/emu/window_grouped_emu.cpp -- TEST INFRASTRUCTURE: grouped window calls (csrc/window_plan.h: group_items,
// run_windows_grouped; csrc/window_kernel.h: GroupedWindowBlock) on the host lane emulator.  This file INCLUDES
// window_strided_emu.cpp (which includes window_emu.cpp) -- one translation unit, so that the grouped calls fill the stats
// wnemu_window_stats reports, as cimg_engine_window_stats does for every kind of call -- and is linked with emu.cpp and wide_emu.cpp
// in its place (tests/_windows_grouped.py builds the three into one library).
#include "window_strided_emu.cpp"
#include "window_grouped_env.h"

extern "C" {

// = cimg_decompress_windows_grouped_device
int wnemu_windows_grouped_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const StridedWindowSpec* w, uint8_t* out,
                                 int32_t* status)
{
    return emu_windows_grouped_device(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w,
                                      out, status, &g_wnemu_stats);
}

// = cimg_decompress_windows_grouped_host
int wnemu_windows_grouped_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                               const StridedWindowSpec* w, uint8_t* out, int32_t* status)
{
    return emu_windows_grouped_host(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nwindows, w, out, status, &g_wnemu_stats);
}

// the grouping on its own: items given by their block (b[k]; < 0: copy mode) -> the sorted order (order[k]: the item's index in
// the input) and the units; returns the number of units
int wnemu_group_items(int nitems, const int32_t* b, int32_t* order, int32_t* unit_item0, int32_t* unit_nitems)
{
    std::vector<StridedWindowItem> items((size_t)nitems);
    for (int k = 0; k < nitems; k++) { items[(size_t)k] = StridedWindowItem{}; items[(size_t)k].b = b[k]; items[(size_t)k].r0 = k; }
    std::vector<WindowUnit> units;
    std::vector<int32_t> ord;
    group_items(items, &ord, &units);
    for (int k = 0; k < nitems; k++) order[k] = ord[(size_t)k];
    for (size_t u = 0; u < units.size(); u++) { unit_item0[u] = units[u].item0; unit_nitems[u] = units[u].nitems; }
    return (int)units.size();
}

}  // extern "C"
