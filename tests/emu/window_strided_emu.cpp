// tests/emu/window_strided_emu.cpp -- TEST INFRASTRUCTURE: strided window calls (csrc/window_plan.h, csrc/window_kernel.h) on the
// host lane emulator.  This file INCLUDES window_emu.cpp -- one translation unit, so that the strided calls fill the stats
// wnemu_window_stats reports, as cimg_engine_window_stats does for both kinds of call -- and is linked with emu.cpp and wide_emu.cpp
// in its place (tests/test_emu_windows_strided.py builds the three into one library).
#include "window_emu.cpp"
#include "window_strided_env.h"

extern "C" {

// = cimg_decompress_windows_strided_device
int wnemu_windows_strided_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const StridedWindowSpec* w, uint8_t* out,
                                 int32_t* status)
{
    return emu_windows_strided_device(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nbytes, blocksize, typesize, nwindows, w,
                                      out, status, &g_wnemu_stats);
}

// = cimg_decompress_windows_strided_host
int wnemu_windows_strided_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                               const StridedWindowSpec* w, uint8_t* out, int32_t* status)
{
    return emu_windows_strided_host(wemu_decompress_batch, nchunks, comp, comp_off, comp_size, nwindows, w, out, status, &g_wnemu_stats);
}

}  // extern "C"
