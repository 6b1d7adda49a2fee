// tests/emu/window_write_strided_emu.cpp -- TEST INFRASTRUCTURE: strided window writes (csrc/update_plan.h over StridedWindowSpec,
// csrc/update_kernel.h: StridedPatchBlock) on the host lane emulator.  This file INCLUDES window_write_emu.cpp -- one translation
// unit, so that the strided calls fill the stats its wwemu_update_stats reports and the plain calls of the same library serve as
// the col_pitch 1 comparison -- and is linked with emu.cpp and wide_emu.cpp in its place (tests/_window_writes_strided.py).
#include "window_write_emu.cpp"
#include "window_write_strided_env.h"

extern "C" {

static EmuScheduleStats g_wwsemu_sched;

// = cimg_update_windows_strided_device
int wwsemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                         const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const StridedWindowSpec* w,
                         const uint8_t* src, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    g_wwsemu_sched = EmuScheduleStats{};
    return emu_update_strided_device(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, nbytes,
                                     blocksize, destsize, nwindows, w, src, newbuf, new_off, new_cbytes, status, &g_wwemu_stats, &g_wwsemu_sched);
}

// = cimg_update_windows_strided_host (alloc: malloc; the caller frees with wwemu_free)
int wwsemu_update_host(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                       const int32_t* destsize, int nwindows, const StridedWindowSpec* w, const uint8_t* src, void** new_chunks,
                       int32_t* new_cbytes, int32_t* status)
{
    g_wwsemu_sched = EmuScheduleStats{};
    return emu_update_strided_host(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, destsize,
                                   nwindows, w, src, wwemu_alloc, nullptr, new_chunks, new_cbytes, status, &g_wwemu_stats, &g_wwsemu_sched);
}

// units of more than one item in the last strided call: out[0] disjoint, out[1] ordered
void wwsemu_schedule_stats(int64_t* out)
{
    out[0] = g_wwsemu_sched.disjoint_units; out[1] = g_wwsemu_sched.ordered_units;
}

}  // extern "C"
