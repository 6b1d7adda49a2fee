// tests/emu/window_write_typed_emu.cpp -- TEST INFRASTRUCTURE: typed window writes (csrc/update_plan.h over TypedWindowSpec,
// csrc/update_kernel.h: TypedPatchBlock) on the host lane emulator.  This file INCLUDES window_write_strided_emu.cpp (which includes
// the plain write emulator) -- one translation unit, so that the typed call fills the stats wwemu_update_stats and
// wwsemu_schedule_stats report and the strided call of the same library serves as the identity comparison -- and is linked with
// emu.cpp and wide_emu.cpp in its place (tests/_window_writes_typed.py builds the three into one library, with -ffp-contract=off).
#include "window_write_strided_emu.cpp"
#include "window_write_typed_env.h"

extern "C" {

// = cimg_update_windows_typed_device
int wwtemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                         const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const TypedWindowSpec* w,
                         const uint8_t* src, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes, int32_t* status)
{
    g_wwsemu_sched = EmuScheduleStats{};
    return emu_update_typed_device(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, nbytes,
                                   blocksize, destsize, nwindows, w, src, newbuf, new_off, new_cbytes, status, &g_wwemu_stats, &g_wwsemu_sched);
}

}  // extern "C"
