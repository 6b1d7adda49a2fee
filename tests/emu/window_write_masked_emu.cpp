// tests/emu/window_write_masked_emu.cpp -- TEST INFRASTRUCTURE: masked and constant window writes (csrc/update_plan.h over
// MaskedWindowSpec, csrc/update_kernel.h: MaskedPatchBlock) on the host lane emulator.  This file INCLUDES window_write_typed_emu.cpp
// (which includes the strided and the plain write emulators) -- one translation unit, so that the masked calls fill the stats
// wwemu_update_stats and wwsemu_schedule_stats report and the strided calls of the same library serve as the flags == 0 comparison
// -- and is linked with emu.cpp and wide_emu.cpp in its place (tests/_window_writes_masked.py builds the three into one library).
#include "window_write_typed_emu.cpp"
#include "window_write_masked_env.h"

extern "C" {

// = cimg_update_windows_masked_device
int wwmemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                         const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const MaskedWindowSpec* w,
                         const uint8_t* src, const uint8_t* mask, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes,
                         int32_t* status)
{
    g_wwsemu_sched = EmuScheduleStats{};
    return emu_update_masked_device(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, nbytes,
                                    blocksize, destsize, nwindows, w, src, mask, newbuf, new_off, new_cbytes, status, &g_wwemu_stats,
                                    &g_wwsemu_sched);
}

// = cimg_update_windows_masked_host (alloc: malloc; the caller frees with wwemu_free)
int wwmemu_update_host(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                       const int32_t* destsize, int nwindows, const MaskedWindowSpec* w, const uint8_t* src, const uint8_t* mask,
                       void** new_chunks, int32_t* new_cbytes, int32_t* status)
{
    g_wwsemu_sched = EmuScheduleStats{};
    return emu_update_masked_host(wemu_decompress_batch, wemu_compress_batch, host_params(p), nchunks, comp, comp_off, comp_size, destsize,
                                  nwindows, w, src, mask, wwemu_alloc, nullptr, new_chunks, new_cbytes, status, &g_wwemu_stats, &g_wwsemu_sched);
}

}  // extern "C"
