// tests/emu/stored_emu.cpp -- TEST INFRASTRUCTURE: the emulated encode batch of emu.cpp plus a view of what became of its stored
// planes.  A plane that comes out stored in a chunk assembled inside the encode launch is not written to the scratch slot: its record
// says REC_RAW_SRC and the wave that places it selects it from the launch's input again (encode_kernel.h: encode_resident).  The
// counters tell a test that this path -- and not the scratch path, which gives the same bytes -- produced the chunks it compares.
// Built by tests/test_emu_stored_planes.py into a library of its own; never linked into libcimg_hip.so.
#include "emu.cpp"

extern "C" {

// out[0]: streams left as REC_RAW_SRC, out[1]: streams placed from the source, since the last call
void emu_stored_stats(long* out)
{
    out[0] = cimg::g_emu_src_left; out[1] = cimg::g_emu_src_placed;
    cimg::g_emu_src_left = 0; cimg::g_emu_src_placed = 0;
}

// the batch of emu_compress_batch with every chunk at a caller-chosen address (comp_off may be odd: bstarts[] off a 4-byte
// boundary takes the fenced branch of the in-launch layout)
int emu_stored_compress_batch(const EmuCParams* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                              uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes, long* stats)
{
    long drop[2];
    emu_stored_stats(drop);
    const int rc = emu_compress_batch(p, nchunks, raw, raw_off, nbytes, comp, comp_off, destsize, cbytes);
    emu_stored_stats(stats);
    return rc;
}

}
