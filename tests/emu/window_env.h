// tests/emu/window_env.h -- TEST INFRASTRUCTURE: a window call (csrc/window_plan.h: run_windows) with the window kernel's body
// (csrc/window_kernel.h) on the host lane emulator.  Shared by window_emu.cpp (tests/test_emu_windows.py) and mock_window.cpp (the
// Python module's mock backend); each hands in the batch decoder that takes the chunks decoded whole.
#pragma once
#ifndef CIMG_EMULATE
#define CIMG_EMULATE 1
#endif
#include "window_plan.h"
#include <cstring>
#include <vector>

#ifndef EMU_LDS_SLACK
#define EMU_LDS_SLACK 64
#endif

namespace cimg {

// the batch path over some chunks (comp_size may be null): what the engine's decode_whole calls
typedef int (*EmuWholeFn)(int n, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);

struct EmuWindowEnv {
    EmuWholeFn whole_fn;
    const uint8_t* comp;
    const int64_t* comp_off;
    const int32_t* comp_size;
    const int32_t* nbytes;
    const int32_t* blocksize;
    uint8_t* out;
    int32_t typesize;
    std::vector<uint8_t> scratch;

    int decode_whole(const std::vector<int>& list, const std::vector<int64_t>& dst_off, int64_t total, int32_t* st)
    {
        scratch.assign((size_t)total + 64, 0xEE);
        const size_t n = list.size();
        std::vector<int64_t> co(n);
        std::vector<int32_t> cs(n), nb(n), bs(n);
        for (size_t k = 0; k < n; k++) {
            const int i = list[k];
            co[k] = comp_off[i]; cs[k] = comp_size ? comp_size[i] : 0x7fffffff; nb[k] = nbytes[i]; bs[k] = blocksize[i];
        }
        const int rc = whole_fn((int)n, comp, co.data(), comp_size ? cs.data() : nullptr, nb.data(), bs.data(), scratch.data(), dst_off.data(), st);
        if (rc < 0) {
            bool any = false;
            for (size_t k = 0; k < n; k++) any |= st[k] != 0;
            if (!any) for (size_t k = 0; k < n; k++) st[k] = rc;
        }
        return 0;
    }

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
        wa.whole = scratch.data();
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
    if (nchunks < 0 || nwindows < 0) return ERR_INVALID_PARAM;
    for (int i = 0; i < nchunks; i++) status[i] = 0;
    if (nwindows == 0) return 0;
    if (nchunks == 0 || typesize <= 0 || typesize > 255) return ERR_INVALID_PARAM;
    std::vector<int32_t> ts((size_t)nchunks, typesize);
    EmuWindowEnv env{fn, comp, comp_off, comp_size, nbytes, blocksize, out, typesize, {}};
    return run_windows(env, nchunks, nbytes, blocksize, ts.data(), nwindows, w, {}, status, stats);
}

// cimg_decompress_windows_host: the headers read on the host, zstd chunks known up front, the touched chunks' bytes counted
inline int emu_windows_host(EmuWholeFn fn, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                            int nwindows, const WindowSpec* w, uint8_t* out, int32_t* status, WindowStats* stats)
{
    *stats = WindowStats{};
    if (nchunks < 0 || nwindows < 0) return ERR_INVALID_PARAM;
    for (int i = 0; i < nchunks; i++) status[i] = 0;
    if (nwindows == 0) return 0;
    if (nchunks == 0) return ERR_INVALID_PARAM;
    std::vector<uint8_t> named((size_t)nchunks, 0), hint((size_t)nchunks, 0);
    for (int k = 0; k < nwindows; k++) {
        if (w[k].chunk_first < 0 || w[k].chunk_count < 1 || w[k].chunk_first > nchunks - w[k].chunk_count) return ERR_INVALID_PARAM;
        for (int i = w[k].chunk_first; i < w[k].chunk_first + w[k].chunk_count; i++) named[(size_t)i] = 1;
    }
    std::vector<int32_t> nb((size_t)nchunks, 0), bs((size_t)nchunks, 1), ts((size_t)nchunks, 0), cb((size_t)nchunks, 0);
    std::vector<int> version((size_t)nchunks, 0);
    for (int i = 0; i < nchunks; i++) {
        if (!named[(size_t)i]) continue;
        if (comp_size && comp_size[i] < HEADER_LEN) return ERR_READ_BUFFER;
        const uint8_t* c = comp + comp_off[i];
        memcpy(&nb[(size_t)i], c + OFF_NBYTES, 4); memcpy(&bs[(size_t)i], c + OFF_BLOCKSIZE, 4); memcpy(&cb[(size_t)i], c + OFF_CBYTES, 4);
        ts[(size_t)i] = c[OFF_TYPESIZE];
        version[(size_t)i] = c[0];
        hint[(size_t)i] = (c[OFF_FLAGS] >> 5) == 4 && !(c[OFF_FLAGS] & FLAG_MEMCPYED);
    }
    WindowPlan plan;
    int rc = plan_windows(nchunks, nb.data(), bs.data(), ts.data(), nwindows, w, hint.data(), &plan);
    if (rc < 0) return rc;
    int64_t uploaded = 0;
    for (int i = 0; i < nchunks; i++) {
        if (!plan.touched[(size_t)i]) continue;
        int code = 0;
        if (version[(size_t)i] > 5) code = ERR_VERSION_SUPPORT;
        else if (cb[(size_t)i] < HEADER_LEN) code = ERR_INVALID_HEADER;
        else if (comp_size && cb[(size_t)i] > comp_size[i]) code = ERR_READ_BUFFER;
        if (code) { status[i] = code; return code; }
        uploaded += cb[(size_t)i];
    }
    EmuWindowEnv env{fn, comp, comp_off, cb.data(), nb.data(), bs.data(), out, 0, {}};
    rc = run_windows(env, nchunks, nb.data(), bs.data(), ts.data(), nwindows, w, hint, status, stats);
    stats->comp_bytes_uploaded = uploaded;
    return rc;
}

}  // namespace cimg
