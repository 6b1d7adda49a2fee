// tests/emu/special_asan_main.cpp -- TEST INFRASTRUCTURE: special-value chunks (csrc/special_plan.h) through the pattern fill of the
// batch decode (csrc/decode_kernel.h: wave_fill_pattern) and the pattern mode of the window kernels (csrc/window_kernel.h), for the
// AddressSanitizer / UBSan build of emu.cpp, wide_emu.cpp and window_grouped_emu.cpp (tests/test_emu_special_chunks.py).
// Every chunk and every output is a heap allocation of its exact size: a read past a 32 + typesize byte chunk or a store past the
// last pixel is a report.  The chunks are written here from the format; what comes back is compared with the pattern.  Prints
// "special asan ok <cases>" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" {
int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
void emu_set_lean(int on);
int wnemu_windows_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                         const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                       const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_strided_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_grouped_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_grouped_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                               const void* w, uint8_t* out, int32_t* status);
}

struct Win { int32_t chunk_first, chunk_count; int64_t origin, row_pitch; int32_t width, height; int64_t out_off, out_pitch; };
struct SWin { int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch; };

enum { ZERO = 1, NAN_ = 2, VALUE = 3, UNINIT = 4 };

// a chunk in an allocation of exactly its size
struct Chunk {
    std::unique_ptr<uint8_t[]> p;
    int32_t cbytes, nbytes, blocksize, ts;
    int kind;
    Chunk(int kind_, int ts_, int32_t nbytes_, int32_t blocksize_) : cbytes(32 + (kind_ == VALUE ? ts_ : 0)), nbytes(nbytes_), blocksize(blocksize_), ts(ts_), kind(kind_)
    {
        p.reset(new uint8_t[(size_t)cbytes]);
        memset(p.get(), 0, 32);
        p[0] = 5; p[1] = 1; p[2] = 0x01 | 0x04 | 0x10 | (1 << 5); p[3] = (uint8_t)ts;
        memcpy(p.get() + 4, &nbytes, 4); memcpy(p.get() + 8, &blocksize, 4); memcpy(p.get() + 12, &cbytes, 4);
        p[16 + 5] = 1; p[22] = 1;
        p[31] = (uint8_t)(kind << 4);
        for (int k = 0; k < cbytes - 32; k++) p[32 + k] = (uint8_t)(17 + 5 * k);
    }
    uint8_t want(int64_t k) const
    {
        const int i = (int)(k % ts);
        if (kind == VALUE) return (uint8_t)(17 + 5 * i);
        if (kind == NAN_) return i == ts - 1 ? 0x7F : i == ts - 2 ? (ts == 4 ? 0xC0 : 0xF8) : 0;
        return 0;
    }
};

static int g_cases = 0;

static bool batch(const Chunk& c, int mis)
{
    // the output: `mis` bytes of canary, then exactly the pixels
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)c.nbytes + mis]);
    memset(out.get(), 0xA5, (size_t)c.nbytes + mis);
    const int64_t zero = 0, ro = mis;
    int32_t st = 0;
    const int rc = wemu_decompress_batch(1, c.p.get(), &zero, &c.cbytes, &c.nbytes, &c.blocksize, out.get(), &ro, &st);
    if (rc != 0 || st != 0) { printf("batch kind %d ts %d mis %d: rc %d status %d\n", c.kind, c.ts, mis, rc, st); return false; }
    for (int k = 0; k < mis; k++) if (out[k] != 0xA5) { printf("batch kind %d ts %d mis %d: canary byte %d written\n", c.kind, c.ts, mis, k); return false; }
    for (int64_t k = 0; k < c.nbytes; k++)
        if (out[mis + k] != c.want(k)) { printf("batch kind %d ts %d mis %d: byte %lld is %d\n", c.kind, c.ts, mis, (long long)k, out[mis + k]); return false; }
    g_cases++;
    return true;
}

static bool window_result(const Chunk& c, const char* what, int rc, int32_t st, const uint8_t* out, int64_t first, int64_t count, int64_t step)
{
    if (rc != 0 || st != 0) { printf("%s kind %d ts %d: rc %d status %d\n", what, c.kind, c.ts, rc, st); return false; }
    for (int64_t e = 0; e < count; e++)
        for (int b = 0; b < c.ts; b++)
            if (out[e * c.ts + b] != c.want((first + e * step) * c.ts + b)) { printf("%s kind %d ts %d: element %lld byte %d is %d\n", what, c.kind, c.ts, (long long)e, b, out[e * c.ts + b]); return false; }
    g_cases++;
    return true;
}

static bool windows(const Chunk& c)
{
    const int64_t elems = c.nbytes / c.ts, zero = 0;
    int32_t st = 0;
    // the plain call, device and host form: everything from element 1 on (the window starts off every boundary), and the last element
    for (int probe = 0; probe < 2; probe++) {
        const int64_t first = probe ? elems - 1 : 1, count = probe ? 1 : elems - 1;
        const Win w{0, 1, first, count, (int32_t)count, 1, 0, count * c.ts};
        for (int host = 0; host < 2; host++) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(count * c.ts)]);
            const int rc = host ? wnemu_windows_host(1, c.p.get(), &zero, &c.cbytes, 1, &w, out.get(), &st)
                                : wnemu_windows_device(1, c.p.get(), &zero, &c.cbytes, &c.nbytes, &c.blocksize, c.ts, 1, &w, out.get(), &st);
            if (!window_result(c, host ? "window host" : "window device", rc, st, out.get(), first, count, 1)) return false;
        }
    }
    // strided and grouped: every 5th element from element 2 on
    const int64_t first = 2, step = 5, count = (elems - first + step - 1) / step;
    const SWin s{0, 1, first, count, step, (int32_t)count, 1, 0, count * c.ts};
    for (int kind = 0; kind < 3; kind++) {
        std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(count * c.ts)]);
        const int rc = kind == 0 ? wnemu_windows_strided_device(1, c.p.get(), &zero, &c.cbytes, &c.nbytes, &c.blocksize, c.ts, 1, &s, out.get(), &st)
                     : kind == 1 ? wnemu_windows_grouped_device(1, c.p.get(), &zero, &c.cbytes, &c.nbytes, &c.blocksize, c.ts, 1, &s, out.get(), &st)
                                 : wnemu_windows_grouped_host(1, c.p.get(), &zero, &c.cbytes, 1, &s, out.get(), &st);
        if (!window_result(c, kind == 0 ? "strided" : kind == 1 ? "grouped device" : "grouped host", rc, st, out.get(), first, count, step)) return false;
    }
    return true;
}

int main()
{
    // The emulated batch call has no sized form (a chunk's buffer is taken to reach as far as the lean launch's early read of
    // bstarts[j], as in an unsized engine call, whose chunks lie in 64-byte slots): with exact-size chunks the general kernel, whose
    // phase A holds the pattern fill, runs alone.  The window calls hand the sizes on.
    emu_set_lean(0);
    const int value_ts[] = {1, 2, 3, 4, 8, 12, 16, 255};
    std::vector<Chunk> chunks;
    for (int ts : value_ts) chunks.emplace_back(VALUE, ts, (2 * 4096 + 1000) / ts * ts, 4096);     // (4096 is no multiple of 3, 12, 255: every phase)
    chunks.emplace_back(VALUE, 4, (2 * 4098 + 1000) / 4 * 4, 4098);                                // a rotated 16-byte pattern
    chunks.emplace_back(VALUE, 16, 200 * 16, 1000);
    chunks.emplace_back(NAN_, 4, 9192, 4096);
    chunks.emplace_back(NAN_, 8, 9192, 4096);
    chunks.emplace_back(UNINIT, 4, 9192, 4096);
    chunks.emplace_back(ZERO, 2, 9192, 4096);
    chunks.emplace_back(VALUE, 4, 192 * 1024 * 2 + 40, 192 * 1024);                                // wide blocks (cimg_decode_wide's body)
    for (const Chunk& c : chunks) {
        for (int mis : {0, 1, 3, 7, 15, 16}) if (!batch(c, mis)) return 1;
        if (c.blocksize <= 64 * 1024 && !windows(c)) return 1;               // (a window over wide blocks is a batch decode and a copy)
    }
    printf("special asan ok %d\n", g_cases);
    return 0;
}
