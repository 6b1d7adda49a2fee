// tests/emu/pack_asan_main.cpp -- TEST INFRASTRUCTURE: the pack and interleave kernel bodies under AddressSanitizer / UBSan (host code
// only; tests/test_emu_pack.py builds it with pack_emu.cpp).  Every source and every destination piece is a heap allocation of exactly
// its size, so one byte read or written outside a piece is reported.  Sizes come from the command line; every pair of source and
// destination misalignment 0..15 is run for sizes up to 4095, four pairs for larger ones.  Prints "ok <pieces>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
int pkemu_pack(int n, const void* const* src, const int32_t* bytes, uint8_t* dst, const int64_t* dst_off);
int pkemu_interleave(const uint8_t* src, int64_t plane_stride, int nch, int ts, int64_t npixels, uint8_t* dst);
}

// an allocation that ends exactly where the piece ends, with the piece `mis` bytes past a 16-byte boundary: a byte read or written
// behind the piece is reported by the sanitizer; the `mis` bytes in front are a canary checked when the piece is dropped
struct Exact {
    uint8_t* raw = nullptr; uint8_t* p; int lead;
    Exact(size_t n, int mis) : lead(mis)
    {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n + (size_t)mis + (n + (size_t)mis == 0))) abort();
        raw = (uint8_t*)q; p = raw + mis;
        memset(raw, 0xA5, (size_t)mis);
    }
    ~Exact()
    {
        for (int i = 0; i < lead; i++) if (raw[i] != 0xA5) { printf("byte in front of a piece overwritten\n"); abort(); }
        free(raw);
    }
};

int main(int argc, char** argv)
{
    long pieces = 0;
    static const int few[4][2] = {{0, 0}, {0, 7}, {9, 0}, {5, 11}};
    for (int k = 1; k < argc; k++) {
        const int n = atoi(argv[k]);
        const int pairs = n <= 4095 ? 256 : 4;
        for (int q = 0; q < pairs; q++) {
            const int sm = pairs == 256 ? q >> 4 : few[q][0], dm = pairs == 256 ? q & 15 : few[q][1];
            Exact s((size_t)n, sm), d((size_t)n, dm);
            for (int i = 0; i < n; i++) s.p[i] = (uint8_t)(i * 131 + q);
            const void* srcs[1] = {s.p};
            const int32_t bytes[1] = {n};
            const int64_t off[1] = {0};
            if (pkemu_pack(1, srcs, bytes, d.p, off)) { printf("pack refused %d\n", n); return 1; }
            if (n && memcmp(s.p, d.p, (size_t)n)) { printf("pack differs %d %d %d\n", n, sm, dm); return 1; }
            pieces++;
        }
    }
    // interleave: planes and pixels of exactly their sizes (16-byte aligned, as the entry point demands)
    for (int nch : {1, 3, 4, 9}) for (int ts : {1, 2, 4, 8}) for (long npix : {1L, 17L, 1000L, 4099L}) {
        const int64_t stride = (npix * ts + 15) & ~15L;
        uint8_t* planes = (uint8_t*)aligned_alloc(16, (size_t)(stride * nch));
        const size_t ob = (size_t)(npix * nch * ts);
        uint8_t* out = (uint8_t*)aligned_alloc(16, (ob + 15) & ~(size_t)15);       // (aligned_alloc wants a multiple of 16)
        for (int64_t i = 0; i < stride * nch; i++) planes[i] = (uint8_t)(i * 7);
        if (pkemu_interleave(planes, stride, nch, ts, npix, out)) { printf("interleave refused\n"); return 1; }
        for (long p = 0; p < npix; p++) for (int c = 0; c < nch; c++)
            if (memcmp(out + ((size_t)p * nch + c) * ts, planes + c * stride + p * ts, (size_t)ts)) { printf("interleave differs\n"); return 1; }
        free(planes); free(out);
    }
    printf("ok %ld\n", pieces);
    return 0;
}
