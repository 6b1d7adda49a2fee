// tests/emu/trunc_asan_main.cpp -- TEST INFRASTRUCTURE: the trunc-prec kernel body and its piece planner under AddressSanitizer / UBSan
// (host code only; tests/test_emu_trunc_prec.py builds it with trunc_emu.cpp and runs it once).  Every source and every destination
// piece is a heap allocation of exactly its size, so one byte read or written outside a piece is reported.  Sizes come from the
// command line; every pair of source and destination misalignment 0..15 is run for sizes up to 4099, four pairs for larger ones, each
// for typesizes 2, 4 and 8, copied and in place.  Prints "ok <pieces>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

extern "C" int tremu_pass(int n, const void* const* src, void* const* dst, const int32_t* bytes, int typesize, int meta);

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

static uint8_t want(const uint8_t* s, int k, int n, int ts, int zeroed)
{
    if (k >= n - n % ts) return s[k];
    const int b = k % ts;                                   // byte b of a little-endian element keeps its bits from zeroed on
    const int lo = zeroed - 8 * b;
    const uint8_t m = lo <= 0 ? 0xFF : lo >= 8 ? 0 : (uint8_t)(0xFF << lo);
    return s[k] & m;
}

int main(int argc, char** argv)
{
    long pieces = 0;
    static const int few[4][2] = {{0, 0}, {0, 7}, {9, 0}, {5, 11}};
    static const int M[9] = {0, 0, 10, 0, 23, 0, 0, 0, 52};
    for (int k = 1; k < argc; k++) {
        const int n = atoi(argv[k]);
        const int pairs = n <= 4099 ? 256 : 4;
        for (int ts : {2, 4, 8}) for (int q = 0; q < pairs; q++) {
            const int sm = pairs == 256 ? q >> 4 : few[q][0], dm = pairs == 256 ? q & 15 : few[q][1];
            const int zeroed = (q & 1) ? M[ts] - 1 : 1;      // the largest and the smallest that zero something
            const int meta = (-zeroed) & 0xFF;
            Exact s((size_t)n, sm), d((size_t)n, dm);
            for (int i = 0; i < n; i++) s.p[i] = (uint8_t)(i * 131 + q) | 1;
            const void* srcs[1] = {s.p};
            void* dsts[1] = {d.p};
            const int32_t bytes[1] = {n};
            if (tremu_pass(1, srcs, dsts, bytes, ts, meta)) { printf("pass refused %d\n", n); return 1; }
            for (int i = 0; i < n; i++) if (d.p[i] != want(s.p, i, n, ts, zeroed)) { printf("copy differs %d %d %d %d at %d\n", n, ts, sm, dm, i); return 1; }
            // in place over the copy's source
            Exact t((size_t)n, sm);
            memcpy(t.p, s.p, (size_t)n);
            const void* src2[1] = {t.p};
            void* dst2[1] = {t.p};
            if (tremu_pass(1, src2, dst2, bytes, ts, meta)) { printf("pass refused %d\n", n); return 1; }
            if (n && memcmp(t.p, d.p, (size_t)n)) { printf("in place differs %d %d %d\n", n, ts, sm); return 1; }
            pieces += 2;
        }
    }
    printf("ok %ld\n", pieces);
    return 0;
}
