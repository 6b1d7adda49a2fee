// tests/emu/blosclz_wide_asan_main.cpp -- TEST INFRASTRUCTURE: blosclz_wide_encode (csrc/wide_kernel.h) under AddressSanitizer / UBSan
// (host code only; tests/test_emu_blosclz_wide.py builds this one file and runs it once).  The check for the encoder's rule that no
// load touches a byte outside [in, in + n): input, table and output are heap allocations of exactly n, 16 384 and cap bytes, and
// every stream is presented twice -- staged at the start of its allocation, and "in place" at the END of a larger one, as a
// slice of the caller's pixels that ends with them.  Both presentations must give the same bytes, under each lane order of the
// emulator, at clevels 1 / 5 / 9, and again with cap = need (same bytes) and cap = need - 1 (0).  Prints "ok <calls>".
#define CIMG_EMULATE 1
#include "wide_kernel.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace cimg { int g_emu_write_order = 0; }
using namespace cimg;

static uint64_t mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static std::vector<uint8_t> far_stream(int n, int d)
{
    std::vector<uint8_t> a((size_t)n, 0);
    for (int i = 0; i < 200; i++) a[100 + i] = a[100 + d + i] = (uint8_t)(1 + mix(700 + i) % 255);
    for (int i = 0; i < 5000; i++) a[n - 5000 + i] = (uint8_t)mix(9000 + i);
    return a;
}
static std::vector<uint8_t> steps(int n, int rep)
{
    std::vector<uint8_t> a((size_t)n);
    for (int i = 0; i < n; i++) a[i] = (uint8_t)mix(40 + i / rep);
    return a;
}
static std::vector<uint8_t> period(int n, int p)
{
    std::vector<uint8_t> a((size_t)n);
    for (int i = 0; i < n; i++) a[i] = (uint8_t)mix(77 + i % p);
    return a;
}
static std::vector<uint8_t> noise(int n, int mod)
{
    std::vector<uint8_t> a((size_t)n);
    for (int i = 0; i < n; i++) a[i] = (uint8_t)(mix(123 + i) % (uint64_t)mod);
    return a;
}

static int encode(const std::vector<uint8_t>& s, int cap, int clevel, bool in_place, std::vector<uint8_t>& got, int& need)
{
    const int n = (int)s.size();
    const size_t lead = in_place ? 4099 : 0;
    uint8_t* in = (uint8_t*)malloc(lead + (size_t)n + (n == 0));
    uint32_t* tab = (uint32_t*)malloc(LZ4_HASH_BYTES);
    uint8_t* out = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1));
    if (n) memcpy(in + lead, s.data(), (size_t)n);
    memset(tab, 0xCD, LZ4_HASH_BYTES);
    need = 0;
    const int r = blosclz_wide_encode(in + lead, tab, n, out, cap, clevel, need);
    got.assign(out, out + (r > 0 ? r : 0));
    free(in); free(tab); free(out);
    return r;
}

int main()
{
    std::vector<std::vector<uint8_t>> streams;
    for (int n : {0, 15, 16, 17, 100, 1000}) streams.push_back(steps(n, 5));     // short leftover blocks go through the wide kernel too
    for (int n : {65535, 65536, 65537}) streams.push_back(steps(n, 7));
    streams.push_back(period(98304, 211));                                        // one match that runs to the stream's end
    streams.push_back(period(200001, 3));
    streams.push_back(noise(131072, 4));
    streams.push_back(noise(70001, 256));                                         // the probe gives up
    for (int d : {8191, 8192, 73724, 73725}) streams.push_back(far_stream(100000, d));
    streams.push_back(far_stream(262144, 73724));
    long calls = 0;
    for (const auto& s : streams) {
        const int n = (int)s.size();
        for (int clevel : {1, 5, 9}) {
            std::vector<uint8_t> ref, got;
            int need0 = 0, need = 0;
            g_emu_write_order = 0;
            const int r0 = encode(s, n, clevel, false, ref, need0);
            if (r0 < 0) { printf("loop guard tripped: n %d clevel %d\n", n, clevel); return 1; }
            calls++;
            for (int order = 0; order < 3; order++) {
                g_emu_write_order = order;
                for (int place = 0; place < 2; place++) {
                    if (order == 0 && place == 0) continue;
                    const int r = encode(s, n, clevel, place != 0, got, need);
                    if (r != r0 || need != need0 || got != ref) { printf("presentations differ: n %d clevel %d order %d place %d\n", n, clevel, order, place); return 1; }
                    calls++;
                }
            }
            g_emu_write_order = 0;
            if (r0 > 0) {
                if (need0 != (r0 + 1 > 66 ? r0 + 1 : 66)) { printf("need: n %d clevel %d\n", n, clevel); return 1; }
                if (encode(s, need0, clevel, true, got, need) != r0 || got != ref) { printf("cap = need: n %d clevel %d\n", n, clevel); return 1; }
                if (encode(s, need0 - 1, clevel, true, got, need) != 0) { printf("cap = need - 1: n %d clevel %d\n", n, clevel); return 1; }
                calls += 2;
            }
        }
    }
    printf("ok %ld\n", calls);
    return 0;
}
