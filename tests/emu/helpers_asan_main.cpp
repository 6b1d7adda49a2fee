// tests/emu/helpers_asan_main.cpp -- TEST INFRASTRUCTURE: the helper schedules of helpers_emu.cpp for the AddressSanitizer / UBSan
// build (tests/test_emu_helpers_place.py).  Every chunk destination is a heap allocation of exactly destsize, the pixels one of
// exactly their size: a plane placed past its chunk's capacity, by its owner or by a helper, is a report.  No oracle here: every
// schedule, item form and the switched-off form must give the same chunks, and the chunks must decode to the pixels.  Prints
// "helpers asan ok <runs>" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

struct EmuCParams {
    int32_t typesize, clevel, blocksize, compcode, splitmode;
    uint8_t filters[6], filters_meta[6];
};

extern "C" {
int emu_helpers_compress_batch(const EmuCParams* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes,
                               uint8_t* comp, const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes,
                               int schedule, int block_items_mode, int helpers, long* stats);
int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes,
                         const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
}

enum { BLOCK = 32768, NCHUNKS = 3, NBLOCKS = 2 };

static uint32_t g_rng = 12345;
static uint8_t noise() { g_rng = g_rng * 1664525u + 1013904223u; return (uint8_t)(g_rng >> 24); }

// the most significant byte of every element repeats a short pattern (a coded plane), the others are noise (stored planes)
static void fill(uint8_t* raw, size_t n, int ts)
{
    for (size_t i = 0; i < n; i++) raw[i] = (i % ts == (size_t)ts - 1) ? (uint8_t)(((i / ts) % 37) * 3) : noise();
}

static int g_runs = 0;

static bool one(int ts, bool odd_second)
{
    const int32_t chunk = NBLOCKS * BLOCK;
    const size_t n = (size_t)NCHUNKS * chunk;
    std::unique_ptr<uint8_t[]> raw(new uint8_t[n]);
    fill(raw.get(), n, ts);
    EmuCParams p{ts, 9, BLOCK, 1, 3, {0, 0, 0, 0, 0, 1}, {0, 0, 0, 0, 0, 0}};
    int64_t raw_off[NCHUNKS];
    int32_t nbytes[NCHUNKS], destsize[NCHUNKS], blocksize[NCHUNKS];
    for (int c = 0; c < NCHUNKS; c++) { raw_off[c] = (int64_t)c * chunk; nbytes[c] = chunk; destsize[c] = chunk + 32; blocksize[c] = BLOCK; }
    std::vector<std::vector<uint8_t>> first;
    for (int helpers = 1; helpers >= 0; helpers--)
        for (int schedule = 0; schedule < 4; schedule++)
            for (int items = 0; items < 3; items++) {
                // exact-size destinations; the second one byte into its allocation when the chunk is to start off a 4-byte boundary
                std::unique_ptr<uint8_t[]> dst[NCHUNKS];
                uint8_t* at[NCHUNKS];
                for (int c = 0; c < NCHUNKS; c++) {
                    const int lead = (odd_second && c == 1) ? 1 : 0;
                    dst[c].reset(new uint8_t[(size_t)destsize[c] + lead]);
                    memset(dst[c].get(), 0x5A, (size_t)destsize[c] + lead);
                    at[c] = dst[c].get() + lead;
                }
                const uint8_t* base = at[0];
                for (int c = 1; c < NCHUNKS; c++) if (at[c] < base) base = at[c];
                int64_t comp_off[NCHUNKS];
                for (int c = 0; c < NCHUNKS; c++) comp_off[c] = (int64_t)((uintptr_t)at[c] - (uintptr_t)base);
                int32_t cbytes[NCHUNKS] = {0, 0, 0};
                long stats[5];
                const int rc = emu_helpers_compress_batch(&p, NCHUNKS, raw.get(), raw_off, nbytes, (uint8_t*)(uintptr_t)base, comp_off, destsize, cbytes,
                                                          schedule, items, helpers, stats);
                if (rc != 0) { printf("ts %d odd %d schedule %d items %d helpers %d: rc %d\n", ts, (int)odd_second, schedule, items, helpers, rc); return false; }
                if (helpers && schedule == 1 && stats[3] == 0) { printf("ts %d schedule 1 items %d: no plane placed by a helper\n", ts, items); return false; }
                if (!helpers && (stats[3] || stats[4])) { printf("ts %d schedule %d items %d: helpers at work with the switch off\n", ts, schedule, items); return false; }
                for (int c = 0; c < NCHUNKS; c++) {
                    if (cbytes[c] <= 0 || cbytes[c] > destsize[c]) { printf("ts %d chunk %d: cbytes %d\n", ts, c, cbytes[c]); return false; }
                    std::vector<uint8_t> got(at[c], at[c] + cbytes[c]);
                    if (first.size() <= (size_t)c) first.push_back(got);
                    else if (first[(size_t)c] != got) { printf("ts %d odd %d schedule %d items %d helpers %d: chunk %d differs\n", ts, (int)odd_second, schedule, items, helpers, c); return false; }
                }
                g_runs++;
            }
    // the chunks decode to the pixels (each from an allocation of exactly its size)
    for (int c = 0; c < NCHUNKS; c++) {
        std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)chunk]);
        // (the emulated batch decode reads a chunk as an unsized engine call does: up to 64 bytes past bstarts[] -- give it the slot)
        std::vector<uint8_t> slot(first[(size_t)c]);
        slot.resize(slot.size() + 64, 0);
        const int64_t zero = 0;
        int32_t st = 0;
        const int rc = emu_decompress_batch(1, slot.data(), &zero, &nbytes[c], &blocksize[c], out.get(), &zero, &st);
        if (rc != 0 || st != 0 || memcmp(out.get(), raw.get() + raw_off[c], (size_t)chunk)) { printf("ts %d chunk %d: decode rc %d status %d or pixels differ\n", ts, c, rc, st); return false; }
    }
    return true;
}

int main()
{
    if (!one(2, false) || !one(4, false) || !one(2, true)) return 1;
    printf("helpers asan ok %d\n", g_runs);
    return 0;
}
