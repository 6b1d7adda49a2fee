// tests/emu/zstd_frames_asan_main.cpp -- TEST INFRASTRUCTURE: zstd frames through emu_zstd_decode (emu.cpp: csrc/zstd_decode.h in place,
// through a stage, all copies serial, and walked + replayed) under AddressSanitizer / UBSan (host code only;
// tests/test_emu_zstd_streams.py builds it with emu.cpp and runs it once per write order).  The file named on the command line holds a count, then
// per frame: its size, the size of its output, the frame, the output.  Frame and destination are heap allocations of exactly their
// size, so one byte read or written outside them is reported.  Every frame is decoded at capacity n and n + 8 and must be refused
// at n - 1.  Prints "ok <frames>".
// A second file, if named, holds chunks (a count, then per chunk: its size, nbytes, blocksize, 1 if it must be refused, the chunk, its
// pixels): they go through emu_decompress_batch in one batch -- the kernels of the zstd read path with LDS modelled at its exact size
// (EMU_LDS_SLACK=0) -- in the five forms of the read path, into an output buffer of exactly the pixels' size.  Prints "ok <chunks>".
// A third argument, a digit, is the emulator's write order (0 ascending, 1 descending, 2 shuffled; wave.h R2) for everything above.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int emu_zstd_decode(const uint8_t* src, int csize, uint8_t* dst, int cap);
extern "C" int emu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* nbytes, const int32_t* blocksize,
                                    uint8_t* raw, const int64_t* raw_off, int32_t* status);
extern "C" void emu_set_zstd_plan(int cap);
extern "C" void emu_set_zstd_lanes(int n);
extern "C" void emu_set_write_order(int o);

static uint32_t rd32(FILE* f)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { printf("short file\n"); exit(1); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static int run_chunks(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    std::vector<int64_t> comp_off(count), raw_off(count);
    std::vector<int32_t> nbytes(count), blocksize(count), refused(count), csize(count);
    std::vector<std::vector<uint8_t>> chunks(count), pixels(count);
    int64_t at = 0, rat = 0;
    for (uint32_t k = 0; k < count; k++) {
        csize[k] = (int32_t)rd32(f); nbytes[k] = (int32_t)rd32(f); blocksize[k] = (int32_t)rd32(f); refused[k] = (int32_t)rd32(f);
        chunks[k].resize((size_t)csize[k]); pixels[k].resize((size_t)nbytes[k]);
        if (fread(chunks[k].data(), 1, chunks[k].size(), f) != chunks[k].size() || fread(pixels[k].data(), 1, pixels[k].size(), f) != pixels[k].size()) return 1;
        comp_off[k] = at; at += (csize[k] + 15) / 16 * 16 + 16;      // (the layout of tests/_emu.py: decompress_batch)
        raw_off[k] = rat; rat += nbytes[k];
    }
    fclose(f);
    uint8_t* comp = (uint8_t*)calloc((size_t)at + 64, 1);
    for (uint32_t k = 0; k < count; k++) memcpy(comp + comp_off[k], chunks[k].data(), chunks[k].size());
    static const int forms[5][2] = {{-1, 8}, {-1, 3}, {-1, 0}, {0, 8}, {256, 8}};
    for (const auto& form : forms) {
        emu_set_zstd_plan(form[0]); emu_set_zstd_lanes(form[1]);
        uint8_t* raw = (uint8_t*)malloc((size_t)rat ? (size_t)rat : 1);
        memset(raw, 0x77, (size_t)rat);
        std::vector<int32_t> st(count, 0);
        const int rc = emu_decompress_batch((int)count, comp, comp_off.data(), nbytes.data(), blocksize.data(), raw, raw_off.data(), st.data());
        if (rc) { printf("batch %d\n", rc); return 1; }
        for (uint32_t k = 0; k < count; k++) {
            if (refused[k] ? st[k] >= 0 : (st[k] != 0 || memcmp(raw + raw_off[k], pixels[k].data(), pixels[k].size()))) {
                printf("chunk %u form %d/%d: status %d\n", k, form[0], form[1], st[k]); return 1;
            }
        }
        free(raw);
    }
    free(comp);
    printf("ok %u\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    emu_set_write_order(argc > 3 ? argv[3][0] - '0' : 0);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t csize = rd32(f), n = rd32(f);
        uint8_t* frame = (uint8_t*)malloc(csize ? csize : 1);
        uint8_t* want = (uint8_t*)malloc(n ? n : 1);
        if (fread(frame, 1, csize, f) != csize || fread(want, 1, n, f) != n) { printf("short file\n"); return 1; }
        for (int extra : {0, 8}) {
            const size_t cap = (size_t)n + (size_t)extra;
            uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
            const int r = emu_zstd_decode(frame, (int)csize, out, (int)cap);
            if (r != (int)n || (n && memcmp(out, want, n))) { printf("frame %u at capacity %zu: %d\n", k, cap, r); return 1; }
            free(out);
        }
        if (n) {
            uint8_t* out = (uint8_t*)malloc(n);
            const int r = emu_zstd_decode(frame, (int)csize, out, (int)n - 1);
            if (r >= 0) { printf("frame %u fits %u bytes?\n", k, n - 1); return 1; }
            free(out);
        }
        free(frame);
        free(want);
    }
    fclose(f);
    printf("ok %u\n", count);
    return argc > 2 ? run_chunks(argv[2]) : 0;
}
