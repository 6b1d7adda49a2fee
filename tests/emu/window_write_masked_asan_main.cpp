// tests/emu/window_write_masked_asan_main.cpp -- TEST INFRASTRUCTURE: masked and constant window writes (planner, the coverage and
// disjointness proofs, the host call's packing of rows and mask rows, and the body of cimg_update_patch_masked) once more under
// AddressSanitizer / UBSan, as a stand-alone program: linked with window_write_masked_emu.cpp, emu.cpp and wide_emu.cpp
// (tests/_window_writes_masked.py: build_emu(sanitize=True)).  Every buffer handed to a call is an allocation of its exact size, so a
// read or write one byte past a chunk, a source row, a mask row or a new chunk's capacity is reported; a call whose windows are all
// constant gets no source at all, one without masks no mask.  Chunks come from the emulated compress; the result is checked against
// a plain loop over the decoded pixels.
//   window_write_masked_asan [write order 0 | 1 | 2]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct CParams { int32_t typesize, clevel, blocksize, compcode, splitmode; uint8_t filters[6], filters_meta[6]; };
struct MaskedWindow {
    int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch;
    int64_t mask_off, mask_pitch; int32_t flags, pad_; uint8_t value[8];
};
enum { WM_CONST = 1, WM_MASK = 2 };

extern "C" {
int wemu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                        const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);
int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
int wwmemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                         const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const MaskedWindow* w,
                         const uint8_t* src, const uint8_t* mask, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes,
                         int32_t* status);
int wwmemu_update_host(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                       const int32_t* destsize, int nwindows, const MaskedWindow* w, const uint8_t* src, const uint8_t* mask,
                       void** new_chunks, int32_t* new_cbytes, int32_t* status);
void wwemu_free(void* m);
void emu_set_write_order(int o);
}

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// forms: 0 the four forms in turn, 1 every window constant and unmasked (no source, no mask), 2 every window a masked array
static int run(int ts, int compcode, int clevel, int blocksize, int forms)
{
    const int chunk_elems = 13000, elems = 2 * chunk_elems + 5001, nchunks = 3;
    std::vector<uint8_t> plane((size_t)elems * ts);
    for (size_t i = 0; i < plane.size(); i++) plane[i] = (uint8_t)((i / 7) % 251 ^ ((i % 97) ? 0 : rnd()));
    CParams p{};
    p.typesize = ts; p.clevel = clevel; p.blocksize = blocksize; p.compcode = compcode; p.splitmode = 3; p.filters[5] = 1;
    // each chunk an allocation of its exact size
    std::vector<std::vector<uint8_t>> chunks;
    std::vector<int32_t> nbytes, bsz, csz, dsz;
    for (int i = 0; i < nchunks; i++) {
        const int32_t nb = (i < 2 ? chunk_elems : elems - 2 * chunk_elems) * ts, ds = nb + 32;
        std::vector<uint8_t> c((size_t)ds);
        const int64_t zero = 0;
        int32_t cb = 0;
        CHECK(wemu_compress_batch(&p, 1, plane.data() + (size_t)i * chunk_elems * ts, &zero, &nb, c.data(), &zero, &ds, &cb) == 0 && cb > 0);
        c.resize((size_t)cb);
        int32_t hb;
        memcpy(&hb, c.data() + 8, 4);
        chunks.push_back(std::vector<uint8_t>(c.begin(), c.end()));
        nbytes.push_back(nb); bsz.push_back(hb); csz.push_back(cb); dsz.push_back(ds);
    }
    // windows: dense rectangles from odd origins, strided ones, far-apart samples, whole blocks, rows over the chunk boundary,
    // interleaved columns, alternating rows, the last element
    std::vector<MaskedWindow> w;
    auto add = [&](int64_t origin, int width, int height, int64_t rp, int64_t cp) {
        MaskedWindow s{};
        s.chunk_first = 0; s.chunk_count = nchunks; s.origin = origin; s.row_pitch = rp; s.col_pitch = cp; s.width = width; s.height = height;
        w.push_back(s);
    };
    add(181, 25, 7, 180, 3); add(180 * 20 + 3, 41, 12, 180, 1); add(180 * 22 + 7, 12, 8, 180, 2); add(3, (elems - 4) / (8192 / ts + 5) + 1, 1, 1, 8192 / ts + 5);
    add(chunk_elems - 2 * 180 - 17, 29, 6, 180, 2); add(8000, 2600, 1, 1, 2); add(8001, 2600, 1, 1, 2); add(elems - 1, 1, 1, 1, 9);
    add(8192 / ts - 10, 2 * (8192 / ts) + 30, 1, 1, 1);                                     // two whole blocks and more
    add(180 * 60 + 1, 177, 10, 360, 1); add(180 * 61 + 1, 177, 10, 360, 1);                 // alternating rows
    add(chunk_elems + 180 * 3 + 2, 63, 9, 180, 1); add(chunk_elems + 180 * 14 + 3, 62, 9, 180, 1);
    // forms, sources and masks: every row an exact piece of an exact buffer (out_pitch = width * ts, mask_pitch = width)
    int64_t at = 0, mat = 0;
    for (size_t k = 0; k < w.size(); k++) {
        MaskedWindow& s = w[k];
        s.flags = forms == 1 ? WM_CONST : forms == 2 ? WM_MASK : (int)(k % 4);
        if (s.flags & WM_CONST) for (int i = 0; i < ts && i < 8; i++) s.value[i] = (uint8_t)rnd();
        else { s.out_off = at; s.out_pitch = (int64_t)s.width * ts; at += s.out_pitch * s.height; }
        if (s.flags & WM_MASK) { s.mask_off = mat; s.mask_pitch = s.width; mat += (int64_t)s.width * s.height; }
    }
    std::vector<uint8_t> src((size_t)at), mask((size_t)mat);
    for (uint8_t& b : src) b = (uint8_t)rnd();
    for (size_t i = 0; i < mask.size(); i++) { const uint32_t r = rnd(); mask[i] = (i / 50) % 3 == 0 ? 1 : (r & 1) ? (uint8_t)(r >> 8 | 1) : 0; }
    const uint8_t* srcp = src.empty() ? nullptr : src.data();
    const uint8_t* maskp = mask.empty() ? nullptr : mask.data();
    // the expectation: a plain loop
    std::vector<uint8_t> want = plane;
    for (const MaskedWindow& s : w)
        for (int r = 0; r < s.height; r++)
            for (int c = 0; c < s.width; c++) {
                if ((s.flags & WM_MASK) && mask[(size_t)(s.mask_off + r * s.mask_pitch + c)] == 0) continue;
                uint8_t* d = want.data() + (size_t)(s.origin + r * (s.height > 1 ? s.row_pitch : 0) + c * (s.width > 1 ? s.col_pitch : 0)) * ts;
                if (s.flags & WM_CONST) memcpy(d, s.value, (size_t)ts);
                else memcpy(d, src.data() + s.out_off + r * s.out_pitch + (int64_t)c * ts, (size_t)ts);
            }
    for (int host = 0; host < 2; host++) {
        std::vector<int32_t> ncb((size_t)nchunks, 0), st((size_t)nchunks, 0);
        std::vector<std::vector<uint8_t>> out((size_t)nchunks);
        std::vector<uint8_t> all;
        std::vector<int64_t> off, noff;
        int64_t nt = 0;
        for (int i = 0; i < nchunks; i++) { off.push_back((int64_t)all.size()); all.insert(all.end(), chunks[(size_t)i].begin(), chunks[(size_t)i].end()); noff.push_back(nt); nt += dsz[(size_t)i]; }
        const std::vector<uint8_t> exact(all.begin(), all.end());
        if (host) {
            std::vector<void*> ptrs((size_t)nchunks, nullptr);
            CHECK(wwmemu_update_host(&p, nchunks, exact.data(), off.data(), csz.data(), dsz.data(), (int)w.size(), w.data(), srcp, maskp, ptrs.data(),
                                     ncb.data(), st.data()) == 0);
            for (int i = 0; i < nchunks; i++) { CHECK(ptrs[(size_t)i]); out[(size_t)i].assign((uint8_t*)ptrs[(size_t)i], (uint8_t*)ptrs[(size_t)i] + ncb[(size_t)i]); wwemu_free(ptrs[(size_t)i]); }
        } else {
            std::vector<uint8_t> nbuf((size_t)nt);
            CHECK(wwmemu_update_device(&p, nchunks, exact.data(), off.data(), csz.data(), nbytes.data(), bsz.data(), dsz.data(), (int)w.size(), w.data(),
                                       srcp, maskp, nbuf.data(), noff.data(), ncb.data(), st.data()) == 0);
            for (int i = 0; i < nchunks; i++) out[(size_t)i].assign(nbuf.begin() + noff[(size_t)i], nbuf.begin() + noff[(size_t)i] + ncb[(size_t)i]);
        }
        for (int i = 0; i < nchunks; i++) {
            CHECK(st[(size_t)i] == 0 && ncb[(size_t)i] > 0);
            std::vector<uint8_t> raw((size_t)nbytes[(size_t)i]);
            const int64_t zero = 0;
            int32_t s1 = 0;
            CHECK(wemu_decompress_batch(1, out[(size_t)i].data(), &zero, &ncb[(size_t)i], &nbytes[(size_t)i], &bsz[(size_t)i], raw.data(), &zero, &s1) == 0 && s1 == 0);
            CHECK(memcmp(raw.data(), want.data() + (size_t)i * chunk_elems * ts, raw.size()) == 0);
        }
    }
    return 0;
}

int main(int argc, char** argv)
{
    const int order = argc > 1 ? argv[1][0] - '0' : 0;
    // splice route: lz4 shuffle ts 1 / 2 / 3 / 4 / 8, blosclz; whole route: zstd, memcpyed; then all-constant and all-masked calls
    const int cases[][5] = {{1, 1, 5, 8192, 0}, {2, 1, 5, 8192, 0}, {3, 1, 5, 8192, 0}, {4, 1, 5, 8192, 0}, {8, 1, 5, 8192, 0}, {2, 0, 5, 8192, 0},
                            {4, 5, 3, 8192, 0}, {4, 1, 0, 8192, 0}, {1, 1, 5, 8192, 1}, {4, 1, 5, 8192, 1}, {1, 1, 5, 8192, 2}, {2, 1, 5, 8192, 2}};
    emu_set_write_order(order);
    for (const auto& c : cases) {
        if (run(c[0], c[1], c[2], c[3], c[4])) { printf("case ts %d codec %d clevel %d forms %d failed\n", c[0], c[1], c[2], c[4]); return 1; }
    }
    printf("ok\n");
    return 0;
}
