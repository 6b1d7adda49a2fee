// tests/emu/window_write_typed_asan_main.cpp -- TEST INFRASTRUCTURE: typed window writes (the typed checks, the planner, both
// schedules and the body of cimg_update_patch_typed) once more under AddressSanitizer / UBSan, as a stand-alone program: linked with
// window_write_typed_emu.cpp, emu.cpp and wide_emu.cpp (tests/_window_writes_typed.py: build_emu(sanitize=True)).  Every buffer
// handed to a call is an allocation of its exact size -- the source ends with the last byte of its last element, whatever the
// elem_pitch --, so a load or store one byte too wide or too far is reported.  Chunks come from the emulated compress; the result is
// checked against a plain loop over the decoded pixels with the conversion written out in C (this file is built with
// -ffp-contract=off too).
//   window_write_typed_asan [write order 0 | 1 | 2]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct CParams { int32_t typesize, clevel, blocksize, compcode, splitmode; uint8_t filters[6], filters_meta[6]; };
struct TypedWindow {
    int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch;
    int64_t elem_pitch; int32_t src_type, out_type; float scale, offset;
};
static_assert(sizeof(TypedWindow) == 80, "cimg_window_typed");
enum { U8 = 0, I8 = 1, U16 = 2, I16 = 3, U32 = 4, I32 = 5, F16 = 6, F32 = 7 };

extern "C" {
int wemu_compress_batch(const void* p, int nchunks, const uint8_t* raw, const int64_t* raw_off, const int32_t* nbytes, uint8_t* comp,
                        const int64_t* comp_off, const int32_t* destsize, int32_t* cbytes);
int wemu_decompress_batch(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                          const int32_t* blocksize, uint8_t* raw, const int64_t* raw_off, int32_t* status);
int wwtemu_update_device(const void* p, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                         const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize, int nwindows, const TypedWindow* w,
                         const uint8_t* src, uint8_t* newbuf, const int64_t* new_off, int32_t* new_cbytes, int32_t* status);
void emu_set_write_order(int o);
}

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int tsize(int t) { return t < U16 ? 1 : t < U32 || t == F16 ? 2 : 4; }

// float16 -> float32, exact (normals, subnormals, inf / NaN)
static float half_value(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 0x3FF;
    float v = e == 31 ? (m ? NAN : INFINITY) : e ? std::ldexp((float)(m | 0x400), e - 25) : std::ldexp((float)m, -24);
    return (h & 0x8000) ? -v : v;
}

// the conversion of include/cimg_hip.h for an integer or float32 plane, written out
static void convert(float y, int stored, float scale, float offset, uint8_t* out)
{
    const float d = y - offset;
    const float t = d / scale;
    if (stored == F32) { memcpy(out, &t, 4); return; }
    double r = std::isnan(t) ? 0.0 : std::nearbyint((double)t);
    const double lo = stored == U8 || stored == U16 || stored == U32 ? 0.0 : stored == I8 ? -128.0 : stored == I16 ? -32768.0 : -2147483648.0;
    const double hi = stored == U8 ? 255.0 : stored == I8 ? 127.0 : stored == U16 ? 65535.0 : stored == I16 ? 32767.0 : stored == U32 ? 4294967295.0 : 2147483647.0;
    r = r < lo ? lo : r > hi ? hi : r;
    const int64_t v = (int64_t)r;
    memcpy(out, &v, (size_t)tsize(stored));                        // (little endian: the low bytes)
}

static int run(int stored, int mem, int compcode, int clevel, int blocksize)
{
    const int ts = tsize(stored), msz = tsize(mem);
    const int chunk_elems = 13000, elems = 2 * chunk_elems + 5001, nchunks = 3;
    std::vector<uint8_t> plane((size_t)elems * ts);
    for (size_t i = 0; i < plane.size(); i++) plane[i] = (uint8_t)((i / 7) % 251 ^ ((i % 97) ? 0 : rnd()));
    if (stored == F32) for (int i = 0; i < elems; i++) { const float f = (float)(i % 977) * 0.25f; memcpy(plane.data() + (size_t)i * 4, &f, 4); }
    CParams p{};
    p.typesize = ts; p.clevel = clevel; p.blocksize = blocksize; p.compcode = compcode; p.splitmode = 3; p.filters[5] = 1;
    std::vector<std::vector<uint8_t>> chunks;
    std::vector<int32_t> nbytes, bsz, csz, dsz;
    for (int i = 0; i < nchunks; i++) {
        const int32_t nb = (i < 2 ? chunk_elems : elems - 2 * chunk_elems) * ts, ds = nb + 32;
        std::vector<uint8_t> c((size_t)ds);
        const int64_t zero = 0;
        int32_t cb = 0;
        CHECK(wemu_compress_batch(&p, 1, plane.data() + (size_t)i * chunk_elems * ts, &zero, &nb, c.data(), &zero, &ds, &cb) == 0 && cb > 0);
        int32_t hb;
        memcpy(&hb, c.data() + 8, 4);
        chunks.push_back(std::vector<uint8_t>(c.begin(), c.begin() + cb));
        nbytes.push_back(nb); bsz.push_back(hb); csz.push_back(cb); dsz.push_back(ds);
    }
    // windows: strided rectangles, a dense one, overlapping ones, far-apart samples, 300 pixels of one block and 20 duplicates,
    // interleaved rows, an identity window, the last element; elem_pitch of 1, 3 and 4 memory sizes
    std::vector<TypedWindow> w;
    const float pairs[4][2] = {{1.0f / 255, 0.0f}, {1.0f / 255, -0.4851f}, {-0.5f, 3.0f}, {1.0f, 0.0f}};
    auto add = [&](int64_t origin, int width, int height, int64_t rp, int64_t cp) {
        const size_t k = w.size();
        const int mult = (int)(k % 3 == 0 ? 1 : k % 3 == 1 ? 3 : 4);
        w.push_back(TypedWindow{0, nchunks, origin, rp, cp, width, height, 0, 0, (int64_t)mult * msz, stored, mem, pairs[k % 4][0], pairs[k % 4][1]});
    };
    add(181, 25, 7, 180, 3); add(180 * 20 + 3, 40, 12, 180, 1); add(180 * 22 + 7, 12, 8, 180, 2); add(3, (elems - 4) / (8192 / ts + 5) + 1, 1, 1, 8192 / ts + 5);
    add(chunk_elems - 2 * 180 - 17, 29, 6, 180, 2); add(8000, 2600, 1, 1, 2); add(8001, 2600, 1, 1, 2); add(elems - 1, 1, 1, 1, 9);
    add(0, 8192 / ts, 1, 1, 1);                                                        // covers block 0 of chunk 0: not staged
    const int epb = 8192 / ts;
    std::vector<int> px;
    for (int k = 0; k < 300; k++) px.push_back(epb + 3 + (int)((k * 7919u) % (unsigned)(epb - 10)));
    for (int k = 0; k < 20; k++) px.push_back(px[(size_t)(k * 13)]);
    for (const int a : px) add(a, 1, 1, 1, 1 + a % 3);
    for (int k = 0; k < 4; k++) add(2 * epb + 10 + 220 * k, 70, 1, 1, 3);              // a disjoint unit of strided rows
    w.push_back(TypedWindow{0, nchunks, 180 * 30 + 5, 180, 2, 30, 5, 0, 0, ts, stored, stored, 1.0f, 0.0f});      // identity, dense source
    w.push_back(TypedWindow{0, nchunks, 180 * 40 + 5, 180, 1, 30, 5, 0, 0, 3 * ts, stored, stored, 1.0f, 0.0f});  // identity, spaced source
    // the source: each window's rows in one allocation that ends with the last element's last byte
    int64_t at = 0;
    for (TypedWindow& s : w) {
        const int sz = s.out_type == stored && s.scale == 1.0f && s.offset == 0.0f ? ts : msz;
        at = (at + 7) / 8 * 8;
        s.out_off = at; s.out_pitch = ((int64_t)(s.width - 1) * s.elem_pitch + sz + 7) / 8 * 8;
        at += s.out_pitch * (s.height - 1) + (int64_t)(s.width - 1) * s.elem_pitch + sz;
    }
    std::vector<uint8_t> src((size_t)at);
    for (uint8_t& b : src) b = (uint8_t)rnd();
    const float special[12] = {NAN, INFINITY, -INFINITY, -0.0f, 0.5f / 255, 1.5f / 255, 2.5f / 255, 300.0f, -300.0f, 1e-40f, 70000.0f, 4.3e9f};
    std::vector<uint8_t> want = plane;
    for (const TypedWindow& s : w) {
        const bool identity = s.out_type == stored && s.scale == 1.0f && s.offset == 0.0f;
        for (int r = 0; r < s.height; r++)
            for (int c = 0; c < s.width; c++) {
                uint8_t* m = src.data() + s.out_off + r * s.out_pitch + c * s.elem_pitch;
                uint8_t* d = want.data() + (size_t)(s.origin + r * (s.height > 1 ? s.row_pitch : 0) + c * (s.width > 1 ? s.col_pitch : 0)) * ts;
                if (identity) { memcpy(d, m, (size_t)ts); continue; }
                float y;
                if (mem == F32) {
                    y = rnd() % 5 == 0 ? special[rnd() % 12] : ((float)(rnd() % 70000) - 2000.0f) * 0.25f * s.scale + s.offset;
                    memcpy(m, &y, 4);
                } else {
                    uint16_t h = (uint16_t)rnd();
                    memcpy(m, &h, 2);
                    y = half_value(h);
                }
                convert(y, stored, s.scale, s.offset, d);
            }
    }
    std::vector<uint8_t> all;
    std::vector<int64_t> off, noff;
    int64_t nt = 0;
    for (int i = 0; i < nchunks; i++) { off.push_back((int64_t)all.size()); all.insert(all.end(), chunks[(size_t)i].begin(), chunks[(size_t)i].end()); noff.push_back(nt); nt += dsz[(size_t)i]; }
    all.shrink_to_fit();
    std::vector<uint8_t> nbuf((size_t)nt);
    std::vector<int32_t> ncb((size_t)nchunks, 0), st((size_t)nchunks, 0);
    CHECK(wwtemu_update_device(&p, nchunks, all.data(), off.data(), csz.data(), nbytes.data(), bsz.data(), dsz.data(), (int)w.size(), w.data(),
                               src.data(), nbuf.data(), noff.data(), ncb.data(), st.data()) == 0);
    for (int i = 0; i < nchunks; i++) {
        CHECK(st[(size_t)i] == 0 && ncb[(size_t)i] > 0);
        std::vector<uint8_t> out(nbuf.begin() + noff[(size_t)i], nbuf.begin() + noff[(size_t)i] + ncb[(size_t)i]);
        std::vector<uint8_t> raw((size_t)nbytes[(size_t)i]);
        const int64_t zero = 0;
        int32_t s1 = 0;
        CHECK(wemu_decompress_batch(1, out.data(), &zero, &ncb[(size_t)i], &nbytes[(size_t)i], &bsz[(size_t)i], raw.data(), &zero, &s1) == 0 && s1 == 0);
        const uint8_t* e = want.data() + (size_t)i * chunk_elems * ts;
        for (size_t k = 0; k < raw.size(); k += (size_t)ts) {
            if (memcmp(raw.data() + k, e + k, (size_t)ts) == 0) continue;
            float a, b;
            if (stored == F32) { memcpy(&a, raw.data() + k, 4); memcpy(&b, e + k, 4); if (std::isnan(a) && std::isnan(b)) continue; }
            printf("chunk %d element %zu differs\n", i, k / (size_t)ts);
            return 1;
        }
    }
    // a refusal touches nothing
    TypedWindow bad = w[0];
    bad.scale = 0.0f;
    std::vector<int32_t> ncb2((size_t)nchunks, 77), st2((size_t)nchunks, 77);
    CHECK(wwtemu_update_device(&p, nchunks, all.data(), off.data(), csz.data(), nbytes.data(), bsz.data(), dsz.data(), 1, &bad, src.data(), nbuf.data(),
                               noff.data(), ncb2.data(), st2.data()) == -12);
    for (int i = 0; i < nchunks; i++) CHECK(ncb2[(size_t)i] == 77 && st2[(size_t)i] == 77);
    return 0;
}

int main(int argc, char** argv)
{
    const int order = argc > 1 ? argv[1][0] - '0' : 0;
    // (stored, memory, codec, clevel, blocksize) -- splice route: lz4 and blosclz; whole route: zstd, memcpyed
    const int cases[][5] = {{U8, F32, 1, 5, 8192}, {U8, F16, 1, 5, 8192}, {U16, F32, 1, 5, 8192}, {I16, F16, 0, 5, 8192}, {I32, F32, 1, 5, 8192},
                            {F32, F32, 1, 5, 8192}, {U16, F32, 5, 3, 8192}, {U8, F32, 1, 0, 8192}};
    emu_set_write_order(order);
    for (const auto& c : cases) {
        if (run(c[0], c[1], c[2], c[3], c[4])) { printf("case stored %d mem %d codec %d clevel %d failed\n", c[0], c[1], c[2], c[3]); return 1; }
    }
    printf("ok\n");
    return 0;
}
