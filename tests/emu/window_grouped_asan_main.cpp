// tests/emu/window_grouped_asan_main.cpp -- TEST INFRASTRUCTURE: one grouped window call from a case file, for the AddressSanitizer /
// UBSan build of window_grouped_emu.cpp (tests/test_emu_windows_grouped.py): planner, grouping and kernel body on the host lane
// emulator (host code only).  The file holds: int64 nchunks, typesize, output size, nwindows; int64 comp_off[n]; int32 comp_size[n],
// nbytes[n], blocksize[n]; nwindows cimg_window_strided; int64 buffer size; the buffer.  Every buffer is a heap allocation of exactly
// its size (the emulator's own tables too: window_grouped_env.h).  The windows run through the device-style and the host-style
// grouped call and through the strided call; prints the two grouped return codes, the strided one, and 1 if the three outputs and
// the status words agree byte for byte.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int wnemu_windows_grouped_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_grouped_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                               const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_strided_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
void emu_set_write_order(int o);
}

struct Win { int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch; };
static_assert(sizeof(Win) == 56, "cimg_window_strided");

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[4];
    if (!rd(f, hdr, 4)) return 2;
    const int n = (int)hdr[0], ts = (int)hdr[1], nw = (int)hdr[3];
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> cs((size_t)n), nb((size_t)n), bs((size_t)n);
    std::vector<Win> w((size_t)nw);
    int64_t bytes = 0;
    if (!rd(f, off.data(), (size_t)n) || !rd(f, cs.data(), (size_t)n) || !rd(f, nb.data(), (size_t)n) || !rd(f, bs.data(), (size_t)n)) return 2;
    if (!rd(f, w.data(), (size_t)nw) || !rd(f, &bytes, 1)) return 2;
    std::vector<uint8_t> buf((size_t)bytes);
    if (!rd(f, buf.data(), (size_t)bytes)) return 2;
    fclose(f);
    emu_set_write_order(argc > 2 ? argv[2][0] - '0' : 0);
    std::vector<int32_t> st1((size_t)n), st2((size_t)n), st3((size_t)n);
    std::vector<uint8_t> out1((size_t)hdr[2], 0xA5), out2((size_t)hdr[2], 0xA5), out3((size_t)hdr[2], 0xA5);
    const int a = wnemu_windows_grouped_device(n, buf.data(), off.data(), cs.data(), nb.data(), bs.data(), ts, nw, w.data(), out1.data(), st1.data());
    const int b = wnemu_windows_grouped_host(n, buf.data(), off.data(), cs.data(), nw, w.data(), out2.data(), st2.data());
    const int c = wnemu_windows_strided_device(n, buf.data(), off.data(), cs.data(), nb.data(), bs.data(), ts, nw, w.data(), out3.data(), st3.data());
    const bool same = out1 == out3 && out2 == out3 && st1 == st3 && st2 == st3;
    printf("%d %d %d %d\n", a, b, c, same ? 1 : 0);
    return 0;
}
