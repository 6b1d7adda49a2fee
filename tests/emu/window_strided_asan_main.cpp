// tests/emu/window_strided_asan_main.cpp -- TEST INFRASTRUCTURE: one strided window call from a case file, for the AddressSanitizer /
// UBSan build of window_strided_emu.cpp (tests/test_emu_windows_strided.py).  The file holds: int64 nchunks, typesize, output
// size; int64 comp_off[n]; int32 comp_size[n], nbytes[n], blocksize[n]; one cimg_window_strided; int64 buffer size; the buffer.
// The window runs through the device-style and the host-style call, each into an output of exactly the given size; prints both
// return codes.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int wnemu_windows_strided_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                 const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
int wnemu_windows_strided_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                               const void* w, uint8_t* out, int32_t* status);
}

struct Win { int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch; };

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[3];
    if (!rd(f, hdr, 3)) return 2;
    const int n = (int)hdr[0], ts = (int)hdr[1];
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> cs((size_t)n), nb((size_t)n), bs((size_t)n);
    Win w;
    int64_t bytes = 0;
    if (!rd(f, off.data(), (size_t)n) || !rd(f, cs.data(), (size_t)n) || !rd(f, nb.data(), (size_t)n) || !rd(f, bs.data(), (size_t)n)) return 2;
    if (!rd(f, &w.chunk_first, 2) || !rd(f, &w.origin, 3) || !rd(f, &w.width, 2) || !rd(f, &w.out_off, 2) || !rd(f, &bytes, 1)) return 2;
    std::vector<uint8_t> buf((size_t)bytes);
    if (!rd(f, buf.data(), (size_t)bytes)) return 2;
    fclose(f);
    std::vector<int32_t> st((size_t)n);
    std::vector<uint8_t> out1((size_t)hdr[2]), out2((size_t)hdr[2]);
    const int a = wnemu_windows_strided_device(n, buf.data(), off.data(), cs.data(), nb.data(), bs.data(), ts, 1, &w, out1.data(), st.data());
    const int b = wnemu_windows_strided_host(n, buf.data(), off.data(), cs.data(), 1, &w, out2.data(), st.data());
    printf("%d %d\n", a, b);
    return 0;
}
