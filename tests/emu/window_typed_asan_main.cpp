// tests/emu/window_typed_asan_main.cpp -- TEST INFRASTRUCTURE: one typed window call from a case file, for the AddressSanitizer /
// UBSan build of window_typed_emu.cpp (tests/test_emu_windows_typed.py): planner, grouping, unit order and kernel body on the host
// lane emulator (host code only).  The file holds: int64 nchunks, typesize, output size, nwindows; int64 comp_off[n]; int32
// comp_size[n], nbytes[n], blocksize[n]; nwindows cimg_window_typed; int64 buffer size; the buffer.  Every buffer is a heap
// allocation of exactly its size (the emulator's own tables too: window_typed_env.h); the output is filled with 0xA5 first.
// Prints the return code and the status words on one line and writes the output to the path given as the second argument.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int wnemu_windows_typed_device(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                               const int32_t* blocksize, int typesize, int nwindows, const void* w, uint8_t* out, int32_t* status);
void emu_set_write_order(int o);
}

struct Win {
    int32_t chunk_first, chunk_count; int64_t origin, row_pitch, col_pitch; int32_t width, height; int64_t out_off, out_pitch;
    int64_t elem_pitch; int32_t src_type, out_type; float scale, offset;
};
static_assert(sizeof(Win) == 80, "cimg_window_typed");

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
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
    emu_set_write_order(argc > 3 ? argv[3][0] - '0' : 0);
    std::vector<int32_t> st((size_t)n);
    std::vector<uint8_t> out((size_t)hdr[2], 0xA5);
    const int rc = wnemu_windows_typed_device(n, buf.data(), off.data(), cs.data(), nb.data(), bs.data(), ts, nw, w.data(), out.data(), st.data());
    printf("%d", rc);
    for (int i = 0; i < n; i++) printf(" %d", st[(size_t)i]);
    printf("\n");
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    if (!out.empty() && fwrite(out.data(), 1, out.size(), g) != out.size()) return 2;
    fclose(g);
    return 0;
}
