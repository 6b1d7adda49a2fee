// tests/cpp/regions_test.cpp -- get_regions of compressed::channel<T> / image<T> / device_channel<T> / device_image<T>: many rectangles
// in one grouped engine call.  Results against plain loops over the source pixels: back to back in region order, region-major and
// channel-minor for images, each row-major with its subsampled shape; the span form checks its size; every region is checked before
// anything runs; an empty list does nothing.  tests/test_host_mirror_regions.py builds it against the emulator-backed mock of the C
// ABI (where the mock's call counter pins one engine call per get_regions) and against the library on the GPU.
#include <compressed/device_image.h>
#include <compressed/image.h>

#include <cstdio>
#include <cstring>
#include <string>

using namespace compressed;

#ifdef CIMG_MOCK_BACKEND
// (tests/emu/mock_window_grouped.cpp: window read calls of every kind, and the grouped ones among them)
extern "C" int64_t mock_window_calls(void);
extern "C" int64_t mock_grouped_window_calls(void);
static int64_t calls() { return mock_window_calls(); }
static bool all_grouped() { return mock_window_calls() == mock_grouped_window_calls(); }
#else
static int64_t calls() { return -1; }
static bool all_grouped() { return true; }
#endif

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)
#define CHECK_THROWS(T, expr) do { bool caught_ = false; try { expr; } catch (const T&) { caught_ = true; } catch (...) {} \
	if (!caught_) { std::printf("FAILED %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #T); ++g_failures; } } while (0)
// (one engine call on the mock, and this program reads through get_regions alone, so every window read call so far was a grouped
// one; nothing to count against the library)
#define CHECK_CALLS(before, n) CHECK(calls() < 0 || (calls() == (before) + (n) && all_grouped()))

template <typename T>
struct dev_array
{
	T* p; size_t n;
	explicit dev_array(size_t count) : p(static_cast<T*>(cimg_device_malloc(blosc2::batch::engine(), count * sizeof(T) + 1))), n(count) {}
	explicit dev_array(const std::vector<T>& h) : dev_array(h.size()) { cimg_memcpy_h2d(blosc2::batch::engine(), p, h.data(), n * sizeof(T)); }
	~dev_array() { cimg_device_free(blosc2::batch::engine(), p); }
	dev_array(const dev_array&) = delete;
	std::vector<T> host() const { std::vector<T> h(n); if (n) cimg_memcpy_d2h(blosc2::batch::engine(), h.data(), p, n * sizeof(T)); return h; }
};

constexpr size_t W = 512, H = 130, BLOCK = 4096;

template <typename T> static std::vector<T> pixels(unsigned seed)
{
	std::vector<T> v(W * H);
	uint32_t s = seed * 2654435761u + 1;
	for (size_t i = 0; i < v.size(); ++i)
	{
		s = s * 1664525u + 1013904223u;
		v[i] = static_cast<T>(((i % W) / 7) * 3 + ((i / W) / 5) * 11 + (s >> 30));
	}
	return v;
}

// the regions of every case: a row of tiles, crops over chunk boundaries and in the leftover chunk (one twice), subsampled ones,
// 1 x 1 regions, empty ones
static std::vector<region> cases()
{
	std::vector<region> r;
	for (size_t k = 0; k < 4; ++k) r.push_back({ 128 * k, 10, 128, 40 });
	r.push_back({ 200, 25, 100, 11 }); r.push_back({ 200, 25, 100, 11 }); r.push_back({ 412, 119, 100, 11 });
	r.push_back({ 0, 0, W, H, 7, 9 }); r.push_back({ 5, 58, 300, 29, 3, 1 }); r.push_back({ 17, 4, 71, 60, 3, 5 });
	r.push_back({ 0, 0, 1, 1 }); r.push_back({ W - 1, H - 1, 1, 1 }); r.push_back({ 77, 90, 1, 1, 4, 4 });
	r.push_back({ 10, 10, 0, 5 }); r.push_back({ 10, 10, 5, 0, 2, 2 });
	return r;
}

// what get_regions must give: planes[c] are the source pixels of channel c
template <typename T> static std::vector<T> expect(const std::vector<std::vector<T>>& planes, const std::vector<region>& regions)
{
	std::vector<T> out;
	for (const region& r : regions)
		for (const auto& p : planes)
			for (size_t y = r.y; y < r.y + r.height; y += r.step_y)
				for (size_t x = r.x; x < r.x + r.width; x += r.step_x) out.push_back(p[y * W + x]);
	return out;
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T> static void run(enums::codec codec)
{
	const size_t CHUNK = W * sizeof(T) * 30;                         // four chunks of 30 rows and a leftover chunk of 10
	std::vector<std::vector<T>> planes{ pixels<T>(1), pixels<T>(2), pixels<T>(3) };
	const std::vector<region> regions = cases();
	const std::vector<T> want1 = expect<T>({ planes[0] }, regions), want3 = expect<T>(planes, regions);
	const std::vector<region> none;
	const std::vector<region> bad{ { 0, 0, 4, 4 }, { W - 3, 0, 4, 4 } }, bad_step{ { 0, 0, 4, 4 }, { 0, 0, 4, 4, 0, 1 } };

	channel<T> ch(std::span<const T>(planes[0]), W, H, codec, 9, BLOCK, CHUNK);
	CHECK(ch.num_chunks() == 5);
	int64_t n = calls();
	CHECK(same(ch.get_regions(regions), want1));
	CHECK_CALLS(n, 1);
	std::vector<T> buf(want1.size() + 3, T(99));
	ch.get_regions(std::span<T>(buf), regions);
	CHECK(std::memcmp(buf.data(), want1.data(), want1.size() * sizeof(T)) == 0 && buf[want1.size()] == T(99));
	CHECK_THROWS(std::invalid_argument, ch.get_regions(std::span<T>(buf.data(), want1.size() - 1), regions));
	n = calls();
	CHECK(ch.get_regions(none).empty());
	CHECK_THROWS(std::out_of_range, ch.get_regions(bad));
	CHECK_THROWS(std::invalid_argument, ch.get_regions(bad_step));
	std::fill(buf.begin(), buf.end(), T(99));
	CHECK_THROWS(std::out_of_range, ch.get_regions(std::span<T>(buf), bad));
	CHECK(buf[0] == T(99) && buf[15] == T(99));                      // checked before anything runs
	CHECK_CALLS(n, 0);

	std::vector<std::span<const T>> spans;
	for (const auto& p : planes) spans.emplace_back(p);
	image<T> img(spans, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
	n = calls();
	CHECK(same(img.get_regions(regions), want3));
	CHECK_CALLS(n, 1);
	CHECK(img.get_regions(none).empty());
	CHECK_THROWS(std::out_of_range, img.get_regions(bad));
	CHECK_THROWS(std::invalid_argument, img.get_regions(std::span<T>(buf.data(), 5), regions));
	CHECK_CALLS(n, 1);

	dev_array<T> d0(planes[0]);
	device_channel<T> dch(d0.p, W, H, codec, 9, BLOCK, CHUNK);
	dev_array<T> out1(want1.size());
	n = calls();
	dch.get_regions(out1.p, regions);
	CHECK_CALLS(n, 1);
	CHECK(same(out1.host(), want1));
	dch.get_regions(out1.p, none);
	CHECK_THROWS(std::out_of_range, dch.get_regions(out1.p, bad));
	CHECK_THROWS(std::invalid_argument, dch.get_regions(out1.p, bad_step));
	CHECK_CALLS(n, 1);
	CHECK(same(out1.host(), want1));                                 // (the refused calls wrote nothing)

	std::vector<T> all;
	for (const auto& p : planes) all.insert(all.end(), p.begin(), p.end());
	dev_array<T> d3(all);
	std::vector<const T*> ptrs{ d3.p, d3.p + W * H, d3.p + 2 * W * H };
	device_image<T> dimg(ptrs, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
	dev_array<T> out3(want3.size());
	n = calls();
	dimg.get_regions(out3.p, regions);
	CHECK_CALLS(n, 1);
	CHECK(same(out3.host(), want3));
	dimg.get_regions(out3.p, none);
	CHECK_THROWS(std::out_of_range, dimg.get_regions(out3.p, bad));
	CHECK_CALLS(n, 1);
	// a channel handle of the image reads the same pixels
	dimg.channel(1).get_regions(out1.p, regions);
	CHECK(same(out1.host(), expect<T>({ planes[1] }, regions)));
}

int main()
{
	try
	{
		run<uint8_t>(enums::codec::lz4);
		run<uint16_t>(enums::codec::blosclz);
		run<float>(enums::codec::lz4);
		run<uint16_t>(enums::codec::zstd);
	}
	catch (const std::exception& e)
	{
		std::printf("FAILED: exception %s\n", e.what());
		++g_failures;
	}
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
