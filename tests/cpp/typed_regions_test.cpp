// tests/cpp/typed_regions_test.cpp -- typed region reads of compressed::device_channel<T> / device_image<T>: get_region<U> and
// get_regions<U> with scale / offset, planar and pixel-major, over cimg_decompress_windows_typed_device.  Every result is compared
// bit for bit with plain loops over the source pixels: float results with the two-step (float)v * scale, then + offset (this file is
// built with -ffp-contract=off); half results only where the value is exact in float16, through half's exact widening to float
// (the rounding itself is checked against numpy in tests/test_emu_windows_typed.py and tests/test_python_windows_typed.py).  Bytes
// around a result must stay as they were.  tests/test_host_mirror_typed.py builds it against the emulator-backed mock of the C ABI
// (tests/emu/mock_window_typed.cpp) and against the library on the GPU.
#include <compressed/device_image.h>
#include <compressed/image.h>

#include <cstdio>
#include <cstring>
#include <string>

using namespace compressed;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)
#define CHECK_THROWS(T, expr) do { bool caught_ = false; try { expr; } catch (const T&) { caught_ = true; } catch (...) {} \
	if (!caught_) { std::printf("FAILED %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #T); ++g_failures; } } while (0)

template <typename T>
struct dev_array
{
	T* p; size_t n;
	explicit dev_array(size_t count) : p(static_cast<T*>(cimg_device_malloc(blosc2::batch::engine(), count * sizeof(T) + 16))), n(count) {}
	explicit dev_array(const std::vector<T>& h) : dev_array(h.size()) { cimg_memcpy_h2d(blosc2::batch::engine(), p, h.data(), n * sizeof(T)); }
	~dev_array() { cimg_device_free(blosc2::batch::engine(), p); }
	dev_array(const dev_array&) = delete;
	std::vector<T> host() const { std::vector<T> h(n); if (n) cimg_memcpy_d2h(blosc2::batch::engine(), h.data(), p, n * sizeof(T)); return h; }
};

constexpr size_t W = 512, H = 130, BLOCK = 4096;

template <typename T> static std::vector<T> pixels(unsigned seed, size_t count = W * H)
{
	std::vector<T> v(count);
	uint32_t s = seed * 2654435761u + 1;
	for (size_t i = 0; i < v.size(); ++i)
	{
		s = s * 1664525u + 1013904223u;
		const uint32_t val = static_cast<uint32_t>(((i % W) / 7) * 3 + ((i / W) / 5) * 11 + (s >> 30) + seed);       // (at most 511: exact in every type but the 8-bit ones, which wrap)
		if constexpr (std::is_integral_v<T>) v[i] = static_cast<T>(val);
		else v[i] = static_cast<T>(static_cast<float>(val));
	}
	return v;
}

// tiles that share rows, overlapping crops over chunk boundaries, subsampled ones, 1 x 1 regions, empty ones
static std::vector<region> cases()
{
	std::vector<region> r;
	for (size_t k = 0; k < 4; ++k) r.push_back({ 128 * k, 10, 128, 40 });
	r.push_back({ 200, 25, 100, 11 }); r.push_back({ 210, 28, 100, 11, 2, 1 }); r.push_back({ 412, 119, 100, 11 });
	r.push_back({ 0, 0, W, H, 7, 9 }); r.push_back({ 5, 58, 300, 29, 3, 1 }); r.push_back({ 17, 4, 71, 60, 3, 5 });
	r.push_back({ 0, 0, 1, 1 }); r.push_back({ W - 1, H - 1, 1, 1 }); r.push_back({ 77, 90, 1, 1, 4, 4 });
	r.push_back({ 10, 10, 0, 5 }); r.push_back({ 10, 10, 5, 0, 2, 2 });
	return r;
}
static size_t elems(const std::vector<region>& regions) { size_t n = 0; for (const region& r : regions) n += r.out_elems(); return n; }

// what one element becomes: the stored value itself, or two float steps (and, for half, a value that float16 holds exactly)
template <typename T, typename U> static U convert(T v, float scale, float offset)
{
	if constexpr (std::is_same_v<T, U>) if (scale == 1.0f && offset == 0.0f) return v;
	float y = static_cast<float>(v) * scale;
	y = y + offset;
	return static_cast<U>(y);
}
// the regions of `planes` as get_regions lays them out: region-major; planar (channel-minor planes) or pixel-major within a region
template <typename T, typename U>
static std::vector<U> expect(const std::vector<std::vector<T>>& planes, const std::vector<region>& regions, const std::vector<float>& scales,
	const std::vector<float>& offsets, bool interleaved)
{
	const size_t C = planes.size();
	std::vector<U> out(elems(regions) * C);
	size_t at = 0;
	for (const region& r : regions)
	{
		const size_t n = r.out_elems();
		for (size_t c = 0; c < C; ++c)
		{
			const float sc = scales[scales.size() == 1 ? 0 : c], of = offsets[offsets.size() == 1 ? 0 : c];
			size_t k = 0;
			for (size_t y = r.y; y < r.y + r.height; y += r.step_y)
				for (size_t x = r.x; x < r.x + r.width; x += r.step_x, ++k)
					out[interleaved ? at + k * C + c : at + c * n + k] = convert<T, U>(planes[c][y * W + x], sc, of);
		}
		at += n * C;
	}
	return out;
}
template <typename U> static bool same(const std::vector<U>& a, const std::vector<U>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(U)) == 0);
}

// T stored, U read; the scales keep half results exact (small integers and halves of them)
template <typename T, typename U> static void run(enums::codec codec, float s0, float o0)
{
	const size_t CHUNK = W * sizeof(T) * 30;                         // four chunks of 30 rows and a leftover chunk of 10
	const std::vector<std::vector<T>> planes{ pixels<T>(1), pixels<T>(2), pixels<T>(3) };
	const std::vector<region> regions = cases(), none;
	const bool ident = std::is_same_v<T, U> && s0 == 1.0f && o0 == 0.0f;
	const std::vector<float> one_s{ s0 }, one_o{ o0 };
	const std::vector<float> per_s = ident ? std::vector<float>{ 1.0f, 1.0f, 1.0f } : std::vector<float>{ s0, 0.5f, 2.0f };
	const std::vector<float> per_o = ident ? std::vector<float>{ 0.0f, 0.0f, 0.0f } : std::vector<float>{ o0, -3.0f, 0.25f };

	// ---- device_channel ----
	{
		dev_array<T> d0(planes[0]);
		device_channel<T> dch(d0.p, W, H, codec, 9, BLOCK, CHUNK);
		const std::vector<std::vector<T>> p1{ planes[0] };
		const region r{ 17, 4, 71, 60, 3, 5 };
		dev_array<U> one(std::vector<U>(r.out_elems() + 8, U{}));
		dch.get_region(one.p + 4, r.x, r.y, r.width, r.height, r.step_x, r.step_y, s0, o0);
		std::vector<U> got = one.host();
		CHECK(same(std::vector<U>(got.begin() + 4, got.end() - 4), expect<T, U>(p1, { r }, one_s, one_o, false)));
		for (size_t k = 0; k < 4; ++k) CHECK(std::memcmp(&got[k], &got[got.size() - 1 - k], sizeof(U)) == 0 && static_cast<float>(got[k]) == 0.0f);
		dev_array<U> many(elems(regions));
		dch.get_regions(many.p, std::span<const region>(regions), s0, o0);
		CHECK(same(many.host(), expect<T, U>(p1, regions, one_s, one_o, false)));
		dch.get_regions(many.p, std::span<const region>(none), s0, o0);          // an empty batch does nothing
		const std::vector<region> bad{ { 0, 0, 4, 4 }, { W - 3, 0, 4, 4 } }, bad_step{ { 0, 0, 4, 4, 0, 1 } };
		CHECK_THROWS(std::out_of_range, dch.get_regions(many.p, std::span<const region>(bad), s0, o0));
		CHECK_THROWS(std::invalid_argument, dch.get_regions(many.p, std::span<const region>(bad_step), s0, o0));
#ifndef CIMG_MOCK_BACKEND                                                      // (the mock's device memory is host memory)
		std::vector<U> on_host(16);
		CHECK_THROWS(std::invalid_argument, dch.get_region(on_host.data(), 0, 0, 4, 4, 1, 1, s0, o0));
#endif
		if constexpr (std::is_same_v<T, U> && !std::is_same_v<U, float> && !std::is_same_v<U, half>)
			CHECK_THROWS(std::invalid_argument, dch.get_region(many.p, 0, 0, 4, 4, 1, 1, 2.0f, 0.0f));
	}
	// ---- device_image: per-channel scale and offset, planar and pixel-major ----
	{
		std::vector<T> all;
		for (const auto& p : planes) all.insert(all.end(), p.begin(), p.end());
		dev_array<T> dall(all);
		device_image<T> dimg(std::vector<const T*>{ dall.p, dall.p + W * H, dall.p + 2 * W * H }, W, H, {}, codec, 9, BLOCK, CHUNK);
		for (const bool il : { false, true })
		{
			dev_array<U> out(elems(regions) * 3);
			dimg.get_regions(out.p, std::span<const region>(regions), std::span<const float>(per_s), std::span<const float>(per_o), il);
			CHECK(same(out.host(), expect<T, U>(planes, regions, per_s, per_o, il)));
			dimg.get_regions(out.p, std::span<const region>(regions), std::span<const float>(one_s), std::span<const float>(one_o), il);
			CHECK(same(out.host(), expect<T, U>(planes, regions, one_s, one_o, il)));
			const region r{ 100, 20, 224, 64, 1, 1 };
			dev_array<U> one(std::vector<U>(r.out_elems() * 3 + 2, U{}));
			dimg.get_region(one.p + 1, r.x, r.y, r.width, r.height, r.step_x, r.step_y, std::span<const float>(per_s), std::span<const float>(per_o), il);   // (no 16-byte rule)
			std::vector<U> got = one.host();
			CHECK(same(std::vector<U>(got.begin() + 1, got.end() - 1), expect<T, U>(planes, { r }, per_s, per_o, il)));
			CHECK(static_cast<float>(got.front()) == 0.0f && static_cast<float>(got.back()) == 0.0f);
			dimg.get_regions(out.p, std::span<const region>(none), std::span<const float>(per_s), std::span<const float>(per_o), il);
		}
		dev_array<U> out(elems(regions) * 3);
		const std::vector<float> two{ 1.0f, 1.0f };
		CHECK_THROWS(std::invalid_argument, dimg.get_regions(out.p, std::span<const region>(regions), std::span<const float>(two), std::span<const float>(one_o)));
		CHECK_THROWS(std::invalid_argument, dimg.get_regions(out.p, std::span<const region>(regions), std::span<const float>(one_s), std::span<const float>(two)));
		const std::vector<region> bad{ { 0, H - 3, 4, 4 } };
		CHECK_THROWS(std::out_of_range, dimg.get_regions(out.p, std::span<const region>(bad), std::span<const float>(one_s), std::span<const float>(one_o), true));
		// the existing pixel-major route gives the same bytes as the identity typed read
		if (ident)
		{
			const region r{ 96, 20, 224, 64, 1, 1 };
			dev_array<T> a(r.out_elems() * 3), b(r.out_elems() * 3);
			dimg.get_region(a.p, r.x, r.y, r.width, r.height, true);
			dimg.get_region(b.p, r.x, r.y, r.width, r.height, 1, 1, std::span<const float>(one_s), std::span<const float>(one_o), true);
			CHECK(same(a.host(), b.host()));
		}
	}
	std::printf("typed regions <%zu -> %zu bytes, codec %d>: %d failures so far\n", sizeof(T), sizeof(U), static_cast<int>(codec), g_failures);
}

int main()
{
	run<uint8_t, float>(enums::codec::lz4, 1.0f / 255.0f, -0.4851f);
	run<uint8_t, half>(enums::codec::blosclz, 0.5f, 1.0f);
	run<uint16_t, float>(enums::codec::zstd, 1.0f / 65535.0f, 0.406f);
	run<int16_t, half>(enums::codec::lz4, 0.5f, -8.0f);
	run<float, float>(enums::codec::lz4, 1.0f / 58.395f, -2.1179f);
	run<float, half>(enums::codec::lz4, 0.25f, 1.0f);
	run<half, float>(enums::codec::lz4, 1.0f / 3.0f, 0.1f);
	run<half, half>(enums::codec::lz4, 1.0f, 0.0f);
	run<uint8_t, uint8_t>(enums::codec::lz4, 1.0f, 0.0f);
	run<int32_t, int32_t>(enums::codec::blosclz, 1.0f, 0.0f);
	run<double, float>(enums::codec::lz4, 1.0f / 7.0f, 0.3f);
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
