// tests/cpp/typed_region_writes_test.cpp -- typed region writes of compressed::device_channel<T> / device_image<T>: set_region<U> and
// set_regions<U> with scale / offset, planar and pixel-major sources, over cimg_update_windows_typed_device.  After every write the
// whole plane is decoded and compared bit for bit with plain loops over a copy of the pixels: t = ((float)y - offset) / scale in two
// float steps (this file is built with -ffp-contract=off), then nearbyint saturated to T's range for integer pixels, t for float
// pixels; half sources and half pixels only with values float16 holds exactly (the rounding itself is checked against numpy in
// tests/test_emu_window_writes_typed.py and tests/test_python_window_writes_typed.py).  tests/test_host_mirror_typed_writes.py builds
// it against the emulator-backed mock of the C ABI (tests/emu/mock_window_write_typed.cpp) and against the library on the GPU.
#include <compressed/device_image.h>
#include <compressed/image.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

template <typename T> static std::vector<T> pixels(unsigned seed)
{
	std::vector<T> v(W * H);
	uint32_t s = seed * 2654435761u + 1;
	for (size_t i = 0; i < v.size(); ++i)
	{
		s = s * 1664525u + 1013904223u;
		const uint32_t val = static_cast<uint32_t>(((i % W) / 7) * 3 + ((i / W) / 5) * 11 + (s >> 30) + seed);
		if constexpr (std::is_integral_v<T>) v[i] = static_cast<T>(val);
		else v[i] = static_cast<T>(static_cast<float>(val));
	}
	return v;
}

// overlapping crops over chunk boundaries (the later wins), subsampled ones, 1 x 1 regions, empty ones
static std::vector<region> cases()
{
	std::vector<region> r;
	for (size_t k = 0; k < 4; ++k) r.push_back({ 128 * k, 10, 128, 40 });
	r.push_back({ 200, 25, 100, 11 }); r.push_back({ 210, 28, 100, 11, 2, 1 }); r.push_back({ 412, 119, 100, 11 });
	r.push_back({ 5, 58, 300, 29, 3, 1 }); r.push_back({ 17, 4, 71, 60, 3, 5 });
	r.push_back({ 0, 0, 1, 1 }); r.push_back({ W - 1, H - 1, 1, 1 }); r.push_back({ 77, 90, 1, 1, 4, 4 });
	r.push_back({ 10, 10, 0, 5 }); r.push_back({ 10, 10, 5, 0, 2, 2 });
	return r;
}
static size_t elems(const std::vector<region>& regions) { size_t n = 0; for (const region& r : regions) n += r.out_elems(); return n; }

// what a source element becomes in a plane of T
template <typename T, typename U> static T unconvert(U y, float scale, float offset)
{
	if constexpr (std::is_same_v<T, U>) if (scale == 1.0f && offset == 0.0f) return y;
	float t = static_cast<float>(y) - offset;
	t = t / scale;
	if constexpr (std::is_integral_v<T>)
	{
		if (std::isnan(t)) return T{};
		const double r = std::nearbyint(static_cast<double>(t));
		const double lo = static_cast<double>(std::numeric_limits<T>::min()), hi = static_cast<double>(std::numeric_limits<T>::max());
		return static_cast<T>(r < lo ? lo : r > hi ? hi : r);
	}
	else return static_cast<T>(t);
}

// source values: quarter steps around T's range for float sources (ties and both saturation edges); for half sources and half
// pixels, values that stay exact in float16 through the conversion (the callers choose power-of-two scales for them)
template <typename T, typename U> static std::vector<U> source(size_t n, float scale, float offset, unsigned seed)
{
	std::vector<U> v(n);
	uint32_t s = seed * 747796405u + 1;
	for (size_t i = 0; i < n; ++i)
	{
		s = s * 1664525u + 1013904223u;
		if constexpr (std::is_same_v<T, U>) { v[i] = static_cast<U>(static_cast<float>((s >> 20) % 200)); continue; }
		const bool exact = std::is_same_v<U, half> || std::is_same_v<T, half>;
		const float stored = exact ? static_cast<float>(static_cast<int>((s >> 16) % 300) - 20) : static_cast<float>(static_cast<int>((s >> 12) % 70000) - 2000) * 0.25f;
		float y = stored * scale;
		y = y + offset;
		v[i] = static_cast<U>(y);
	}
	return v;
}

// the regions written into `planes` from a source laid out as set_regions takes it
template <typename T, typename U>
static void apply(std::vector<std::vector<T>>& planes, const std::vector<region>& regions, const std::vector<U>& src, const std::vector<float>& scales,
	const std::vector<float>& offsets, bool interleaved)
{
	const size_t C = planes.size();
	size_t at = 0;
	for (const region& r : regions)
	{
		const size_t n = r.out_elems();
		for (size_t c = 0; c < C && n; ++c)
		{
			const float sc = scales[scales.size() == 1 ? 0 : c], of = offsets[offsets.size() == 1 ? 0 : c];
			size_t k = 0;
			for (size_t y = r.y; y < r.y + r.height; y += r.step_y)
				for (size_t x = r.x; x < r.x + r.width; x += r.step_x, ++k)
					planes[c][y * W + x] = unconvert<T, U>(src[interleaved ? at + k * C + c : at + c * n + k], sc, of);
		}
		at += n * C;
	}
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

// T stored, U in memory
template <typename T, typename U> static void run(enums::codec codec, float s0, float o0)
{
	const size_t CHUNK = W * sizeof(T) * 30;                         // four chunks of 30 rows and a leftover chunk of 10
	const std::vector<std::vector<T>> planes{ pixels<T>(1), pixels<T>(2), pixels<T>(3) };
	const std::vector<region> regions = cases(), none;
	const bool ident = std::is_same_v<T, U> && s0 == 1.0f && o0 == 0.0f;
	const std::vector<float> one_s{ s0 }, one_o{ o0 };
	const std::vector<float> per_s = ident ? std::vector<float>{ 1.0f, 1.0f, 1.0f } : std::vector<float>{ s0, 0.5f, -2.0f };
	const std::vector<float> per_o = ident ? std::vector<float>{ 0.0f, 0.0f, 0.0f } : std::vector<float>{ o0, -3.0f, 0.25f };

	// ---- device_channel ----
	{
		dev_array<T> d0(planes[0]);
		device_channel<T> dch(d0.p, W, H, codec, 9, BLOCK, CHUNK);
		std::vector<std::vector<T>> edited{ planes[0] };
		const region r{ 17, 4, 71, 60, 3, 5 };
		const std::vector<U> one = source<T, U>(r.out_elems(), s0, o0, 5);
		dev_array<U> done(one);
		dch.set_region(done.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y, s0, o0);
		apply<T, U>(edited, { r }, one, one_s, one_o, false);
		dev_array<T> back(W * H);
		dch.decompress_into(back.p);
		CHECK(same(back.host(), edited[0]));
		const std::vector<U> many = source<T, U>(elems(regions), s0, o0, 6);
		dev_array<U> dmany(many);
		dch.set_regions(std::span<const region>(regions), dmany.p, s0, o0);
		apply<T, U>(edited, regions, many, one_s, one_o, false);
		dch.decompress_into(back.p);
		CHECK(same(back.host(), edited[0]));
		dch.set_regions(std::span<const region>(none), dmany.p, s0, o0);        // an empty batch does nothing
		const std::vector<region> bad{ { 0, 0, 4, 4 }, { W - 3, 0, 4, 4 } }, bad_step{ { 0, 0, 4, 4, 0, 1 } };
		CHECK_THROWS(std::out_of_range, dch.set_regions(std::span<const region>(bad), dmany.p, s0, o0));
		CHECK_THROWS(std::invalid_argument, dch.set_regions(std::span<const region>(bad_step), dmany.p, s0, o0));
		CHECK_THROWS(std::invalid_argument, dch.set_region(dmany.p, 0, 0, 4, 4, 1, 1, 0.0f, o0));
		CHECK_THROWS(std::invalid_argument, dch.set_region(dmany.p, 0, 0, 4, 4, 1, 1, std::numeric_limits<float>::infinity(), o0));
		CHECK_THROWS(std::invalid_argument, dch.set_region(dmany.p, 0, 0, 4, 4, 1, 1, s0, std::nanf("")));
#ifndef CIMG_MOCK_BACKEND                                                      // (the mock's device memory is host memory)
		std::vector<U> on_host(16);
		CHECK_THROWS(std::invalid_argument, dch.set_region(on_host.data(), 0, 0, 4, 4, 1, 1, s0, o0));
#endif
		if constexpr (std::is_same_v<T, U> && !std::is_same_v<U, float> && !std::is_same_v<U, half>)
			CHECK_THROWS(std::invalid_argument, dch.set_region(dmany.p, 0, 0, 4, 4, 1, 1, 2.0f, 0.0f));
		dch.decompress_into(back.p);
		CHECK(same(back.host(), edited[0]));                                    // a refused call changes nothing
	}
	// ---- device_image: per-channel scale and offset, planar and pixel-major sources ----
	for (const bool il : { false, true })
	{
		std::vector<T> all;
		for (const auto& p : planes) all.insert(all.end(), p.begin(), p.end());
		dev_array<T> dall(all);
		device_image<T> dimg(std::vector<const T*>{ dall.p, dall.p + W * H, dall.p + 2 * W * H }, W, H, {}, codec, 9, BLOCK, CHUNK);
		std::vector<std::vector<T>> edited = planes;
		auto check = [&]() {
			dev_array<T> back(3 * W * H);
			dimg.decompress_into(back.p);
			const std::vector<T> got = back.host();
			for (size_t c = 0; c < 3; ++c) CHECK(std::memcmp(got.data() + c * W * H, edited[c].data(), W * H * sizeof(T)) == 0);
		};
		// (one source serves all three channels: its values follow channel 0's pair, the other channels saturate or round -- all the better)
		const std::vector<U> many = source<T, U>(elems(regions) * 3, s0, o0, il ? 8 : 7);
		dev_array<U> dmany(many);
		const bool float_pixels = !std::is_integral_v<T>;
		const std::vector<float>& ps = float_pixels && !ident ? one_s : per_s;  // (float pixels from other pairs would need float16's rounding here)
		const std::vector<float>& po = float_pixels && !ident ? one_o : per_o;
		dimg.set_regions(std::span<const region>(regions), dmany.p, std::span<const float>(ps), std::span<const float>(po), il);
		apply<T, U>(edited, regions, many, ps, po, il);
		check();
		const region r{ 100, 20, 224, 64, 1, 1 };
		const std::vector<U> one = source<T, U>(r.out_elems() * 3, s0, o0, 9);
		dev_array<U> done(one);
		dimg.set_region(done.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y, std::span<const float>(one_s), std::span<const float>(one_o), il);
		apply<T, U>(edited, { r }, one, one_s, one_o, il);
		check();
		dimg.set_regions(std::span<const region>(none), dmany.p, std::span<const float>(per_s), std::span<const float>(per_o), il);
		const std::vector<float> two{ 1.0f, 1.0f }, zero{ s0, 0.0f, 1.0f };
		CHECK_THROWS(std::invalid_argument, dimg.set_regions(std::span<const region>(regions), dmany.p, std::span<const float>(two), std::span<const float>(one_o), il));
		CHECK_THROWS(std::invalid_argument, dimg.set_regions(std::span<const region>(regions), dmany.p, std::span<const float>(one_s), std::span<const float>(two), il));
		CHECK_THROWS(std::invalid_argument, dimg.set_regions(std::span<const region>(regions), dmany.p, std::span<const float>(zero), std::span<const float>(one_o), il));
		const std::vector<region> bad{ { 0, H - 3, 4, 4 } };
		CHECK_THROWS(std::out_of_range, dimg.set_regions(std::span<const region>(bad), dmany.p, std::span<const float>(one_s), std::span<const float>(one_o), il));
		check();
	}
	std::printf("typed region writes <%zu <- %zu bytes, codec %d>: %d failures so far\n", sizeof(T), sizeof(U), static_cast<int>(codec), g_failures);
}

int main()
{
	run<uint8_t, float>(enums::codec::lz4, 1.0f / 255.0f, -0.4851f);
	run<uint8_t, half>(enums::codec::blosclz, 0.5f, 1.0f);
	run<uint16_t, float>(enums::codec::zstd, 1.0f / 65535.0f, 0.406f);
	run<int16_t, half>(enums::codec::lz4, 0.5f, -8.0f);
	run<int32_t, float>(enums::codec::lz4, 1.0f / 3.0f, 0.1f);
	run<float, float>(enums::codec::lz4, 1.0f / 58.395f, -2.1179f);
	run<float, half>(enums::codec::lz4, 0.25f, 1.0f);
	run<half, float>(enums::codec::lz4, 0.5f, 2.0f);
	run<half, half>(enums::codec::lz4, 1.0f, 0.0f);
	run<uint8_t, uint8_t>(enums::codec::lz4, 1.0f, 0.0f);
	run<int32_t, int32_t>(enums::codec::blosclz, 1.0f, 0.0f);
	run<double, double>(enums::codec::lz4, 1.0f, 0.0f);
	{
		// float64 pixels are written from float64 only
		const std::vector<double> p = pixels<double>(1);
		dev_array<double> d(p);
		device_channel<double> dch(d.p, W, H, enums::codec::lz4, 9, BLOCK, W * 8 * 30);
		dev_array<float> f(std::vector<float>(16, 1.0f));
		CHECK_THROWS(std::invalid_argument, dch.set_region(f.p, 0, 0, 4, 4, 1, 1, 1.0f, 0.0f));
	}
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
