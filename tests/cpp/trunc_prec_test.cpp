// tests/cpp/trunc_prec_test.cpp -- the mantissa_bits parameter of compressed::channel<T> / image<T> / device_channel<T> / device_image<T>
// (lossy float storage through blosc2's trunc-prec filter).  `checks`: the argument checks, which need no codec (run against the
// emulator-backed mock of the C ABI, which refuses the filter itself).  `all`: the checks and the round trips, against the library
// on the GPU.  tests/test_host_mirror_trunc.py builds both.
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
	explicit dev_array(const std::vector<T>& h) : p(static_cast<T*>(cimg_device_malloc(blosc2::batch::engine(), h.size() * sizeof(T)))), n(h.size())
	{
		cimg_memcpy_h2d(blosc2::batch::engine(), p, h.data(), n * sizeof(T));
	}
	~dev_array() { cimg_device_free(blosc2::batch::engine(), p); }
	dev_array(const dev_array&) = delete;
	std::vector<T> host() const { std::vector<T> h(n); cimg_memcpy_d2h(blosc2::batch::engine(), h.data(), p, n * sizeof(T)); return h; }
};

static std::vector<float> pixels(size_t w, size_t h, unsigned seed)
{
	std::vector<float> v(w * h);
	uint32_t s = seed * 2654435761u + 1;
	for (size_t i = 0; i < v.size(); ++i)
	{
		s = s * 1664525u + 1013904223u;
		v[i] = static_cast<float>((i % w) / 7) * 0.25f + static_cast<float>(s >> 8) / 16777216.0f;      // noise in every mantissa bit
	}
	return v;
}
static std::vector<float> trunc(std::vector<float> v, int bits)
{
	for (float& f : v)
	{
		uint32_t u;
		std::memcpy(&u, &f, 4);
		u &= ~((1u << (23 - bits)) - 1u);
		std::memcpy(&f, &u, 4);
	}
	return v;
}
static bool same(const std::vector<float>& a, const std::vector<float>& b)
{
	return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

constexpr size_t W = 300, H = 90, BLOCK = 4096, CHUNK = W * 4 * 13;

static void checks()
{
	const std::vector<float> f = pixels(W, H, 1);
	const std::vector<uint16_t> u(W * H, 7);
	const std::vector<half> hf(W * H);
	using fspan = std::span<const float>;
	// a non-float T, and values outside 1 .. M: std::invalid_argument, before anything is compressed
	CHECK_THROWS(std::invalid_argument, channel<uint16_t>(std::span<const uint16_t>(u), W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 5));
	CHECK_THROWS(std::invalid_argument, channel<float>(fspan(f), W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 0));
	CHECK_THROWS(std::invalid_argument, channel<float>(fspan(f), W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 24));
	CHECK_THROWS(std::invalid_argument, channel<float>(fspan(f), W, H, enums::codec::lz4, 9, BLOCK, CHUNK, -12));
	CHECK_THROWS(std::invalid_argument, channel<half>(std::span<const half>(hf), W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 11));
	CHECK_THROWS(std::invalid_argument, image<float>(std::vector<fspan>{ fspan(f) }, W, H, {}, enums::codec::lz4, 9, BLOCK, CHUNK, 24));
	CHECK_THROWS(std::invalid_argument, image<uint16_t>(std::vector<std::span<const uint16_t>>{ std::span<const uint16_t>(u) }, W, H, {},
		enums::codec::lz4, 9, BLOCK, CHUNK, 3));
	{
		image<float> img(std::vector<fspan>{ fspan(f) }, W, H, {}, enums::codec::lz4, 9, BLOCK, CHUNK);
		CHECK(!img.mantissa_bits());
		CHECK_THROWS(std::invalid_argument, img.add_channel(fspan(f), W, H, std::nullopt, enums::codec::lz4, 5, 0));
		CHECK(img.num_channels() == 1);
	}
	{
		dev_array<float> d(f);
		dev_array<uint16_t> du(u);
		CHECK_THROWS(std::invalid_argument, device_channel<float>(d.p, W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 0));
		CHECK_THROWS(std::invalid_argument, device_channel<float>(d.p, W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 24));
		CHECK_THROWS(std::invalid_argument, device_channel<uint16_t>(du.p, W, H, enums::codec::lz4, 9, BLOCK, CHUNK, 5));
		CHECK_THROWS(std::invalid_argument, device_image<float>(std::vector<const float*>{ d.p }, W, H, {}, enums::codec::lz4, 9, BLOCK, CHUNK, 24));
		CHECK_THROWS(std::invalid_argument, device_image<uint16_t>(std::vector<const uint16_t*>{ du.p }, W, H, {}, enums::codec::lz4, 9, BLOCK, CHUNK, 5));
	}
	// without the parameter nothing changes
	channel<float> plain(fspan(f), W, H, enums::codec::lz4, 9, BLOCK, CHUNK);
	CHECK(!plain.mantissa_bits());
	CHECK(same(plain.get_decompressed(), f));
}

static void round_trips()
{
	const int m = 12;
	const std::vector<float> f = pixels(W, H, 2), want = trunc(f, m);
	CHECK(!same(f, want));
	for (const auto codec : { enums::codec::lz4, enums::codec::blosclz, enums::codec::zstd })
	{
		channel<float> ch(std::span<const float>(f), W, H, codec, 9, BLOCK, CHUNK, m);
		CHECK(ch.mantissa_bits() && *ch.mantissa_bits() == m);
		CHECK(same(ch.get_decompressed(), want));
		// set_chunk, the iterator's write-back and set_region truncate too
		std::vector<float> edited = want;
		std::vector<float> fresh = pixels(ch.chunk_elems(1), 1, 3);
		ch.set_chunk(std::span<float>(fresh), 1);
		const std::vector<float> tf = trunc(pixels(ch.chunk_elems(1), 1, 3), m);
		std::copy(tf.begin(), tf.end(), edited.begin() + static_cast<std::ptrdiff_t>(ch.chunk_elems(0)));
		CHECK(same(ch.get_decompressed(), edited));
		size_t at = 0;
		for (auto chunk : ch)
		{
			for (auto& v : chunk) v = v * 1.0009765625f + 0.001f;
			for (size_t k = 0; k < chunk.size(); ++k) edited[at + k] = edited[at + k] * 1.0009765625f + 0.001f;
			at += chunk.size();
		}
		edited = trunc(edited, m);
		CHECK(same(ch.get_decompressed(), edited));
		const std::vector<float> patch = pixels(120, 33, 4), tp = trunc(patch, m);
		ch.set_region(std::span<const float>(patch), 40, 20, 120, 33);
		for (size_t r = 0; r < 33; ++r) std::copy(tp.begin() + static_cast<std::ptrdiff_t>(r * 120), tp.begin() + static_cast<std::ptrdiff_t>((r + 1) * 120),
			edited.begin() + static_cast<std::ptrdiff_t>((20 + r) * W + 40));
		CHECK(same(ch.get_decompressed(), edited));
		// the device class, and the parameter's way through from_channel / to_channel
		dev_array<float> d(f);
		device_channel<float> dc(d.p, W, H, codec, 9, BLOCK, CHUNK, m);
		CHECK(dc.mantissa_bits() && *dc.mantissa_bits() == m);
		CHECK(same(d.host(), f));                                          // the caller's pixels are not modified
		CHECK(same(dc.to_channel().get_decompressed(), want));
		CHECK(dc.to_channel().mantissa_bits() == std::optional<int>(m));
		device_channel<float> up = device_channel<float>::from_channel(ch);
		CHECK(up.mantissa_bits() == std::optional<int>(m));
		dev_array<float> dp(patch);
		up.set_region(dp.p, 0, 0, 120, 33);
		for (size_t r = 0; r < 33; ++r) std::copy(tp.begin() + static_cast<std::ptrdiff_t>(r * 120), tp.begin() + static_cast<std::ptrdiff_t>((r + 1) * 120),
			edited.begin() + static_cast<std::ptrdiff_t>(r * W));
		CHECK(same(up.to_channel().get_decompressed(), edited));
	}
	// images
	const std::vector<float> g = pixels(W, H, 5);
	image<float> img(std::vector<std::span<const float>>{ std::span<const float>(f), std::span<const float>(g) }, W, H, { "a", "b" }, enums::codec::lz4, 9, BLOCK, CHUNK, m);
	CHECK(img.mantissa_bits() == std::optional<int>(m));
	CHECK(same(img.channel(1).get_decompressed(), trunc(g, m)));
	img.add_channel(std::span<const float>(g), W, H, "c", enums::codec::lz4, 5, 7);
	CHECK(img.channel(2).mantissa_bits() == std::optional<int>(7) && same(img.channel(2).get_decompressed(), trunc(g, 7)));
	dev_array<float> df(f), dg(g);
	device_image<float> di(std::vector<const float*>{ df.p, dg.p }, W, H, { "a", "b" }, enums::codec::lz4, 9, BLOCK, CHUNK, m);
	CHECK(di.mantissa_bits() == std::optional<int>(m));
	image<float> down = di.to_image();
	CHECK(down.mantissa_bits() == std::optional<int>(m) && same(down.channel(0).get_decompressed(), want) && same(down.channel(1).get_decompressed(), trunc(g, m)));
	device_image<float> back = device_image<float>::from_image(down);
	CHECK(back.mantissa_bits() == std::optional<int>(m));
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "checks";
	try
	{
		checks();
		if (mode == "all") round_trips();
	}
	catch (const std::exception& e)
	{
		std::printf("FAILED: unexpected exception: %s\n", e.what());
		++g_failures;
	}
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
