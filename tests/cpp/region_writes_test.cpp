// tests/cpp/region_writes_test.cpp -- strided and batched region writes of compressed::channel<T> / image<T> / device_channel<T> /
// device_image<T>: set_region(..., step_x, step_y) and set_regions(regions, data) over cimg_update_windows_strided_host / _device, lazy
// `full` channels included.  After every write the object
// must decode to the pixels edited by plain loops (later regions win), set_region(get_region(r), r) must change nothing, its chunks
// must have the sizes of an object built from the edited pixels, every region is checked before anything runs, an empty list does
// nothing and a refused call leaves the object as it was.  tests/test_host_mirror_region_writes.py builds it against the
// emulator-backed mock of the C ABI (tests/emu/mock_window_write_strided.cpp) and against the library on the GPU.
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
	explicit dev_array(size_t count) : p(static_cast<T*>(cimg_device_malloc(blosc2::batch::engine(), count * sizeof(T) + 1))), n(count) {}
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
		v[i] = static_cast<T>(((i % W) / 7) * 3 + ((i / W) / 5) * 11 + (s >> 30) + seed);
	}
	return v;
}

// a row of tiles, crops over chunk boundaries (one lying on an earlier one: it wins), subsampled ones, 1 x 1 regions, empty ones
static std::vector<region> cases()
{
	std::vector<region> r;
	for (size_t k = 0; k < 4; ++k) r.push_back({ 128 * k, 10, 128, 40 });
	r.push_back({ 200, 25, 100, 11 }); r.push_back({ 210, 28, 100, 11, 2, 1 }); r.push_back({ 412, 119, 100, 11 });
	r.push_back({ 0, 0, W, H, 7, 9 }); r.push_back({ 5, 58, 300, 29, 3, 1 }); r.push_back({ 17, 4, 71, 60, 3, 5 });
	r.push_back({ 0, 0, 1, 1 }); r.push_back({ W - 1, H - 1, 1, 1 }); r.push_back({ 77, 90, 1, 1, 4, 4 }); r.push_back({ 0, 0, 1, 1 });
	r.push_back({ 10, 10, 0, 5 }); r.push_back({ 10, 10, 5, 0, 2, 2 });
	return r;
}
static size_t elems(const std::vector<region>& regions) { size_t n = 0; for (const region& r : regions) n += r.out_elems(); return n; }

// the regions written into planes, one after the other: data region-major, channel-minor, each row-major in its subsampled shape
template <typename T> static void apply(std::vector<std::vector<T>>& planes, const std::vector<region>& regions, const std::vector<T>& data)
{
	size_t at = 0;
	for (const region& r : regions)
		for (auto& p : planes)
			for (size_t y = r.y; y < r.y + r.height; y += r.step_y)
				for (size_t x = r.x; x < r.x + r.width; x += r.step_x) p[y * W + x] = data[at++];
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
// chunk for chunk the same compressed bytes (the header's cbytes at offset 12 says how many)
template <typename A, typename B> static bool same_chunks(A&& a, B&& b)             // (channels; to_schunk is not const)
{
	auto ra = std::visit([](auto& s) { return s.to_schunk(); }, a.chunks());
	auto rb = std::visit([](auto& s) { return s.to_schunk(); }, b.chunks());
	if (ra->nchunks != rb->nchunks || ra->nchunks == 0) return false;
	auto csize = [](const uint8_t* c) { return static_cast<size_t>(c[12]) | (static_cast<size_t>(c[13]) << 8) | (static_cast<size_t>(c[14]) << 16) | (static_cast<size_t>(c[15]) << 24); };
	for (int64_t k = 0; k < ra->nchunks; ++k)
		if (csize(ra->data[k]) != csize(rb->data[k]) || !std::equal(ra->data[k], ra->data[k] + csize(ra->data[k]), rb->data[k])) return false;
	return true;
}
template <typename T> static std::vector<T> decoded(const device_channel<T>& c)
{
	dev_array<T> out(W * H);
	c.decompress_into(out.p);
	return out.host();
}

template <typename T> static void run(enums::codec codec)
{
	const size_t CHUNK = W * sizeof(T) * 30;                         // four chunks of 30 rows and a leftover chunk of 10
	std::vector<std::vector<T>> planes{ pixels<T>(1), pixels<T>(2), pixels<T>(3) };
	const std::vector<region> regions = cases();
	const std::vector<region> none;
	const std::vector<region> bad{ { 0, 0, 4, 4 }, { W - 3, 0, 4, 4 } }, bad_step{ { 0, 0, 4, 4 }, { 0, 0, 4, 4, 0, 1 } };

	// ---- device_channel ----
	{
		std::vector<std::vector<T>> want{ planes[0] };
		dev_array<T> d0(planes[0]);
		device_channel<T> dch(d0.p, W, H, codec, 9, BLOCK, CHUNK);
		// one strided region
		const region r{ 17, 4, 71, 60, 3, 5 };
		const std::vector<T> v = pixels<T>(9, r.out_elems());
		dev_array<T> dv(v);
		dch.set_region(dv.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		apply<T>(want, { r }, v);
		CHECK(same(decoded(dch), want[0]));
		// set_region(get_region(r), r) changes nothing
		dev_array<T> back(r.out_elems());
		dch.get_region(back.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		CHECK(same(back.host(), v));
		const size_t bytes = dch.compressed_bytes();
		dch.set_region(back.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		CHECK(same(decoded(dch), want[0]) && dch.compressed_bytes() == bytes);
		// many regions, one call
		const std::vector<T> data = pixels<T>(5, elems(regions));
		dev_array<T> dd(data);
		dch.set_regions(regions, dd.p);
		apply<T>(want, regions, data);
		CHECK(same(decoded(dch), want[0]));
		if (codec != enums::codec::zstd)
		{
			dev_array<T> de(want[0]);
			device_channel<T> fresh(de.p, W, H, codec, 9, BLOCK, CHUNK);
			CHECK(fresh.compressed_bytes() == dch.compressed_bytes());
			CHECK(same_chunks(dch.to_channel(), fresh.to_channel()));            // byte for byte the edited pixels compressed from scratch
		}
		// nothing runs unless every region is good; an empty list does nothing
		const size_t before = dch.compressed_bytes();
		CHECK_THROWS(std::out_of_range, dch.set_regions(bad, dd.p));
		CHECK_THROWS(std::invalid_argument, dch.set_regions(bad_step, dd.p));
		CHECK_THROWS(std::invalid_argument, dch.set_region(dd.p, 0, 0, 4, 4, 1, 0));
		CHECK_THROWS(std::out_of_range, dch.set_region(dd.p, W - 3, 0, 4, 4, 2, 2));
		dch.set_regions(none, dd.p);
		dch.set_regions(none, nullptr);
		CHECK(same(decoded(dch), want[0]) && dch.compressed_bytes() == before);
	}
	// ---- channel (host) ----
	{
		std::vector<std::vector<T>> want{ planes[0] };
		channel<T> ch(std::span<const T>(planes[0]), W, H, codec, 9, BLOCK, CHUNK);
		const region r{ 17, 4, 71, 60, 3, 5 };
		const std::vector<T> v = pixels<T>(9, r.out_elems());
		ch.set_region(std::span<const T>(v), r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		apply<T>(want, { r }, v);
		CHECK(same(ch.get_decompressed(), want[0]));
		const std::vector<T> back = ch.get_region(r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		CHECK(same(back, v));
		const size_t bytes = ch.compressed_bytes();
		ch.set_region(std::span<const T>(back), r.x, r.y, r.width, r.height, r.step_x, r.step_y);          // set_region(get_region(r), r)
		CHECK(same(ch.get_decompressed(), want[0]) && ch.compressed_bytes() == bytes);
		const std::vector<T> data = pixels<T>(5, elems(regions));
		ch.set_regions(regions, std::span<const T>(data));
		apply<T>(want, regions, data);
		CHECK(same(ch.get_decompressed(), want[0]));
		if (codec != enums::codec::zstd)
		{
			channel<T> fresh(std::span<const T>(want[0]), W, H, codec, 9, BLOCK, CHUNK);
			CHECK(fresh.compressed_bytes() == ch.compressed_bytes());
			CHECK(same_chunks(ch, fresh));                                        // byte for byte the edited pixels compressed from scratch
		}
		// the span must hold exactly the subsampled elements; every region is checked first; nothing changes on a refusal
		const size_t before = ch.compressed_bytes();
		CHECK_THROWS(std::invalid_argument, ch.set_regions(regions, std::span<const T>(data).first(data.size() - 1)));
		CHECK_THROWS(std::invalid_argument, ch.set_region(std::span<const T>(v).first(v.size() - 1), r.x, r.y, r.width, r.height, r.step_x, r.step_y));
		CHECK_THROWS(std::invalid_argument, ch.set_region(std::span<const T>(v), r.x, r.y, r.width, r.height, 1, 1));
		CHECK_THROWS(std::out_of_range, ch.set_regions(bad, std::span<const T>(data).first(32)));
		CHECK_THROWS(std::invalid_argument, ch.set_regions(bad_step, std::span<const T>(data).first(32)));
		CHECK_THROWS(std::invalid_argument, ch.set_region(std::span<const T>(data).first(16), 0, 0, 4, 4, 1, 0));
		ch.set_regions(none, std::span<const T>());
		CHECK(same(ch.get_decompressed(), want[0]) && ch.compressed_bytes() == before);
	}
	// ---- a lazy `full` channel: the chunks a region meets become real, filled and patched with stride, in region order ----
	{
		const T fill = static_cast<T>(7);
		std::vector<std::vector<T>> want{ std::vector<T>(W * H, fill) };
		channel<T> lz = channel<T>::full(W, H, fill, codec, 9, BLOCK, CHUNK);
		const std::vector<region> rs{ { 5, 58, 300, 29, 3, 2 }, { 0, 0, 1, 1 }, { 100, 59, 50, 3, 2, 1 }, { 0, 0, 1, 1 } };   // chunks 0, 1 and 2; overlaps
		const std::vector<T> data = pixels<T>(6, elems(rs));
		lz.set_regions(rs, std::span<const T>(data));
		apply<T>(want, rs, data);
		CHECK(same(lz.get_decompressed(), want[0]));
		const std::vector<T> more = pixels<T>(4, elems(regions));                // real and lazy chunks in one call
		lz.set_regions(regions, std::span<const T>(more));
		apply<T>(want, regions, more);
		CHECK(same(lz.get_decompressed(), want[0]));
		if (codec != enums::codec::zstd)
		{
			channel<T> fresh(std::span<const T>(want[0]), W, H, codec, 9, BLOCK, CHUNK);
			CHECK(fresh.compressed_bytes() == lz.compressed_bytes());            // (every chunk is real by now)
			CHECK(same_chunks(lz, fresh));
		}
	}
	// ---- image (host) ----
	{
		std::vector<std::vector<T>> want = planes;
		image<T> img(planes, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
		const region r{ 3, 7, 400, 100, 4, 3 };
		const std::vector<T> v = pixels<T>(7, 3 * r.out_elems());
		std::vector<std::span<const T>> spans;
		for (size_t c = 0; c < 3; ++c) spans.push_back(std::span<const T>(v).subspan(c * r.out_elems(), r.out_elems()));
		img.set_region(spans, r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		apply<T>(want, { r }, v);
		const std::vector<T> data = pixels<T>(8, 3 * elems(regions));
		img.set_regions(regions, std::span<const T>(data));
		apply<T>(want, regions, data);
		auto dec = img.get_decompressed();
		for (size_t c = 0; c < 3; ++c) CHECK(same(dec[c], want[c]));
		if (codec != enums::codec::zstd)
			for (size_t c = 0; c < 3; ++c)
			{
				channel<T> fresh(std::span<const T>(want[c]), W, H, codec, 9, BLOCK, CHUNK);
				CHECK(same_chunks(img.channel(c), fresh));
			}
		const std::vector<T> got = img.get_regions(regions);                     // what get_regions returns is what set_regions takes
		img.set_regions(regions, std::span<const T>(got));
		dec = img.get_decompressed();
		for (size_t c = 0; c < 3; ++c) CHECK(same(dec[c], want[c]));
		CHECK_THROWS(std::invalid_argument, img.set_regions(regions, std::span<const T>(data).first(data.size() - 1)));
		spans.pop_back();
		CHECK_THROWS(std::invalid_argument, img.set_region(spans, r.x, r.y, r.width, r.height, r.step_x, r.step_y));
		CHECK_THROWS(std::out_of_range, img.set_regions(bad, std::span<const T>(data).first(96)));
		CHECK_THROWS(std::invalid_argument, img.set_regions(bad_step, std::span<const T>(data).first(96)));
		img.set_regions(none, std::span<const T>());
		dec = img.get_decompressed();
		for (size_t c = 0; c < 3; ++c) CHECK(same(dec[c], want[c]));
	}
	// ---- device_image ----
	{
		std::vector<std::vector<T>> want = planes;
		dev_array<T> d0(planes[0]), d1(planes[1]), d2(planes[2]);
		std::vector<const T*> ptrs{ d0.p, d1.p, d2.p };
		device_image<T> dimg(ptrs, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
		const region r{ 3, 7, 400, 100, 4, 3 };
		const std::vector<T> v = pixels<T>(7, 3 * r.out_elems());
		dev_array<T> dv(v);
		dimg.set_region(dv.p, r.x, r.y, r.width, r.height, r.step_x, r.step_y);
		apply<T>(want, { r }, v);
		const std::vector<T> data = pixels<T>(8, 3 * elems(regions));
		dev_array<T> dd(data);
		dimg.set_regions(regions, dd.p);
		apply<T>(want, regions, data);
		for (size_t c = 0; c < 3; ++c) CHECK(same(decoded(dimg.channel(c)), want[c]));
		if (codec != enums::codec::zstd)
			for (size_t c = 0; c < 3; ++c)
			{
				channel<T> fresh(std::span<const T>(want[c]), W, H, codec, 9, BLOCK, CHUNK);
				CHECK(same_chunks(dimg.channel(c).to_channel(), fresh));
			}
		// what get_regions returns is what set_regions takes
		dev_array<T> got(3 * elems(regions));
		dimg.get_regions(got.p, regions);
		dimg.set_regions(regions, got.p);
		for (size_t c = 0; c < 3; ++c) CHECK(same(decoded(dimg.channel(c)), want[c]));
		CHECK_THROWS(std::out_of_range, dimg.set_regions(bad, dd.p));
		CHECK_THROWS(std::invalid_argument, dimg.set_regions(bad_step, dd.p));
		dimg.set_regions(none, dd.p);
		for (size_t c = 0; c < 3; ++c) CHECK(same(decoded(dimg.channel(c)), want[c]));
	}
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
