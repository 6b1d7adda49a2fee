// tests/cpp/masked_region_writes_test.cpp -- fill_region / fill_regions and the masked set_region / set_regions of
// compressed::channel<T>, image<T>, device_channel<T> and device_image<T>, over cimg_update_windows_masked_host / _device.  An image's
// channels share ONE mask and take one value a channel or one for all; lazy (full) chunks a region meets become real.  After every write the whole plane is decoded and compared
// bit for bit with plain loops over a copy of the pixels: an element is written where there is no mask or its mask byte is not 0.
// tests/test_host_mirror_masked_writes.py builds it against the emulator-backed mock of the C ABI
// (tests/emu/mock_window_write_masked.cpp) and against the library on the GPU.
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

template <typename T> static std::vector<T> pixels(unsigned seed, size_t n = W * H)
{
	std::vector<T> v(n);
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

static std::vector<uint8_t> mask_bytes(size_t n, unsigned seed)
{
	std::vector<uint8_t> m(n);
	uint32_t s = seed * 747796405u + 1;
	for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; m[i] = (s >> 28) & 1 ? static_cast<uint8_t>((s >> 16) | 1) : 0; }
	return m;
}

// overlapping crops over chunk boundaries (the later wins), subsampled ones, whole rows, 1 x 1 regions, empty ones
static std::vector<region> cases()
{
	std::vector<region> r;
	for (size_t k = 0; k < 4; ++k) r.push_back({ 128 * k, 10, 128, 40 });
	r.push_back({ 200, 25, 100, 11 }); r.push_back({ 210, 28, 100, 11, 2, 1 }); r.push_back({ 412, 119, 100, 11 });
	r.push_back({ 5, 58, 300, 29, 3, 1 }); r.push_back({ 17, 4, 71, 60, 3, 5 }); r.push_back({ 0, 70, W, 40 });
	r.push_back({ 0, 0, 1, 1 }); r.push_back({ W - 1, H - 1, 1, 1 }); r.push_back({ 77, 90, 1, 1, 4, 4 });
	r.push_back({ 10, 10, 0, 5 }); r.push_back({ 10, 10, 5, 0, 2, 2 });
	return r;
}
static size_t elems(const std::vector<region>& regions) { size_t n = 0; for (const region& r : regions) n += r.out_elems(); return n; }

// the regions written into `plane`: src null -> values (one, or one per region); mask null -> everywhere
template <typename T>
static void apply(std::vector<T>& plane, const std::vector<region>& regions, const T* src, const std::vector<T>& values, const uint8_t* mask)
{
	size_t at = 0;
	for (size_t k = 0; k < regions.size(); ++k)
	{
		const region& r = regions[k];
		const size_t ow = r.out_width();
		for (size_t e = 0; e < r.out_elems(); ++e)
		{
			if (mask && !mask[at + e]) continue;
			const size_t px = r.x + (e % ow) * r.step_x, py = r.y + (e / ow) * r.step_y;
			plane[py * W + px] = src ? src[at + e] : values[values.size() == 1 ? 0 : k];
		}
		at += r.out_elems();
	}
}

template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0; }

template <typename T> static void run(enums::codec codec)
{
	const size_t CHUNK = W * sizeof(T) * 30;
	std::vector<T> plane = pixels<T>(3);
	dev_array<T> d0(plane), back(W * H);
	device_channel<T> dch(d0.p, W, H, codec, 9, BLOCK, CHUNK);
	const std::vector<region> regions = cases();
	const size_t n = elems(regions);
	const std::vector<uint8_t> mask = mask_bytes(n, 5);
	dev_array<uint8_t> dmask(mask);
	const std::vector<T> src = pixels<T>(9, n);
	dev_array<T> dsrc(src);
	std::vector<T> values;
	for (size_t k = 0; k < regions.size(); ++k) values.push_back(static_cast<T>(static_cast<float>(40 + k)));

	// one region, a fill and a masked fill, with steps
	dch.fill_region(static_cast<T>(7.0f), 17, 4, 71, 60, 3, 5);
	apply(plane, { region{ 17, 4, 71, 60, 3, 5 } }, static_cast<const T*>(nullptr), { static_cast<T>(7.0f) }, nullptr);
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane));
	// every region: one value each; one value for all through the mask; arrays through the mask
	dch.fill_regions(regions, values);
	apply(plane, regions, static_cast<const T*>(nullptr), values, nullptr);
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane));
	const std::vector<T> one{ static_cast<T>(99.0f) };
	dch.fill_regions(regions, one, dmask.p);
	apply(plane, regions, static_cast<const T*>(nullptr), one, mask.data());
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane));
	dch.set_regions(regions, dsrc.p, dmask.p);
	apply(plane, regions, src.data(), {}, mask.data());
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane));
	dch.set_region(dsrc.p, 300, 95, 200, 30, 1, 1, dmask.p);
	apply(plane, { region{ 300, 95, 200, 30 } }, src.data(), {}, mask.data());
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane));
	// the size is that of a channel made from the edited pixels
	dev_array<T> dfresh(plane);
	device_channel<T> fresh(dfresh.p, W, H, codec, 9, BLOCK, CHUNK);
	if (codec != enums::codec::zstd) CHECK(dch.compressed_bytes() == fresh.compressed_bytes());
	// refused calls leave the object as it was
	const size_t before = dch.compressed_bytes();
	CHECK_THROWS(std::out_of_range, dch.fill_region(static_cast<T>(1.0f), W - 3, 0, 4, 4));
	CHECK_THROWS(std::invalid_argument, dch.fill_region(static_cast<T>(1.0f), 0, 0, 4, 4, 0, 1));
	CHECK_THROWS(std::invalid_argument, dch.fill_regions(regions, std::vector<T>{ values[0], values[1] }));
	CHECK_THROWS(std::invalid_argument, dch.set_regions(regions, dsrc.p, static_cast<const uint8_t*>(nullptr)));
	CHECK_THROWS(std::out_of_range, dch.set_region(dsrc.p, 0, H - 2, 4, 4, 1, 1, dmask.p));
	dch.fill_regions(std::vector<region>{}, one);
	dch.decompress_into(back.p);
	CHECK(same(back.host(), plane) && dch.compressed_bytes() == before);
	// a blank channel: the chunks a fill meets become real
	device_channel<T> blank = device_channel<T>::full(static_cast<T>(5.0f), W, H, codec, 9, BLOCK, CHUNK);
	std::vector<T> bp(W * H, static_cast<T>(5.0f));
	blank.fill_region(static_cast<T>(9.0f), 10, 20, 100, 50, 3, 1);
	apply(bp, { region{ 10, 20, 100, 50, 3, 1 } }, static_cast<const T*>(nullptr), { static_cast<T>(9.0f) }, nullptr);
	blank.decompress_into(back.p);
	CHECK(same(back.host(), bp));
}

// an image's regions written into its planes: data region-major, channel-minor; ONE mask, region-major; values one a channel or one
template <typename T>
static void apply_image(std::vector<std::vector<T>>& planes, const std::vector<region>& regions, const T* src, const std::vector<T>& values, const uint8_t* mask)
{
	const size_t C = planes.size();
	size_t at = 0, mat = 0;
	for (const region& r : regions)
	{
		const size_t n = r.out_elems(), ow = r.out_width();
		for (size_t c = 0; c < C; ++c)
		{
			for (size_t e = 0; e < n; ++e)
			{
				if (mask && !mask[mat + e]) continue;
				const size_t px = r.x + (e % ow) * r.step_x, py = r.y + (e / ow) * r.step_y;
				planes[c][py * W + px] = src ? src[at + e] : values[values.size() == 1 ? 0 : c];
			}
			at += n;
		}
		mat += n;
	}
}

template <typename T> static void run_host_and_images(enums::codec codec)
{
	const size_t CHUNK = W * sizeof(T) * 30;
	const std::vector<region> regions = cases();
	const size_t n = elems(regions);
	const std::vector<uint8_t> mask = mask_bytes(n, 5);
	const std::vector<T> src = pixels<T>(9, 3 * n);
	const std::vector<T> one{ static_cast<T>(99.0f) }, three{ static_cast<T>(11.0f), static_cast<T>(12.0f), static_cast<T>(13.0f) };
	std::vector<T> values;
	for (size_t k = 0; k < regions.size(); ++k) values.push_back(static_cast<T>(static_cast<float>(40 + k)));
	// ---- channel (host), a real one and a lazy one ----
	for (int lazy = 0; lazy < 2; ++lazy)
	{
		std::vector<T> plane = lazy ? std::vector<T>(W * H, static_cast<T>(5.0f)) : pixels<T>(3);
		channel<T> ch = lazy ? channel<T>::full(W, H, static_cast<T>(5.0f), codec, 9, BLOCK, CHUNK) : channel<T>(std::span<const T>(plane), W, H, codec, 9, BLOCK, CHUNK);
		ch.fill_region(static_cast<T>(7.0f), 17, 4, 71, 60, 3, 5);
		apply(plane, { region{ 17, 4, 71, 60, 3, 5 } }, static_cast<const T*>(nullptr), { static_cast<T>(7.0f) }, nullptr);
		ch.fill_regions(regions, values);
		apply(plane, regions, static_cast<const T*>(nullptr), values, nullptr);
		CHECK(same(ch.get_decompressed(), plane));
		ch.fill_regions(regions, one, std::span<const uint8_t>(mask));
		apply(plane, regions, static_cast<const T*>(nullptr), one, mask.data());
		ch.set_regions(regions, std::span<const T>(src).first(n), std::span<const uint8_t>(mask));
		apply(plane, regions, src.data(), {}, mask.data());
		ch.set_region(std::span<const T>(src).first(6000), 300, 95, 200, 30, 1, 1, std::span<const uint8_t>(mask).first(6000));
		apply(plane, { region{ 300, 95, 200, 30 } }, src.data(), {}, mask.data());
		CHECK(same(ch.get_decompressed(), plane));
		if (codec != enums::codec::zstd && !lazy)
		{
			channel<T> fresh(std::span<const T>(plane), W, H, codec, 9, BLOCK, CHUNK);
			CHECK(ch.compressed_bytes() == fresh.compressed_bytes());
		}
		const size_t before = ch.compressed_bytes();
		CHECK_THROWS(std::out_of_range, ch.fill_region(static_cast<T>(1.0f), W - 3, 0, 4, 4));
		CHECK_THROWS(std::invalid_argument, ch.fill_regions(regions, std::vector<T>{ values[0], values[1] }));
		CHECK_THROWS(std::invalid_argument, ch.set_regions(regions, std::span<const T>(src).first(n), std::span<const uint8_t>(mask).first(n - 1)));
		CHECK_THROWS(std::invalid_argument, ch.fill_regions(regions, one, std::span<const uint8_t>(mask).first(n - 1)));
		CHECK(same(ch.get_decompressed(), plane) && ch.compressed_bytes() == before);
	}
	// ---- image (host) and device_image: one mask for the three channels ----
	std::vector<std::vector<T>> planes{ pixels<T>(1), pixels<T>(2), pixels<T>(3) };
	{
		std::vector<std::vector<T>> want = planes;
		image<T> img(planes, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
		img.fill_region(std::span<const T>(one), 17, 4, 71, 60, 3, 5);
		apply_image(want, { region{ 17, 4, 71, 60, 3, 5 } }, static_cast<const T*>(nullptr), one, nullptr);
		img.fill_regions(regions, std::span<const T>(three), std::span<const uint8_t>(mask));
		apply_image(want, regions, static_cast<const T*>(nullptr), three, mask.data());
		img.set_regions(regions, std::span<const T>(src), std::span<const uint8_t>(mask));
		apply_image(want, regions, src.data(), {}, mask.data());
		img.set_region(std::span<const T>(src).first(3 * 6000), 300, 95, 200, 30, 1, 1, std::span<const uint8_t>(mask).first(6000));
		apply_image(want, { region{ 300, 95, 200, 30 } }, src.data(), {}, mask.data());
		auto dec = img.get_decompressed();
		for (size_t c = 0; c < 3; ++c) CHECK(same(dec[c], want[c]));
		CHECK_THROWS(std::invalid_argument, img.fill_regions(regions, std::vector<T>{ values[0], values[1] }));
		CHECK_THROWS(std::invalid_argument, img.set_regions(regions, std::span<const T>(src), std::span<const uint8_t>(mask).first(n - 1)));
		CHECK_THROWS(std::out_of_range, img.fill_region(std::span<const T>(one), W - 3, 0, 4, 4));
		dec = img.get_decompressed();
		for (size_t c = 0; c < 3; ++c) CHECK(same(dec[c], want[c]));
	}
	{
		std::vector<std::vector<T>> want = planes;
		dev_array<T> d0(planes[0]), d1(planes[1]), d2(planes[2]), dsrc(src), back(W * H);
		dev_array<uint8_t> dmask(mask);
		std::vector<const T*> ptrs{ d0.p, d1.p, d2.p };
		device_image<T> dimg(ptrs, W, H, { "r", "g", "b" }, codec, 9, BLOCK, CHUNK);
		dimg.fill_region(std::span<const T>(three), 17, 4, 71, 60, 3, 5);
		apply_image(want, { region{ 17, 4, 71, 60, 3, 5 } }, static_cast<const T*>(nullptr), three, nullptr);
		dimg.fill_regions(regions, std::span<const T>(one), dmask.p);
		apply_image(want, regions, static_cast<const T*>(nullptr), one, mask.data());
		dimg.set_regions(regions, dsrc.p, dmask.p);
		apply_image(want, regions, src.data(), {}, mask.data());
		dimg.set_region(dsrc.p, 300, 95, 200, 30, 1, 1, dmask.p);
		apply_image(want, { region{ 300, 95, 200, 30 } }, src.data(), {}, mask.data());
		for (size_t c = 0; c < 3; ++c) { dimg.channel(c).decompress_into(back.p); CHECK(same(back.host(), want[c])); }
		CHECK_THROWS(std::invalid_argument, dimg.fill_regions(regions, std::vector<T>{ values[0], values[1] }));
		CHECK_THROWS(std::invalid_argument, dimg.set_regions(regions, dsrc.p, static_cast<const uint8_t*>(nullptr)));
		CHECK_THROWS(std::out_of_range, dimg.fill_region(std::span<const T>(one), W - 3, 0, 4, 4));
		for (size_t c = 0; c < 3; ++c) { dimg.channel(c).decompress_into(back.p); CHECK(same(back.host(), want[c])); }
	}
}

int main()
{
	run_host_and_images<uint8_t>(enums::codec::lz4);
	run_host_and_images<uint16_t>(enums::codec::zstd);
	run_host_and_images<float>(enums::codec::blosclz);
	run_host_and_images<half>(enums::codec::lz4);
	run<uint8_t>(enums::codec::lz4);
	run<uint8_t>(enums::codec::blosclz);
	run<uint16_t>(enums::codec::zstd);
	run<int16_t>(enums::codec::lz4);
	run<half>(enums::codec::lz4);
	run<float>(enums::codec::lz4);
	run<double>(enums::codec::lz4);
	std::printf("\n%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
