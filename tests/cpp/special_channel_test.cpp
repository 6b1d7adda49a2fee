// tests/cpp/special_channel_test.cpp -- device_channel<T>::full / zeros / full_like / zeros_like (compressed/device_channel.h): blank
// channels made of blosc2 special-value chunks, and such a channel's chunks inside a device_image<T>.  Device memory comes from
// cimg_device_malloc and is filled / read with cimg_memcpy_*, so the same source runs on the emulator-backed mock of the C ABI and
// on the GPU (tests/test_host_mirror_special.py builds both), like device_objects_test.cpp.
#include <compressed/device_image.h>

#include <cstdio>
#include <utility>

using namespace compressed;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)
#define CHECK_THROWS(T, expr) do { bool caught_ = false; try { expr; } catch (const T&) { caught_ = true; } catch (...) {} \
	if (!caught_) { std::printf("FAILED %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #T); ++g_failures; } } while (0)

template <typename T>
struct dev_array
{
	T* p; size_t n;
	explicit dev_array(size_t n_) : p(static_cast<T*>(cimg_device_malloc(blosc2::batch::engine(), n_ * sizeof(T)))), n(n_) {}
	explicit dev_array(const std::vector<T>& h) : dev_array(h.size()) { cimg_memcpy_h2d(blosc2::batch::engine(), p, h.data(), n * sizeof(T)); }
	~dev_array() { cimg_device_free(blosc2::batch::engine(), p); }
	dev_array(const dev_array&) = delete;
	std::vector<T> host() const { std::vector<T> h(n); cimg_memcpy_d2h(blosc2::batch::engine(), h.data(), p, n * sizeof(T)); return h; }
};

template <typename T> std::vector<T> pixels(size_t w, size_t h, unsigned seed)
{
	std::vector<T> v(w * h);
	for (size_t y = 0; y < h; ++y) for (size_t x = 0; x < w; ++x) v[y * w + x] = static_cast<T>((x / 7 + y / 3) * 5 + ((x * 31 + y * 17 + seed) % 11 == 0 ? seed + x : 0));
	return v;
}
template <typename T> std::vector<T> decoded(const device_channel<T>& c)
{
	dev_array<T> out(c.uncompressed_size());
	c.decompress_into(out.p);
	return out.host();
}

template <typename T> void cases(enums::codec codec, T value)
{
	const size_t W = 300, H = 90, chunk = W * sizeof(T) * 13, block = 4096;
	auto dc = device_channel<T>::full(value, W, H, codec, 9, block, chunk);
	CHECK(dc.width() == W && dc.height() == H && dc.num_chunks() == 7 && dc.block_size() == block && dc.chunk_size() == chunk);
	CHECK(dc.compression() == codec && dc.compression_level() == 9 && !dc.read_only());
	CHECK(dc.device_bytes() == 64 * dc.num_chunks());
	for (size_t i = 0; i < dc.num_chunks(); ++i) CHECK(dc.compressed_bytes(i) == 32 + sizeof(T));
	std::vector<T> want(W * H, value);
	CHECK(decoded(dc) == want);
	{
		dev_array<T> out(71 * 60);
		dc.get_region(out.p, 17, 4, 71, 60);
		CHECK(out.host() == std::vector<T>(71 * 60, value));
		dev_array<T> sub(24 * 12);
		dc.get_region(sub.p, 17, 4, 71, 60, 3, 5);
		CHECK(sub.host() == std::vector<T>(24 * 12, value));
		const std::vector<region> rs = { {0, 0, 50, 13, 1, 1}, {250, 77, 50, 13, 2, 3} };
		dev_array<T> many(50 * 13 + 25 * 5);
		dc.get_regions(many.p, rs);
		CHECK(many.host() == std::vector<T>(50 * 13 + 25 * 5, value));
	}
	// zeros, and a fill of zero bytes: special-zero chunks
	auto dz = device_channel<T>::zeros(W, H, codec, 9, block, chunk);
	CHECK(dz.device_bytes() == 64 * dz.num_chunks() && dz.compressed_bytes() == 32 * dz.num_chunks());
	CHECK(decoded(dz) == std::vector<T>(W * H, T{}));
	auto like = device_channel<T>::full_like(dz, value);
	CHECK(like.compressed_bytes() == dc.compressed_bytes() && like.chunk_size() == chunk && decoded(like) == want);
	CHECK(decoded(device_channel<T>::zeros_like(dc)) == std::vector<T>(W * H, T{}));
	// set_region: only the chunks it touches become regular (rows 20 .. 32: chunks 1 and 2)
	auto patch = pixels<T>(71, 13, 5);
	dev_array<T> d_patch(patch);
	dc.set_region(d_patch.p, 17, 20, 71, 13);
	for (size_t r = 0; r < 13; ++r) for (size_t c = 0; c < 71; ++c) want[(20 + r) * W + 17 + c] = patch[r * 71 + c];
	for (size_t i = 0; i < dc.num_chunks(); ++i) CHECK((dc.compressed_bytes(i) == 32 + sizeof(T)) == (i != 1 && i != 2));
	CHECK(decoded(dc) == want);
	// to_channel hands the special chunks over as they are; the host classes read them through the batch calls
	channel<T> hc = dc.to_channel();
	CHECK(hc.num_chunks() == dc.num_chunks() && hc.compressed_bytes() == dc.compressed_bytes());
	CHECK(hc.get_decompressed() == want);
	// inside a device_image: the blank channel's chunks beside a channel of pixels, moved as they are
	auto px = pixels<T>(W, H, 9);
	std::vector<channel<T>> chans;
	chans.push_back(channel<T>(std::span<const T>(px), W, H, codec, 9, block, chunk));
	chans.push_back(device_channel<T>::full(value, W, H, codec, 9, block, chunk).to_channel());
	image<T> himg(std::move(chans), W, H, { "r", "blank" });
	auto dimg = device_image<T>::from_image(himg);
	CHECK(decoded(dimg.channel("blank")) == std::vector<T>(W * H, value));
	CHECK(decoded(dimg.channel("r")) == px);
	CHECK(dimg.channel("blank").compressed_bytes() == (32 + sizeof(T)) * 7);
	CHECK_THROWS(std::invalid_argument, device_channel<T>::full(value, 0, 4));
}

int main()
{
	for (enums::codec codec : { enums::codec::lz4, enums::codec::blosclz })
	{
		cases<uint8_t>(codec, 7);
		cases<uint16_t>(codec, 0x1234);
		cases<float>(codec, -2.75f);
		cases<double>(codec, 3.0e-7);
	}
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
