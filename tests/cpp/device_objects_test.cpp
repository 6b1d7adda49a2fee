// tests/cpp/device_objects_test.cpp -- compressed::device_channel<T> / device_image<T> (compressed/device_channel.h, device_image.h)
// against the host classes and plain loops.  Device memory comes from cimg_device_malloc and is filled / read with cimg_memcpy_*, so the
// same source runs on the emulator-backed mock of the C ABI (where device memory is host memory) and on the GPU
// (tests/test_host_mirror_device.py builds both).
#include <compressed/device_image.h>

#include <cstdio>
#include <numeric>
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
template <typename T> std::vector<T> crop(const std::vector<T>& v, size_t w, size_t x, size_t y, size_t cw, size_t ch)
{
	std::vector<T> out(cw * ch);
	for (size_t r = 0; r < ch; ++r) for (size_t c = 0; c < cw; ++c) out[r * cw + c] = v[(y + r) * w + x + c];
	return out;
}

template <typename T> void channel_cases(enums::codec codec)
{
	const size_t W = 300, H = 90, chunk = W * sizeof(T) * 13, block = 4096;
	auto px = pixels<T>(W, H, 3);
	dev_array<T> d_px(px);
	device_channel<T> dc(d_px.p, W, H, codec, 9, block, chunk);
	channel<T> hc(std::span<const T>(px), W, H, codec, 9, block, chunk);
	CHECK(dc.num_chunks() == hc.num_chunks() && dc.chunk_size() == hc.chunk_size() && dc.chunk_elems() == hc.chunk_elems());
	CHECK(dc.block_size() == hc.block_size() && dc.width() == W && dc.height() == H && dc.uncompressed_size() == W * H);
	CHECK(dc.compression() == codec && dc.compression_level() == 9);
	CHECK(dc.compressed_bytes() == hc.compressed_bytes());
	CHECK(dc.chunk_size(dc.num_chunks() - 1) == hc.chunk_size(hc.num_chunks() - 1));
	CHECK(dc.device_bytes() >= dc.compressed_bytes() && dc.device_bytes() < dc.compressed_bytes() + 64 * dc.num_chunks());
	CHECK(dc.device_bytes() % 64 == 0 && dc.device_bytes() < W * H * sizeof(T));
	{
		dev_array<T> out(W * H);
		dc.decompress_into(out.p);
		CHECK(out.host() == px);
	}
	const size_t regions[][4] = { {0, 0, W, H}, {0, 0, 1, 1}, {W - 1, H - 1, 1, 1}, {17, 5, 100, 40}, {0, 12, W, 2}, {299, 0, 1, H}, {5, 13, 0, 3}, {40, 25, 33, 28} };
	for (const auto& r : regions)
	{
		dev_array<T> out(r[2] * r[3] + 1);
		dc.get_region(out.p, r[0], r[1], r[2], r[3]);
		auto got = out.host(); got.pop_back();
		CHECK(got == crop(px, W, r[0], r[1], r[2], r[3]));
	}
	dev_array<T> scratch(4);
	CHECK_THROWS(std::out_of_range, dc.get_region(scratch.p, W, 0, 1, 1));
	CHECK_THROWS(std::out_of_range, dc.get_region(scratch.p, 0, 0, W + 1, 1));
	CHECK_THROWS(std::out_of_range, dc.set_region(scratch.p, 10, H - 1, 2, 2));
	CHECK_THROWS(std::invalid_argument, dc.decompress_into(nullptr));
	// set_region: the result is what compressing the edited pixels from scratch gives
	{
		const size_t x = 33, y = 7, w = 120, h = 41;
		auto patch = pixels<T>(w, h, 9);
		dev_array<T> d_patch(patch);
		dc.set_region(d_patch.p, x, y, w, h);
		auto edited = px;
		for (size_t r = 0; r < h; ++r) for (size_t c = 0; c < w; ++c) edited[(y + r) * W + x + c] = patch[r * w + c];
		dev_array<T> out(W * H);
		dc.decompress_into(out.p);
		CHECK(out.host() == edited);
		channel<T> want(std::span<const T>(edited), W, H, codec, 9, block, chunk);
		CHECK(dc.compressed_bytes() == want.compressed_bytes());
		channel<T> back = dc.to_channel();
		CHECK(back.get_decompressed() == edited && back.compressed_bytes() == want.compressed_bytes() && back.num_chunks() == want.num_chunks());
		px = edited;
	}
	// host -> device -> host keeps the chunks
	{
		device_channel<T> up = device_channel<T>::from_channel(hc);
		CHECK(up.compressed_bytes() == hc.compressed_bytes() && up.num_chunks() == hc.num_chunks());
		channel<T> down = up.to_channel();
		CHECK(down.compressed_bytes() == hc.compressed_bytes() && down.get_decompressed() == hc.get_decompressed());
		auto lazy = channel<T>::full(W, H, static_cast<T>(7), codec, 9, block, chunk);
		device_channel<T> filled = device_channel<T>::from_channel(lazy);
		dev_array<T> out(W * H);
		filled.decompress_into(out.p);
		CHECK(out.host() == std::vector<T>(W * H, static_cast<T>(7)));
	}
	// move-only: the moved-to object owns the store, the moved-from one says so when used
	{
		const size_t bytes = dc.device_bytes();
		device_channel<T> moved(std::move(dc));
		CHECK(moved.device_bytes() == bytes);
		dev_array<T> out(W * H);
		moved.decompress_into(out.p);
		CHECK(out.host() == px);
		CHECK_THROWS(std::runtime_error, dc.decompress_into(out.p));
		dc = std::move(moved);
		dc.decompress_into(out.p);
		CHECK(out.host() == px);
		static_assert(!std::is_copy_constructible_v<device_channel<T>> && !std::is_copy_assignable_v<device_channel<T>>);
		static_assert(!std::is_copy_constructible_v<device_image<T>>);
	}
}

template <typename T> void image_cases(enums::codec codec)
{
	const size_t W = 300, H = 90, C = 3, chunk = W * sizeof(T) * 13, block = 4096;
	std::vector<std::vector<T>> planes;
	std::vector<T> all;
	for (size_t c = 0; c < C; ++c) { planes.push_back(pixels<T>(W, H, 20 + static_cast<unsigned>(c))); all.insert(all.end(), planes[c].begin(), planes[c].end()); }
	dev_array<T> d_all(all);
	std::vector<const T*> ptrs;
	for (size_t c = 0; c < C; ++c) ptrs.push_back(d_all.p + c * W * H);
	device_image<T> di(ptrs, W, H, { "R", "G", "B" }, codec, 9, block, chunk);
	image<T> hi(planes, W, H, { "R", "G", "B" }, codec, 9, block, chunk);
	CHECK(di.num_channels() == C && di.width() == W && di.height() == H && di.chunk_size() == hi.chunk_size() && di.block_size() == hi.block_size());
	CHECK(di.channelnames() == hi.channelnames() && di.get_channel_offset("G") == 1);
	CHECK_THROWS(std::invalid_argument, di.get_channel_offset("Z"));
	CHECK_THROWS(std::out_of_range, di.channel(C));
	CHECK_THROWS(std::invalid_argument, di.channelnames({ "only" }));
	size_t host_cbytes = 0;
	for (const auto& c : hi.channels()) host_cbytes += c.compressed_bytes();
	CHECK(di.compressed_bytes() == host_cbytes && di.num_chunks() == C * hi.channel(0).num_chunks());
	CHECK(di.device_bytes() < di.uncompressed_size() * sizeof(T));
	{
		dev_array<T> out(C * W * H);
		di.decompress_into(out.p);
		CHECK(out.host() == all);
	}
	// a channel handle shares the store and is read-only
	{
		device_channel<T> g = di.channel("G");
		CHECK(g.read_only() && g.device_bytes() == di.device_bytes() && g.compressed_bytes() == hi.channel(1).compressed_bytes());
		dev_array<T> out(W * H);
		g.decompress_into(out.p);
		CHECK(out.host() == planes[1]);
		dev_array<T> reg(50 * 20);
		g.get_region(reg.p, 100, 30, 50, 20);
		CHECK(reg.host() == crop(planes[1], W, 100, 30, 50, 20));
		CHECK_THROWS(std::runtime_error, g.set_region(reg.p, 0, 0, 50, 20));
		CHECK(g.to_channel().get_decompressed() == planes[1]);
	}
	const size_t regions[][4] = { {0, 0, W, H}, {17, 5, 100, 40}, {W - 1, H - 1, 1, 1}, {3, 12, 5, 2}, {40, 25, 33, 28} };
	for (const auto& r : regions)
	{
		const size_t n = r[2] * r[3];
		dev_array<T> planar(C * n), il(C * n);
		di.get_region(planar.p, r[0], r[1], r[2], r[3]);
		di.get_region(il.p, r[0], r[1], r[2], r[3], true);
		auto p = planar.host(), q = il.host();
		bool ok = true;
		for (size_t c = 0; c < C; ++c)
		{
			auto want = crop(planes[c], W, r[0], r[1], r[2], r[3]);
			for (size_t i = 0; i < n; ++i) ok = ok && p[c * n + i] == want[i] && q[i * C + c] == want[i];
		}
		CHECK(ok);
	}
	// set_region over all channels, then the handle taken BEFORE still decodes the old pixels (it keeps its store)
	{
		device_channel<T> before = di.channel(0);
		const size_t x = 10, y = 20, w = 200, h = 30;
		std::vector<T> patch;
		for (size_t c = 0; c < C; ++c) { auto p = pixels<T>(w, h, 40 + static_cast<unsigned>(c)); patch.insert(patch.end(), p.begin(), p.end()); }
		dev_array<T> d_patch(patch);
		di.set_region(d_patch.p, x, y, w, h);
		auto edited = planes;
		for (size_t c = 0; c < C; ++c) for (size_t r = 0; r < h; ++r) for (size_t k = 0; k < w; ++k) edited[c][(y + r) * W + x + k] = patch[c * w * h + r * w + k];
		dev_array<T> out(C * W * H);
		di.decompress_into(out.p);
		auto got = out.host();
		for (size_t c = 0; c < C; ++c) CHECK(std::vector<T>(got.begin() + c * W * H, got.begin() + (c + 1) * W * H) == edited[c]);
		image<T> want(edited, W, H, {}, codec, 9, block, chunk);
		size_t want_c = 0;
		for (const auto& c : want.channels()) want_c += c.compressed_bytes();
		CHECK(di.compressed_bytes() == want_c);
		dev_array<T> old(W * H);
		before.decompress_into(old.p);
		CHECK(old.host() == planes[0]);
		image<T> down = di.to_image();
		CHECK(down.get_decompressed() == edited && down.channelnames() == di.channelnames());
		device_image<T> up = device_image<T>::from_image(down);
		CHECK(up.compressed_bytes() == di.compressed_bytes() && up.device_bytes() == di.device_bytes());
		up.decompress_into(out.p);
		CHECK(out.host() == got);
	}
	// interleaved pixels in device memory
	{
		std::vector<T> il(C * W * H);
		for (size_t i = 0; i < W * H; ++i) for (size_t c = 0; c < C; ++c) il[i * C + c] = planes[c][i];
		dev_array<T> d_il(il);
		auto fi = device_image<T>::from_interleaved(d_il.p, W, H, C, {}, codec, 9, block, chunk);
		CHECK(fi.compressed_bytes() == host_cbytes);
		dev_array<T> out(C * W * H);
		fi.decompress_into(out.p);
		CHECK(out.host() == all);
		fi.get_region(out.p, 0, 0, W, H, true);
		CHECK(out.host() == il);
	}
}

// a _packed_fetch whose staging area another batch call has reused fails with an error code, and the engine stays usable
static void voided_fetch()
{
	cimg_engine* e = blosc2::batch::engine();
	auto px = pixels<uint16_t>(256, 64, 1);
	dev_array<uint16_t> d_px(px), d_store(px.size());
	cimg_cparams cp;
	cimg_cparams_init(&cp, 2);
	const int64_t raw_off[2] = { 0, 16384 }, dst_off[2] = { 0, 16512 };
	const int32_t nbytes[2] = { 16384, 16384 }, destsize[2] = { 16384 + 32, 16384 + 32 };
	int32_t cbytes[2] = { 0, 0 };
	CHECK(cimg_compress_batch_device_packed_fetch(e, 2, d_store.p, dst_off) < 0);
	CHECK(cimg_compress_batch_device_packed_begin(e, &cp, 2, d_px.p, raw_off, nbytes, destsize, cbytes) == 0 && cbytes[0] > 32 && cbytes[1] > 32);
	channel<uint16_t> other(std::span<const uint16_t>(px), 256, 64);            // an intervening batch on the same engine
	CHECK(cimg_compress_batch_device_packed_fetch(e, 2, d_store.p, dst_off) < 0);
	CHECK(cimg_compress_batch_device_packed_begin(e, &cp, 2, d_px.p, raw_off, nbytes, destsize, cbytes) == 0);
	CHECK(cimg_compress_batch_device_packed_fetch(e, 2, d_store.p, dst_off) == 0);
	CHECK(cimg_compress_batch_device_packed_fetch(e, 2, d_store.p, dst_off) < 0);
	CHECK(other.get_decompressed() == px);
}

int main()
{
	for (auto codec : { enums::codec::lz4, enums::codec::blosclz })
	{
		channel_cases<uint8_t>(codec);
		channel_cases<uint16_t>(codec);
		channel_cases<float>(codec);
		image_cases<uint16_t>(codec);
	}
	channel_cases<uint16_t>(enums::codec::zstd);
	image_cases<float>(enums::codec::zstd);
	voided_fetch();
	std::printf("%d failures\n", g_failures);
	return g_failures ? 1 : 0;
}
