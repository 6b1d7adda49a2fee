// channel.h -- compressed::channel<T>: one planar image channel stored as blosc2 chunks, with the
// reference's public surface (compressed/channel.h: constructors :97-201, zeros/full factories
// :219-304, iteration :309-327, accessors :353-491, get_chunk :502-516, set_chunk :527-538,
// get_decompressed :545-558).  Compression of the whole channel and get_decompressed are single
// batched calls into the MI355X engine.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <optional>
#include <span>
#include <stdexcept>
#include <thread>
#include <variant>
#include <vector>

#include "blosc2/schunk.h"
#include "constants.h"
#include "enums.h"
#include "iterators/iterator.h"
#include "macros.h"
#include "util.h"

namespace NAMESPACE_COMPRESSED_IMAGE
{
	/// One rectangle of a batched read (get_regions): [x, x + width) x [y, y + height), of which every step_y-th row and every
	/// step_x-th element of those rows are taken -- out_height() rows of out_width() elements.
	struct region
	{
		size_t x = 0, y = 0, width = 0, height = 0, step_x = 1, step_y = 1;
		size_t out_width() const noexcept { return step_x ? (width + step_x - 1) / step_x : 0; }
		size_t out_height() const noexcept { return step_y ? (height + step_y - 1) / step_y : 0; }
		size_t out_elems() const noexcept { return out_width() * out_height(); }
	};

	template <typename T>
	struct channel
	{
		using iterator = channel_iterator<T>;

		channel(channel&&) noexcept = default;
		channel& operator=(channel&&) noexcept = default;
		channel(const channel&) = delete;
		channel& operator=(const channel&) = delete;

		/// A valid-but-empty channel (one lazy element), as the reference's default constructor gives.
		channel()
		{
			m_Schunk = std::make_shared<blosc2::schunk_var<T>>(blosc2::lazy_schunk<T>(T{}, 1, s_default_blocksize, s_default_chunksize));
			make_contexts(s_default_blocksize);
		}

		/// Compress `data` (width * height elements).  Chunks are aligned to whole scanlines.  mantissa_bits (float types only, 1 .. 10 /
		/// 23 / 52): lossy storage -- only that many mantissa bits of every element are kept (blosc2's trunc-prec filter), here and in
		/// everything written later (set_chunk, the iterator's write-back, set_region).
		channel(const std::span<const T> data, size_t width, size_t height,
			enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
			: m_Codec(compression_codec), m_CompressionLevel(util::ensure_compression_level(compression_level)), m_MantissaBits(mantissa_bits), m_Width(width), m_Height(height)
		{
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			if (data.size() != width * height)
				throw std::runtime_error(detail::text("Invalid channel data passed. Expected its size to match up to width * height (", width, " * ", height,
					") which would be ", width * height, ". Instead received ", data.size()));
			make_contexts(block_size);
			const size_t aligned = util::align_chunk_to_scanlines_bytes<T>(m_Width, chunk_size);
			m_Schunk = std::make_shared<blosc2::schunk_var<T>>(blosc2::schunk<T>(data, block_size, aligned, m_CompressionContext));
		}

		/// Adopt an existing chunk table.
		channel(blosc2::schunk_var<T> schunk, size_t width, size_t height,
			enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 9, std::optional<int> mantissa_bits = std::nullopt)
			: m_Codec(compression_codec), m_CompressionLevel(util::ensure_compression_level(compression_level)), m_MantissaBits(mantissa_bits), m_Width(width), m_Height(height)
		{
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			const size_t have = std::visit([](auto& s) { return s.size(); }, schunk);
			if (have != width * height)
				throw std::invalid_argument(detail::text("Invalid schunk passed to compressed::channel constructor. Expected a size of ", width * height, " but instead got ", have));
			m_Schunk = std::make_shared<blosc2::schunk_var<T>>(std::move(schunk));
			m_Adopted = true;
			make_contexts(block_size());
		}

		static channel full(size_t width, size_t height, T fill_value, enums::codec compression_codec = enums::codec::lz4,
			uint8_t compression_level = 9, size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize)
		{
			const size_t aligned = util::align_chunk_to_scanlines_bytes<T>(width, chunk_size);
			return channel(blosc2::schunk_var<T>(blosc2::lazy_schunk<T>(fill_value, width * height, block_size, aligned)), width, height, compression_codec, compression_level);
		}
		static channel zeros(size_t width, size_t height, enums::codec compression_codec = enums::codec::lz4,
			uint8_t compression_level = 9, size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize)
		{
			return full(width, height, T{}, compression_codec, compression_level, block_size, chunk_size);
		}
		static channel full_like(const channel& other, T fill_value)
		{
			return full(other.width(), other.height(), fill_value, other.compression(), other.compression_level(), other.block_size(), other.chunk_size());
		}
		static channel zeros_like(const channel& other) { return full_like(other, T{}); }

		iterator begin() { require_encoder(); return iterator(m_Schunk, m_CompressionContext.get(), m_DecompressionContext.get(), 0, m_Width, m_Height); }
		iterator end() { require_encoder(); return iterator(m_Schunk, m_CompressionContext.get(), m_DecompressionContext.get(), num_chunks(), m_Width, m_Height); }

		blosc2::context_raw_ptr compression_context() { return m_CompressionContext.get(); }
		blosc2::context_raw_ptr decompression_context() { return m_DecompressionContext.get(); }

		/// Rebuilds the contexts (possibly with another block size), as the reference does.  The thread count
		/// itself is meaningless here -- the GPU is the parallelism -- and is only remembered.
		void update_nthreads(size_t nthreads, size_t block_size = s_default_blocksize)
		{
			m_Nthreads = nthreads;
			make_contexts(block_size);
		}

		size_t width() const noexcept { return m_Width; }
		size_t height() const noexcept { return m_Height; }
		enums::codec compression() const noexcept { return m_Codec; }
		uint8_t compression_level() const noexcept { return m_CompressionLevel; }
		/// mantissa bits kept by everything this channel writes (nullopt: lossless)
		std::optional<int> mantissa_bits() const noexcept { return m_MantissaBits; }

		size_t compressed_bytes() const { return visit([](auto& s) { return s.csize(); }); }
		size_t uncompressed_size() const { return visit([](auto& s) { return s.size(); }); }
		size_t num_chunks() const { return visit([](auto& s) { return s.num_chunks(); }); }
		size_t block_size() const { return visit([](auto& s) { return s.max_block_size(); }); }
		size_t chunk_size() const { return visit([](auto& s) { return s.chunk_bytes(); }); }
		size_t chunk_elems() const { return chunk_size() / sizeof(T); }
		size_t chunk_size(size_t chunk_index) const { return visit([&](auto& s) { return s.chunk_bytes(chunk_index); }); }
		size_t chunk_elems(size_t chunk_index) const { return chunk_size(chunk_index) / sizeof(T); }

		void get_chunk(std::span<T> buffer, size_t chunk_idx) const
		{
			visit([&](auto& s) { s.chunk(m_DecompressionContext.get(), buffer, chunk_idx); return 0; });
		}
		void set_chunk(std::span<T> buffer, size_t chunk_idx)
		{
			require();
			require_encoder();
			std::visit([&](auto& s) { s.set_chunk(m_CompressionContext, buffer, chunk_idx); }, *m_Schunk);
		}
		/// Decode into caller-owned memory (uncompressed_size() elements): no intermediate vector, no zero fill.
		void decompress_into(std::span<T> out) const
		{
			require();
			if (out.size() != uncompressed_size())
				throw std::invalid_argument(detail::text("decompress_into: buffer holds ", out.size(), " elements, channel has ", uncompressed_size()));
			std::vector<blosc2::batch::target> work;
			std::visit([&](const auto& table) { table.plan_decode(out.data(), work); }, *m_Schunk);
			blosc2::batch::decompress(work);
		}
		std::vector<T> get_decompressed() const
		{
			require();
			return std::visit([&](const auto& s) { return s.to_uncompressed(const_cast<blosc2::context_ptr&>(m_DecompressionContext)); }, *m_Schunk);
		}

		/// The rectangle [x, x + width) x [y, y + height) of the channel, row-major (width elements a row).  Only the blocks the
		/// rectangle meets are decoded, on the device, and only its pixels come back; lazy chunks fill their part on the host.
		std::vector<T> get_region(size_t x, size_t y, size_t width, size_t height) const
		{
			std::vector<T> out(width * height);
			get_region(std::span<T>(out), x, y, width, height);
			return out;
		}
		void get_region(std::span<T> out, size_t x, size_t y, size_t width, size_t height) const
		{
			check_region(x, y, width, height);
			if (out.size() < width * height)
				throw std::invalid_argument(detail::text("get_region: buffer holds ", out.size(), " elements, the region has ", width * height));
			blosc2::batch::window_job job;
			plan_region(out.data(), width, x, y, width, height, job);
			blosc2::batch::decompress_windows(job);
		}
		/// The rectangle subsampled: every step_y-th row of it and every step_x-th element of those rows, ceil(height / step_y) rows
		/// of ceil(width / step_x) elements -- what a[y:y+height:step_y, x:x+width:step_x] is.  Only the blocks that hold a sampled
		/// element are decoded, and only the samples come back.
		std::vector<T> get_region(size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y) const
		{
			check_steps(step_x, step_y);
			std::vector<T> out(((width + step_x - 1) / step_x) * ((height + step_y - 1) / step_y));
			get_region(std::span<T>(out), x, y, width, height, step_x, step_y);
			return out;
		}
		void get_region(std::span<T> out, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y) const
		{
			check_region(x, y, width, height);
			check_steps(step_x, step_y);
			const size_t ow = (width + step_x - 1) / step_x, oh = (height + step_y - 1) / step_y;
			if (out.size() < ow * oh)
				throw std::invalid_argument(detail::text("get_region: buffer holds ", out.size(), " elements, the subsampled region has ", ow * oh));
			blosc2::batch::strided_window_job job;
			plan_region(out.data(), ow, x, y, width, height, step_x, step_y, job);
			blosc2::batch::decompress_windows(job);
		}
		/// Many rectangles in ONE engine call that decodes every block once, however many of the regions meet it (blocks are runs of
		/// whole scanlines: regions that share rows share blocks).  The results lie back to back in region order, each row-major
		/// with its subsampled shape out_height() x out_width().  Every region is checked before anything runs (get_region's
		/// exceptions); an empty list does nothing.
		std::vector<T> get_regions(std::span<const region> regions) const
		{
			std::vector<T> out(check_regions(regions));
			get_regions(std::span<T>(out), regions);
			return out;
		}
		void get_regions(std::span<T> out, std::span<const region> regions) const
		{
			const size_t total = check_regions(regions);
			if (out.size() < total)
				throw std::invalid_argument(detail::text("get_regions: buffer holds ", out.size(), " elements, the regions have ", total));
			blosc2::batch::strided_window_job job;
			job.share_runs = true;
			size_t at = 0;
			for (const region& r : regions)
			{
				plan_region(out.data() + at, r.out_width(), r.x, r.y, r.width, r.height, r.step_x, r.step_y, job);
				at += r.out_elems();
			}
			blosc2::batch::decompress_windows_grouped(job);
		}
		/// Every region checked as get_region checks it; returns the elements of all results together.
		size_t check_regions(std::span<const region> regions) const
		{
			size_t total = 0;
			for (const region& r : regions)
			{
				check_region(r.x, r.y, r.width, r.height);
				check_steps(r.step_x, r.step_y);
				total += r.out_elems();
			}
			return total;
		}
		/// Write `data` (width * height elements, row-major) over the rectangle [x, x + width) x [y, y + height).  Only the blocks
		/// the rectangle meets are decoded and re-encoded, on the device; the result is what compressing the edited pixels from
		/// scratch gives.  Lazy chunks the rectangle meets become real.  Nothing changes unless the whole call succeeds.
		void set_region(std::span<const T> data, size_t x, size_t y, size_t width, size_t height)
		{
			check_region(x, y, width, height);
			if (data.size() != width * height)
				throw std::invalid_argument(detail::text("set_region: span holds ", data.size(), " elements, the region has ", width * height));
			require();
			require_encoder();
			blosc2::batch::update_job job;
			region_cparams(job.cparams);
			std::visit([&](auto& s) {
				using table_t = std::decay_t<decltype(s)>;
				typename table_t::region_write rw;
				s.plan_region_write(data.data(), width, m_Width, x, y, width, height, job, rw);
				auto made = blosc2::batch::update_windows(job);
				s.prepare_region_write(m_CompressionContext.get(), rw, made);
				s.commit_region_write(rw);
			}, *m_Schunk);
		}
		/// Write `data` over every step_y-th row and every step_x-th element of the rectangle: data holds ceil(height / step_y) rows of
		/// ceil(width / step_x) elements, what get_region with the same steps returns.  Only the blocks that hold a written element are
		/// decoded and re-encoded.  A step of 0 throws std::invalid_argument.
		void set_region(std::span<const T> data, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), data);
		}
		/// Many rectangles in ONE engine call.  The data lies back to back in region order, each region row-major in its subsampled
		/// shape -- the layout get_regions returns.  Later regions win where two overlap.  Every region is checked before anything
		/// runs; an empty list does nothing; lazy chunks a region meets become real; nothing changes unless the whole call succeeds.
		void set_regions(std::span<const region> regions, std::span<const T> data)
		{
			const size_t total = check_regions(regions);
			if (data.size() != total)
				throw std::invalid_argument(detail::text("set_regions: span holds ", data.size(), " elements, the regions have ", total));
			if (total == 0) return;
			require();
			require_encoder();
			blosc2::batch::update_job_strided job;
			region_cparams(job.cparams);
			std::visit([&](auto& s) {
				using table_t = std::decay_t<decltype(s)>;
				typename table_t::region_write rw;
				s.plan_regions_write(data.data(), region_rects<table_t>(regions, 0, 1), m_Width, job, rw);
				auto made = blosc2::batch::update_windows_strided(job);
				s.prepare_region_write(m_CompressionContext.get(), rw, made);
				s.commit_region_write(rw);
			}, *m_Schunk);
		}
		/// Paint the (subsampled) rectangle with one value: np.copyto(view, value).  No h x w copies of the value exist anywhere: only
		/// the touched chunks go to the device.  With trunc-prec storage the value is truncated like any written pixel.
		void fill_region(T value, size_t x, size_t y, size_t width, size_t height, size_t step_x = 1, size_t step_y = 1)
		{
			const region r{ x, y, width, height, step_x, step_y };
			fill_regions(std::span<const region>(&r, 1), std::span<const T>(&value, 1));
		}
		/// Many rectangles painted in ONE engine call: `values` holds one value for all regions or one per region; later regions win.
		void fill_regions(std::span<const region> regions, std::span<const T> values) { write_masked(regions, nullptr, values, nullptr, "fill_regions"); }
		/// fill_regions through mattes: `mask` holds one byte an element, back to back in region order, each region row-major in its
		/// subsampled shape; an element is painted where its mask byte is not 0 and keeps its value elsewhere.
		void fill_regions(std::span<const region> regions, std::span<const T> values, std::span<const uint8_t> mask)
		{
			if (mask.size() != check_regions(regions))
				throw std::invalid_argument(detail::text("fill_regions: the mask holds ", mask.size(), " bytes, the regions have ", check_regions(regions), " elements"));
			if (mask.empty()) return;                                 // (no element anywhere)
			write_masked(regions, nullptr, values, mask.data(), "fill_regions");
		}
		/// set_region through a matte: np.copyto(view, data, where=mask).  data and mask have the subsampled shape.  One engine call,
		/// every touched block decoded once.  (The mask trails the steps, which have no defaults here.)
		void set_region(std::span<const T> data, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, std::span<const uint8_t> mask)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), data, mask);
		}
		/// set_regions through mattes: data and masks lie back to back in region order, both in the subsampled shapes.
		void set_regions(std::span<const region> regions, std::span<const T> data, std::span<const uint8_t> mask)
		{
			const size_t total = check_regions(regions);
			if (data.size() != total)
				throw std::invalid_argument(detail::text("set_regions: span holds ", data.size(), " elements, the regions have ", total));
			if (mask.size() != total)
				throw std::invalid_argument(detail::text("set_regions: the mask holds ", mask.size(), " bytes, the regions have ", total, " elements"));
			if (total == 0) return;
			write_masked(regions, data.data(), std::span<const T>(), mask.data(), "set_regions");
		}
		/// The regions as the chunk table takes them for a masked / constant write of channel `channel` of `channels`: data region-major,
		/// channel-minor as in region_rects, the mask region-major only (an image's channels share it); value: this channel's, one or
		/// one per region.
		template <typename Table>
		static std::vector<typename Table::masked_rect> masked_rects(std::span<const region> regions, size_t channel, size_t channels, std::span<const T> values)
		{
			std::vector<typename Table::masked_rect> out;
			size_t at = 0, mat = 0;
			for (size_t k = 0; k < regions.size(); ++k)
			{
				const region& r = regions[k];
				const size_t n = r.out_elems();
				const T v = values.empty() ? T{} : values[values.size() == 1 ? 0 : k];
				if (n) out.push_back({ { r.x, r.y, (r.width + r.step_x - 1) / r.step_x, (r.height + r.step_y - 1) / r.step_y, r.step_x, r.step_y, at + channel * n }, mat, v });
				at += channels * n;
				mat += n;
			}
			return out;
		}
		/// fill_regions and the masked set_regions: ONE engine call (cimg_update_windows_masked_host).  Every region is checked before
		/// anything runs; lazy chunks a region meets become real; nothing changes unless the whole call succeeds.
		void write_masked(std::span<const region> regions, const T* src, std::span<const T> values, const uint8_t* mask, const char* what)
		{
			if (!src && values.size() != 1 && values.size() != regions.size())
				throw std::invalid_argument(detail::text(what, ": got ", values.size(), " values for ", regions.size(), " regions (one, or one per region)"));
			if (check_regions(regions) == 0) return;
			require();
			require_encoder();
			blosc2::batch::update_job_masked job;
			region_cparams(job.cparams);
			std::visit([&](auto& s) {
				using table_t = std::decay_t<decltype(s)>;
				typename table_t::region_write rw;
				s.plan_regions_write_masked(src, mask, masked_rects<table_t>(regions, 0, 1, values), m_Width, job, rw);
				auto made = blosc2::batch::update_windows_masked(job);
				s.prepare_region_write(m_CompressionContext.get(), rw, made);
				s.commit_region_write(rw);
			}, *m_Schunk);
		}
		/// The regions as the chunk table takes them; region k's data starts where `channels` channels of the regions before it end,
		/// plus `channel` pieces of its own (an image's data is region-major, channel-minor).
		template <typename Table>
		static std::vector<typename Table::strided_rect> region_rects(std::span<const region> regions, size_t channel, size_t channels)
		{
			std::vector<typename Table::strided_rect> out;
			size_t at = 0;
			for (const region& r : regions)
			{
				const size_t n = r.out_elems();
				if (n) out.push_back({ r.x, r.y, (r.width + r.step_x - 1) / r.step_x, (r.height + r.step_y - 1) / r.step_y, r.step_x, r.step_y, at + channel * n });
				at += channels * n;
			}
			return out;
		}
		/// The codec parameters of this channel's compression context (what set_region hands the engine).
		void region_cparams(cimg_cparams& out) const
		{
			require_encoder();
			const int rc = cimg_context_cparams(m_CompressionContext.get(), &out);
			if (rc < 0) throw std::runtime_error(detail::text("Unable to read the compression parameters, error code ", rc));
		}
		blosc2::context_raw_ptr compression_context() const { return m_CompressionContext.get(); }

		/// Batch building block of image<T>::get_region: queue this channel's windows (rows out_pitch elements apart).
		void plan_region(T* out, size_t out_pitch, size_t x, size_t y, size_t width, size_t height, blosc2::batch::window_job& job) const
		{
			visit([&](const auto& s) { s.plan_region(out, out_pitch, m_Width, x, y, width, height, job); return 0; });
		}
		void plan_region(T* out, size_t out_pitch, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y,
			blosc2::batch::strided_window_job& job) const
		{
			visit([&](const auto& s) { s.plan_region(out, out_pitch, m_Width, x, y, width, height, step_x, step_y, job); return 0; });
		}
		static void check_steps(size_t step_x, size_t step_y)
		{
			if (step_x == 0 || step_y == 0) throw std::invalid_argument("get_region: step_x and step_y must be at least 1");
		}
		void check_region(size_t x, size_t y, size_t width, size_t height) const
		{
			if (x > m_Width || y > m_Height || width > m_Width - x || height > m_Height - y)
				throw std::out_of_range(detail::text("Region (x ", x, ", y ", y, ", width ", width, ", height ", height, ") is out of bounds for a channel of ",
					m_Width, " x ", m_Height));
		}

		/// The chunk table itself (used by image<T> to batch across channels).
		blosc2::schunk_var<T>& chunks() { require(); return *m_Schunk; }
		const blosc2::schunk_var<T>& chunks() const { require(); return *m_Schunk; }

		bool operator==(const channel<T>& other) const noexcept { return this == &other; }

	private:
		blosc2::schunk_var_ptr<T> m_Schunk = nullptr;
		enums::codec m_Codec = enums::codec::lz4;
		size_t m_Nthreads = std::thread::hardware_concurrency() / 2;
		blosc2::context_ptr m_CompressionContext = nullptr;
		blosc2::context_ptr m_DecompressionContext = nullptr;
		uint8_t m_CompressionLevel = 9;
		std::optional<int> m_MantissaBits = std::nullopt;
		bool m_Adopted = false;
		size_t m_Width = 1;
		size_t m_Height = 1;

		// All four codecs of the reference have an encoder on this path since round 3 (lz4hc / zstd: format-valid, not the CPU
		// libraries' bytes -- enums.h), so an adopted chunk table of any of them can be rewritten like one built from pixels.
		void make_contexts(size_t block_size)
		{
			m_CompressionContext = blosc2::create_compression_context<T>(m_Nthreads, m_Codec, m_CompressionLevel, block_size, m_MantissaBits);
			m_DecompressionContext = blosc2::create_decompression_context(m_Nthreads);
		}
		void require_encoder() const
		{
			if (!m_CompressionContext)
				throw std::runtime_error("Internal Error: Channel instance has no compression context");
		}
		void require() const
		{
			if (!m_Schunk)
				throw std::runtime_error("Internal Error: Channel instance is not properly initialized, unable to access its data");
		}
		template <typename F> auto visit(F&& f) const
		{
			require();
			return std::visit(std::forward<F>(f), const_cast<const blosc2::schunk_var<T>&>(*m_Schunk));
		}
	};
}
