// image.h -- compressed::image<T>: a set of equally sized compressed channels with names and metadata
// (reference compressed/image.h: constructors :87-325, add/remove/extract :940-1118, statistics
// :1122-1170, accessors :1192-1440, get_decompressed :1307-1315).
//
// Construction from planar pixels and get_decompressed() batch ACROSS channels: all chunks of all
// channels go to the MI355X engine in one call (the reference loops channels serially, image.h:119-159).
// Out of scope in this build: every read() overload and read_oiio_metadata (OpenImageIO is absent; what the read path does
// with the scanlines once it has them -- deinterleave, compress -- is image::from_interleaved) and
// JSON metadata (nlohmann-json is absent; metadata is an ordered string map here).
#pragma once
#include <cstddef>
#include <cstring>
#include <iostream>
#include <map>
#include <optional>
#include <span>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "channel.h"
#include "constants.h"
#include "enums.h"
#include "macros.h"
#include "util.h"

namespace NAMESPACE_COMPRESSED_IMAGE
{
	using metadata_map = std::map<std::string, std::string>;

	template <typename T>
	struct image
	{
		image() = default;
		image(image&&) = default;
		image& operator=(image&&) = default;
		image(const image&) = delete;
		image& operator=(const image&) = delete;

		/// Compress planar channels (each width * height elements).  mantissa_bits: as channel<T>'s, for every channel.
		image(std::vector<std::span<const T>> channels, size_t width, size_t height, std::vector<std::string> channel_names = {},
			enums::codec compression_codec = enums::codec::lz4, size_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
			: m_Width(width), m_Height(height)
		{
			adopt_names(channel_names, channels.size());
			const uint8_t level = util::ensure_compression_level(compression_level);
			for (const auto& c : channels)
				if (c.size() != width * height)
					throw std::runtime_error(detail::text("Invalid channel data passed. Expected its size to match up to width * height (", width, " * ", height,
						") which would be ", width * height, ". Instead received ", c.size()));
			if (channels.empty()) return;

			// one engine call for every chunk of every channel
			const size_t aligned = util::align_chunk_to_scanlines_bytes<T>(width, chunk_size);
			auto cctx = blosc2::create_compression_context<T>(1, compression_codec, level, block_size, mantissa_bits);
			std::vector<blosc2::batch::piece> pieces;
			std::vector<size_t> first(channels.size() + 1, 0);
			for (size_t ch = 0; ch < channels.size(); ++ch)
			{
				const auto* base = reinterpret_cast<const std::byte*>(channels[ch].data());
				const size_t total = channels[ch].size() * sizeof(T);
				for (size_t off = 0; off < total; off += aligned) pieces.push_back({ base + off, std::min(aligned, total - off) });
				first[ch + 1] = pieces.size();
			}
			auto chunks = blosc2::batch::compress(cctx.get(), pieces, aligned);
			for (size_t ch = 0; ch < channels.size(); ++ch)
			{
				blosc2::schunk<T> table(block_size, aligned);
				for (size_t i = first[ch]; i < first[ch + 1]; ++i) table.append_chunk(std::move(chunks[i]));
				m_Channels.push_back(compressed::channel<T>(blosc2::schunk_var<T>(std::move(table)), width, height, compression_codec, level, mantissa_bits));
			}
		}

		image(std::vector<std::vector<T>> channels, size_t width, size_t height, std::vector<std::string> channel_names = {},
			enums::codec compression_codec = enums::codec::lz4, size_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
			: image(as_spans(channels), width, height, std::move(channel_names), compression_codec, compression_level, block_size, chunk_size, mantissa_bits) {}

		/// Compress channels that arrive INTERLEAVED (R G B A R G B A ..., what an image reader hands out per block of
		/// scanlines; the reference's read path deinterleaves them on the host before compressing, image.h:1555-1880 with
		/// image_algo::deinterleave at :1880).  Not a constructor of the reference -- its read path is tied to OpenImageIO --
		/// but the same work: the interleaved pixels are uploaded once, split into planes on the device and compressed
		/// from there, all channels in one engine call.
		static image from_interleaved(std::span<const T> interleaved, size_t width, size_t height, size_t nchannels, std::vector<std::string> channel_names = {},
			enums::codec compression_codec = enums::codec::lz4, size_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
		{
			if (nchannels == 0 || interleaved.size() != width * height * nchannels)
				throw std::runtime_error(detail::text("Invalid interleaved data passed. Expected its size to match up to width * height * channels (", width, " * ", height,
					" * ", nchannels, "). Instead received ", interleaved.size()));
			image out;
			out.m_Width = width; out.m_Height = height;
			out.adopt_names(channel_names, nchannels);
			const uint8_t level = util::ensure_compression_level(compression_level);
			const size_t aligned = util::align_chunk_to_scanlines_bytes<T>(width, chunk_size);
			auto cctx = blosc2::create_compression_context<T>(1, compression_codec, level, block_size, mantissa_bits);
			const size_t npixels = width * height, total = npixels * sizeof(T);
			const size_t stride = blosc2::batch::planar_stride(npixels, sizeof(T));
			std::vector<blosc2::batch::planar_piece> pieces;
			std::vector<size_t> first(nchannels + 1, 0);
			for (size_t ch = 0; ch < nchannels; ++ch)
			{
				for (size_t off = 0; off < total; off += aligned) pieces.push_back({ ch * stride + off, std::min(aligned, total - off) });
				first[ch + 1] = pieces.size();
			}
			auto chunks = blosc2::batch::compress_interleaved(cctx.get(), reinterpret_cast<const std::byte*>(interleaved.data()), nchannels, npixels, pieces, aligned);
			for (size_t ch = 0; ch < nchannels; ++ch)
			{
				blosc2::schunk<T> table(block_size, aligned);
				for (size_t i = first[ch]; i < first[ch + 1]; ++i) table.append_chunk(std::move(chunks[i]));
				out.m_Channels.push_back(compressed::channel<T>(blosc2::schunk_var<T>(std::move(table)), width, height, compression_codec, level, mantissa_bits));
			}
			return out;
		}

		/// Adopt already compressed channels.
		image(std::vector<compressed::channel<T>> channels, size_t width, size_t height, std::vector<std::string> channel_names = {})
			: m_Width(width), m_Height(height)
		{
			adopt_names(channel_names, channels.size());
			for (auto& c : channels)
			{
				check_dims(c.width(), c.height(), "");
				m_Channels.push_back(std::move(c));
			}
		}

		// ---- channel management ----------------------------------------------------------------------------
		void add_channel(compressed::channel<T> _channel, std::optional<std::string> name = std::nullopt)
		{
			check_dims(_channel.width(), _channel.height(), name.value_or(""));
			push_name(name);
			m_Channels.push_back(std::move(_channel));
		}
		/// note the reference's default level for THIS overload is 5, not 9 (image.h:999)
		void add_channel(std::span<const T> data, size_t width, size_t height, std::optional<std::string> name = std::nullopt,
			enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 5, std::optional<int> mantissa_bits = std::nullopt)
		{
			check_dims(width, height, name.value_or(""));
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			push_name(name);
			m_Channels.push_back(compressed::channel<T>(data, width, height, compression_codec, compression_level, s_default_blocksize, s_default_chunksize, mantissa_bits));
		}

		void remove_channel(size_t index) { (void)extract_channel(index); }
		void remove_channel(const std::string_view name) { (void)extract_channel(name); }

		compressed::channel<T> extract_channel(size_t index)
		{
			if (index >= m_Channels.size()) throw std::out_of_range("Channel index out of range");
			auto out = std::move(m_Channels[index]);
			m_Channels.erase(m_Channels.begin() + static_cast<std::ptrdiff_t>(index));
			if (index < m_ChannelNames.size()) m_ChannelNames.erase(m_ChannelNames.begin() + static_cast<std::ptrdiff_t>(index));
			return out;
		}
		compressed::channel<T> extract_channel(const std::string_view name) { return extract_channel(get_channel_offset(name)); }

		compressed::channel<T>& channel(size_t index)
		{
			if (index >= m_Channels.size())
				throw std::out_of_range(detail::text("Channel index ", index, " is out of range for an image with ", m_Channels.size(), " channels"));
			return m_Channels[index];
		}
		compressed::channel<T>& channel(const std::string_view name) { return m_Channels[get_channel_offset(name)]; }
		std::vector<compressed::channel<T>>& channels() { return m_Channels; }
		const std::vector<compressed::channel<T>>& channels() const { return m_Channels; }

		size_t get_channel_offset(const std::string_view channelname) const
		{
			for (size_t i = 0; i < m_ChannelNames.size(); ++i) if (m_ChannelNames[i] == channelname) return i;
			throw std::invalid_argument(detail::text("Unknown channelname '", channelname, "' encountered"));
		}

		// ---- pixels -------------------------------------------------------------------------------------------
		/// All channels, decompressed -- one engine call for every chunk of the image.
		std::vector<std::vector<T>> get_decompressed() const
		{
			std::vector<std::vector<T>> out(m_Channels.size());
			std::vector<blosc2::batch::target> work;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				out[ch].resize(m_Channels[ch].uncompressed_size());
				std::visit([&](const auto& table) { table.plan_decode(out[ch].data(), work); }, m_Channels[ch].chunks());
			}
			blosc2::batch::decompress(work);
			return out;
		}

		/// The rectangle [x, x + width) x [y, y + height) of every channel (row-major, width elements a row) -- one engine call
		/// that decodes only the blocks the rectangle meets.
		std::vector<std::vector<T>> get_region(size_t x, size_t y, size_t width, size_t height) const
		{
			std::vector<std::vector<T>> out(m_Channels.size());
			blosc2::batch::window_job job;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				m_Channels[ch].check_region(x, y, width, height);
				out[ch].resize(width * height);
				m_Channels[ch].plan_region(out[ch].data(), width, x, y, width, height, job);
			}
			blosc2::batch::decompress_windows(job);
			return out;
		}

		/// The rectangle of every channel subsampled (channel<T>::get_region with steps): one engine call that decodes only the
		/// blocks that hold a sampled element.
		std::vector<std::vector<T>> get_region(size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y) const
		{
			if (step_x == 0 || step_y == 0) throw std::invalid_argument("get_region: step_x and step_y must be at least 1");
			const size_t ow = (width + step_x - 1) / step_x, oh = (height + step_y - 1) / step_y;
			std::vector<std::vector<T>> out(m_Channels.size());
			blosc2::batch::strided_window_job job;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				m_Channels[ch].check_region(x, y, width, height);
				out[ch].resize(ow * oh);
				m_Channels[ch].plan_region(out[ch].data(), ow, x, y, width, height, step_x, step_y, job);
			}
			blosc2::batch::decompress_windows(job);
			return out;
		}

		/// Many rectangles of every channel in ONE engine call that decodes every block once (channel<T>::get_regions).  The results
		/// lie back to back in region order and, within a region, in channel order (region-major, channel-minor), each row-major with
		/// the region's subsampled shape.  Every region is checked before anything runs; an empty list does nothing.
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
				for (const auto& ch : m_Channels)
				{
					ch.plan_region(out.data() + at, r.out_width(), r.x, r.y, r.width, r.height, r.step_x, r.step_y, job);
					at += r.out_elems();
				}
			blosc2::batch::decompress_windows_grouped(job);
		}
		/// Every region checked against every channel; returns the elements of all results together.
		size_t check_regions(std::span<const region> regions) const
		{
			size_t total = 0;
			for (const auto& ch : m_Channels) total += ch.check_regions(regions);
			return total;
		}

		/// Write one span per channel (width * height elements each, row-major) over the rectangle of every channel: one engine call
		/// for all channels that share their codec parameters.  Nothing changes unless the whole call succeeds.
		void set_region(const std::vector<std::span<const T>>& data, size_t x, size_t y, size_t width, size_t height)
		{
			if (data.size() != m_Channels.size())
				throw std::invalid_argument(detail::text("set_region: got ", data.size(), " spans for ", m_Channels.size(), " channels"));
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				m_Channels[ch].check_region(x, y, width, height);
				if (data[ch].size() != width * height)
					throw std::invalid_argument(detail::text("set_region: span ", ch, " holds ", data[ch].size(), " elements, the region has ", width * height));
			}
			// one engine call per distinct set of codec parameters (one for an image whose channels share them); every call and every
			// lazy chunk's compress happens before the first chunk of any channel is replaced
			std::vector<blosc2::batch::update_job> jobs;
			std::vector<size_t> job_of(m_Channels.size());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				cimg_cparams c{};
				m_Channels[ch].region_cparams(c);
				size_t k = 0;
				while (k < jobs.size() && std::memcmp(&jobs[k].cparams, &c, sizeof c) != 0) ++k;
				if (k == jobs.size()) { jobs.emplace_back(); jobs.back().cparams = c; }
				job_of[ch] = k;
			}
			using table_var = std::variant<typename blosc2::schunk<T>::region_write, typename blosc2::lazy_schunk<T>::region_write>;
			std::vector<table_var> rws;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					typename std::decay_t<decltype(table)>::region_write rw;
					table.plan_region_write(data[ch].data(), width, m_Channels[ch].width(), x, y, width, height, jobs[job_of[ch]], rw);
					rws.emplace_back(std::move(rw));
				}, m_Channels[ch].chunks());
			std::vector<std::vector<std::vector<std::byte>>> made;
			for (auto& job : jobs) made.push_back(blosc2::batch::update_windows(job));
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.prepare_region_write(m_Channels[ch].compression_context(), std::get<rw_t>(rws[ch]), made[job_of[ch]]);
				}, m_Channels[ch].chunks());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.commit_region_write(std::get<rw_t>(rws[ch]));
				}, m_Channels[ch].chunks());
		}

		/// Write one span per channel over every step_y-th row and step_x-th element of the rectangle of every channel; each span holds
		/// ceil(height / step_y) x ceil(width / step_x) elements.  A step of 0 throws std::invalid_argument.
		void set_region(const std::vector<std::span<const T>>& data, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y)
		{
			if (data.size() != m_Channels.size())
				throw std::invalid_argument(detail::text("set_region: got ", data.size(), " spans for ", m_Channels.size(), " channels"));
			const region r{ x, y, width, height, step_x, step_y };
			for (const auto& ch : m_Channels) ch.check_regions(std::span<const region>(&r, 1));
			std::vector<T> all;
			all.reserve(data.size() * r.out_elems());
			for (size_t ch = 0; ch < data.size(); ++ch)
			{
				if (data[ch].size() != r.out_elems())
					throw std::invalid_argument(detail::text("set_region: span ", ch, " holds ", data[ch].size(), " elements, the subsampled region has ", r.out_elems()));
				all.insert(all.end(), data[ch].begin(), data[ch].end());
			}
			set_regions(std::span<const region>(&r, 1), std::span<const T>(all));
		}
		/// Many rectangles of every channel: the data is region-major, channel-minor, each piece row-major in its subsampled shape --
		/// the layout get_regions returns.  One engine call for all channels that share their codec parameters; later regions win;
		/// every region is checked before anything runs; an empty list does nothing; nothing changes unless the whole call succeeds.
		void set_regions(std::span<const region> regions, std::span<const T> data)
		{
			size_t total = 0;
			for (const auto& ch : m_Channels) total += ch.check_regions(regions);
			if (data.size() != total)
				throw std::invalid_argument(detail::text("set_regions: span holds ", data.size(), " elements, the regions have ", total));
			if (total == 0) return;
			std::vector<blosc2::batch::update_job_strided> jobs;
			std::vector<size_t> job_of(m_Channels.size());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				cimg_cparams c{};
				m_Channels[ch].region_cparams(c);
				size_t k = 0;
				while (k < jobs.size() && std::memcmp(&jobs[k].cparams, &c, sizeof c) != 0) ++k;
				if (k == jobs.size()) { jobs.emplace_back(); jobs.back().cparams = c; }
				job_of[ch] = k;
			}
			using table_var = std::variant<typename blosc2::schunk<T>::region_write, typename blosc2::lazy_schunk<T>::region_write>;
			std::vector<table_var> rws;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using table_t = std::decay_t<decltype(table)>;
					typename table_t::region_write rw;
					table.plan_regions_write(data.data(), compressed::channel<T>::template region_rects<table_t>(regions, ch, m_Channels.size()), m_Channels[ch].width(),
						jobs[job_of[ch]], rw);
					rws.emplace_back(std::move(rw));
				}, m_Channels[ch].chunks());
			std::vector<std::vector<std::vector<std::byte>>> made;
			for (auto& job : jobs) made.push_back(blosc2::batch::update_windows_strided(job));
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.prepare_region_write(m_Channels[ch].compression_context(), std::get<rw_t>(rws[ch]), made[job_of[ch]]);
				}, m_Channels[ch].chunks());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.commit_region_write(std::get<rw_t>(rws[ch]));
				}, m_Channels[ch].chunks());
		}

		/// Paint the (subsampled) rectangle of every channel: `values` holds one value for all channels or one a channel.
		void fill_region(std::span<const T> values, size_t x, size_t y, size_t width, size_t height, size_t step_x = 1, size_t step_y = 1)
		{
			const region r{ x, y, width, height, step_x, step_y };
			fill_regions(std::span<const region>(&r, 1), values);
		}
		/// Many rectangles of every channel painted: one engine call for all channels that share their codec parameters.
		void fill_regions(std::span<const region> regions, std::span<const T> values) { write_masked(regions, nullptr, values, nullptr, false, "fill_regions"); }
		/// fill_regions through mattes.  The channels share ONE mask: a byte an element of a region (not of a region and channel), back
		/// to back in region order, each region row-major in its subsampled shape.
		void fill_regions(std::span<const region> regions, std::span<const T> values, std::span<const uint8_t> mask)
		{
			write_masked(regions, nullptr, values, &mask, false, "fill_regions");
		}
		/// set_region of every channel through one shared matte: data as set_regions takes it (channel-minor), mask (h', w').
		void set_region(std::span<const T> data, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, std::span<const uint8_t> mask)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), data, mask);
		}
		/// set_regions through mattes: data region-major, channel-minor; ONE mask for all channels, region-major.
		void set_regions(std::span<const region> regions, std::span<const T> data, std::span<const uint8_t> mask)
		{
			size_t total = 0;
			for (const auto& ch : m_Channels) total += ch.check_regions(regions);
			if (data.size() != total)
				throw std::invalid_argument(detail::text("set_regions: span holds ", data.size(), " elements, the regions have ", total));
			write_masked(regions, data.data(), std::span<const T>(), &mask, true, "set_regions");
		}
		/// fill_regions and the masked set_regions of every channel: one engine call (cimg_update_windows_masked_host) per group of
		/// channels that share their codec parameters; every region is checked before anything runs; lazy chunks a region meets become
		/// real; nothing changes unless the whole call succeeds.
		void write_masked(std::span<const region> regions, const T* src, std::span<const T> values, const std::span<const uint8_t>* mask, bool has_src, const char* what)
		{
			if (!has_src && values.size() != 1 && values.size() != m_Channels.size())
				throw std::invalid_argument(detail::text(what, ": got ", values.size(), " values for ", m_Channels.size(), " channels (one, or one a channel)"));
			size_t per_channel = 0;
			for (const auto& ch : m_Channels) per_channel = ch.check_regions(regions);
			if (mask && mask->size() != per_channel)
				throw std::invalid_argument(detail::text(what, ": the mask holds ", mask->size(), " bytes, the regions have ", per_channel, " elements a channel"));
			if (per_channel == 0 || m_Channels.empty()) return;
			std::vector<blosc2::batch::update_job_masked> jobs;
			std::vector<size_t> job_of(m_Channels.size());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
			{
				cimg_cparams c{};
				m_Channels[ch].region_cparams(c);
				size_t k = 0;
				while (k < jobs.size() && std::memcmp(&jobs[k].cparams, &c, sizeof c) != 0) ++k;
				if (k == jobs.size()) { jobs.emplace_back(); jobs.back().cparams = c; }
				job_of[ch] = k;
			}
			using table_var = std::variant<typename blosc2::schunk<T>::region_write, typename blosc2::lazy_schunk<T>::region_write>;
			std::vector<table_var> rws;
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using table_t = std::decay_t<decltype(table)>;
					typename table_t::region_write rw;
					const T v = has_src ? T{} : values[values.size() == 1 ? 0 : ch];
					table.plan_regions_write_masked(src, mask ? mask->data() : nullptr,
						compressed::channel<T>::template masked_rects<table_t>(regions, ch, m_Channels.size(), std::span<const T>(&v, 1)), m_Channels[ch].width(),
						jobs[job_of[ch]], rw);
					rws.emplace_back(std::move(rw));
				}, m_Channels[ch].chunks());
			std::vector<std::vector<std::vector<std::byte>>> made;
			for (auto& job : jobs) made.push_back(blosc2::batch::update_windows_masked(job));
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.prepare_region_write(m_Channels[ch].compression_context(), std::get<rw_t>(rws[ch]), made[job_of[ch]]);
				}, m_Channels[ch].chunks());
			for (size_t ch = 0; ch < m_Channels.size(); ++ch)
				std::visit([&](auto& table) {
					using rw_t = typename std::decay_t<decltype(table)>::region_write;
					table.commit_region_write(std::get<rw_t>(rws[ch]));
				}, m_Channels[ch].chunks());
		}

		/// All channels into caller-owned memory (num_channels * height * width elements, channel-major): no
		/// intermediate vectors, no zero fill -- what the Python binding uses to decode straight into a numpy array.
		void decompress_into(std::span<T> out) const
		{
			size_t need = 0;
			for (const auto& c : m_Channels) need += c.uncompressed_size();
			if (out.size() != need)
				throw std::invalid_argument(detail::text("decompress_into: buffer holds ", out.size(), " elements, image has ", need));
			std::vector<blosc2::batch::target> work;
			size_t at = 0;
			for (const auto& c : m_Channels)
			{
				std::visit([&](const auto& table) { table.plan_decode(out.data() + at, work); }, c.chunks());
				at += c.uncompressed_size();
			}
			blosc2::batch::decompress(work);
		}

		// ---- statistics ----------------------------------------------------------------------------------------
		void print_statistics()
		{
			size_t csize = 0, usize = 0, nchunks = 0;
			for (const auto& c : m_Channels) { csize += c.compressed_bytes(); usize += c.uncompressed_size() * sizeof(T); nchunks += c.num_chunks(); }
			std::cout << "Statistics for image buffer:\n Width: " << m_Width << "\n Height: " << m_Height << "\n Channels: " << m_Channels.size()
				<< "\n Channelnames: [";
			for (size_t i = 0; i < m_ChannelNames.size(); ++i) std::cout << (i ? ", " : "") << m_ChannelNames[i];
			std::cout << "]\n --------------\n Compressed Size: " << csize << "\n Uncompressed Size: " << usize << "\n Compression ratio: "
				<< static_cast<double>(usize) / static_cast<double>(csize ? csize : 1) << "x\n Num Chunks: " << nchunks << std::endl;
		}
		/// uncompressed / compressed bytes; both sums start at 1 as in the reference (image.h:1162-1163)
		double compression_ratio() const noexcept
		{
			size_t csize = 1, usize = 1;
			for (const auto& c : m_Channels) { csize += c.compressed_bytes(); usize += c.uncompressed_size() * sizeof(T); }
			return static_cast<double>(usize) / static_cast<double>(csize);
		}

		// ---- plain accessors ---------------------------------------------------------------------------------------
		size_t width() const noexcept { return m_Width; }
		size_t height() const noexcept { return m_Height; }
		size_t num_channels() const noexcept { return m_Channels.size(); }
		std::vector<std::string> channelnames() const noexcept { return m_ChannelNames; }
		void channelnames(std::vector<std::string> names)
		{
			if (names.size() != m_Channels.size())
				throw std::invalid_argument(detail::text("Invalid number of arguments received for setting channelnames. Expected vector size to be exactly ",
					m_Channels.size(), " but instead got ", names.size()));
			m_ChannelNames = std::move(names);
		}
		void metadata(const metadata_map& m) noexcept { m_Metadata = m; }
		metadata_map& metadata() noexcept { return m_Metadata; }
		const metadata_map& metadata() const noexcept { return m_Metadata; }

		void update_nthreads(size_t nthreads) { for (auto& c : m_Channels) c.update_nthreads(nthreads, c.block_size()); }
		size_t chunk_size() const
		{
			if (m_Channels.empty()) throw std::runtime_error("Unable to get chunk size from image without channels");
			return m_Channels.front().chunk_size();
		}
		/// mantissa bits kept by the first channel (nullopt: lossless, or no channels)
		std::optional<int> mantissa_bits() const noexcept { return m_Channels.empty() ? std::nullopt : m_Channels.front().mantissa_bits(); }
		size_t block_size() const
		{
			if (m_Channels.empty()) throw std::runtime_error("Unable to get block size from image without channels");
			return m_Channels.front().block_size();
		}

	private:
		std::vector<compressed::channel<T>> m_Channels{};
		std::vector<std::string> m_ChannelNames{};
		metadata_map m_Metadata{};
		size_t m_Width = 1;
		size_t m_Height = 1;

		static std::vector<std::span<const T>> as_spans(const std::vector<std::vector<T>>& v)
		{
			std::vector<std::span<const T>> out;
			for (const auto& c : v) out.emplace_back(c.data(), c.size());
			return out;
		}
		void adopt_names(const std::vector<std::string>& names, size_t nchannels)
		{
			if (names.size() != nchannels && !names.empty())
				std::cout << "Invalid number of channel names received, expected " << nchannels << " but instead got " << names.size()
					<< ". Ignoring channel names" << std::endl;
			else
				m_ChannelNames = names;
		}
		void push_name(const std::optional<std::string>& name)
		{
			if (name.has_value() && m_ChannelNames.size() == m_Channels.size()) m_ChannelNames.push_back(*name);
			else if (!m_ChannelNames.empty()) m_ChannelNames.push_back(name.value_or(""));
		}
		void check_dims(size_t width, size_t height, const std::string& name) const
		{
			if (width != m_Width)
				throw std::invalid_argument(detail::text("Cannot add channel '", name, "' to the image as its width does not match that of the image. Expected ",
					m_Width, " pixels but instead got ", width, " pixels"));
			if (height != m_Height)
				throw std::invalid_argument(detail::text("Cannot add channel '", name, "' to the image as its height does not match that of the image. Expected ",
					m_Height, " pixels but instead got ", height, " pixels"));
		}
	};
}
