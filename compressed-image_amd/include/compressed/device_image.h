// device_image.h -- compressed::device_image<T>: equally sized channels kept COMPRESSED IN DEVICE MEMORY, in ONE store.
//
// The counterpart of image<T> (image.h) for pixels that live on the GPU.  All channels are compressed in one engine batch into one
// allocation (device_channel.h: the store), so a region of every channel is ONE windows call over one base address, and, if the
// consumer wants pixels (h, w, C) instead of planes (C, h, w), one more launch interleaves them on the device.
// add_channel / remove_channel are not offered: the store is one packed allocation.
#pragma once
#include <optional>
#include <string>
#include <string_view>

#include "device_channel.h"
#include "image.h"

namespace NAMESPACE_COMPRESSED_IMAGE
{
	template <typename T>
	struct device_image
	{
		device_image() = default;
		device_image(device_image&&) noexcept = default;
		device_image& operator=(device_image&&) noexcept = default;
		device_image(const device_image&) = delete;
		device_image& operator=(const device_image&) = delete;

		/// Compress planar channels (each width * height elements in device memory), all in one engine batch.
		device_image(const std::vector<const T*>& d_channels, size_t width, size_t height, std::vector<std::string> channel_names = {},
			enums::codec compression_codec = enums::codec::lz4, size_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
		{
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			m_MantissaBits = mantissa_bits;
			init(compression_codec, compression_level, block_size, chunk_size, width, height, d_channels.size(), channel_names);
			if (d_channels.empty()) return;
			cimg_engine* e = blosc2::batch::engine();
			const size_t total = width * height * sizeof(T);
			const std::byte* base = reinterpret_cast<const std::byte*>(d_channels[0]);
			for (const T* c : d_channels)
			{
				detail::device_range(e, c, total, "device_image");
				base = std::min(base, reinterpret_cast<const std::byte*>(c));
			}
			std::vector<int64_t> raw_off;
			std::vector<int32_t> nbytes;
			for (const T* c : d_channels)
				for (size_t off = 0; off < total; off += m_ChunkSize)
				{
					raw_off.push_back(static_cast<int64_t>(reinterpret_cast<const std::byte*>(c) - base) + static_cast<int64_t>(off));
					nbytes.push_back(static_cast<int32_t>(std::min(m_ChunkSize, total - off)));
				}
			m_Store = detail::compress_to_store(prototype().cparams(), base, raw_off, nbytes, m_ChunkSize);
		}

		/// Channels that arrive INTERLEAVED in device memory (R G B A R G B A ...): split into planes on the device, then as above.
		static device_image from_interleaved(const T* d_interleaved, size_t width, size_t height, size_t nchannels, std::vector<std::string> channel_names = {},
			enums::codec compression_codec = enums::codec::lz4, size_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
		{
			if (nchannels == 0) throw std::runtime_error("Invalid interleaved data passed. Expected at least one channel");
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			cimg_engine* e = blosc2::batch::engine();
			const size_t npixels = width * height;
			detail::device_range(e, d_interleaved, npixels * nchannels * sizeof(T), "from_interleaved");
			if (reinterpret_cast<uintptr_t>(d_interleaved) & 15) throw std::invalid_argument("from_interleaved: the pixels must be 16-byte aligned");
			const size_t stride = blosc2::batch::planar_stride(npixels, sizeof(T));
			detail::device_store planes;
			planes.allocate(e, stride * nchannels + 64);
			detail::engine_call(e, cimg_deinterleave_device(e, d_interleaved, static_cast<int32_t>(nchannels), static_cast<int32_t>(sizeof(T)),
				static_cast<int64_t>(npixels), planes.base, static_cast<int64_t>(stride)), "Splitting the interleaved pixels");
			std::vector<const T*> ch(nchannels);
			for (size_t c = 0; c < nchannels; ++c) ch[c] = reinterpret_cast<const T*>(planes.base + c * stride);
			// (the batch is enqueued on the engine's stream behind the split, and returns after the stream has been synchronised)
			return device_image(ch, width, height, std::move(channel_names), compression_codec, compression_level, block_size, chunk_size, mantissa_bits);
		}

		/// The compressed chunks of a host image, moved over PCIe as they are.  Its channels must share codec, level, block and chunk size.
		static device_image from_image(const image<T>& host)
		{
			device_image out;
			const auto& chans = host.channels();
			if (chans.empty()) { out.m_Width = host.width(); out.m_Height = host.height(); return out; }
			out.init(chans[0].compression(), chans[0].compression_level(), chans[0].block_size(), chans[0].chunk_size(), host.width(), host.height(),
				chans.size(), host.channelnames());
			out.m_ChunkSize = chans[0].chunk_size();
			out.m_MantissaBits = chans[0].mantissa_bits();
			std::vector<std::vector<std::byte>> chunks;
			for (const auto& c : chans)
			{
				if (c.compression() != out.m_Codec || c.compression_level() != out.m_CompressionLevel || c.block_size() != out.m_BlockSize || c.chunk_size() != out.m_ChunkSize ||
					c.mantissa_bits() != out.m_MantissaBits)
					throw std::invalid_argument("from_image: the channels of the image differ in codec, level, block size, chunk size or mantissa bits");
				detail::host_chunks(c, chunks);
			}
			if (chunks.size() != out.m_NumChannels * out.chunks_per_channel()) throw std::runtime_error("from_image: unexpected chunk count");
			auto store = detail::upload_store(chunks);
			out.m_Store = std::move(store);
			return out;
		}
		image<T> to_image() const
		{
			std::vector<compressed::channel<T>> chans;
			for (size_t c = 0; c < m_NumChannels; ++c) chans.push_back(channel(c).to_channel());
			return image<T>(std::move(chans), m_Width, m_Height, m_ChannelNames);
		}

		static void wait_stream(void* stream) { device_channel<T>::wait_stream(stream); }

		/// A handle on channel `index` that shares this image's store and is read-only (edits go through set_region of the image).
		/// It keeps the store it was taken from: a later set_region of the image does not change what the handle decodes.
		device_channel<T> channel(size_t index) const
		{
			if (index >= m_NumChannels)
				throw std::out_of_range(detail::text("Channel index ", index, " is out of range for an image with ", m_NumChannels, " channels"));
			device_channel<T> c = prototype();
			c.m_Store = m_Store;
			c.m_First = index * chunks_per_channel();
			c.m_Count = chunks_per_channel();
			c.m_ReadOnly = true;
			return c;
		}
		device_channel<T> channel(const std::string_view name) const { return channel(get_channel_offset(name)); }
		size_t get_channel_offset(const std::string_view channelname) const
		{
			for (size_t i = 0; i < m_ChannelNames.size(); ++i) if (m_ChannelNames[i] == channelname) return i;
			throw std::invalid_argument(detail::text("Unknown channelname '", channelname, "' encountered"));
		}

		/// All channels into device memory (num_channels * height * width elements, channel-major): one engine call.
		void decompress_into(T* d_out) const
		{
			if (m_NumChannels == 0) return;
			cimg_engine* e = m_Store->engine;
			detail::device_range(e, d_out, m_NumChannels * m_Width * m_Height * sizeof(T), "decompress_into");
			const size_t n = m_Store->num_chunks();
			std::vector<int64_t> raw_off(n);
			int64_t at = 0;
			for (size_t i = 0; i < n; ++i) { raw_off[i] = at; at += m_Store->nbytes[i]; }
			std::vector<int32_t> status(n, 0);
			detail::engine_call(e, cimg_decompress_batch_device_sized(e, static_cast<int32_t>(n), m_Store->base, m_Store->off.data(), m_Store->cbytes.data(),
				m_Store->nbytes.data(), m_Store->blocksize.data(), d_out, raw_off.data(), status.data()), "Decompressing the image");
		}
		/// The rectangle of every channel in ONE windows call: planes (C, height, width) or, with `interleaved`, pixels
		/// (height, width, C) -- then the planes are decoded into scratch and one more launch interleaves them.
		void get_region(T* d_out, size_t x, size_t y, size_t width, size_t height, bool interleaved = false) const
		{
			prototype().check_region(x, y, width, height);
			if (m_NumChannels == 0 || width == 0 || height == 0) return;
			cimg_engine* e = m_Store->engine;
			const size_t plane = width * height * sizeof(T);
			detail::device_range(e, d_out, plane * m_NumChannels, "get_region");
			const bool il = interleaved && m_NumChannels > 1;                  // (one channel: planes and pixels are the same bytes)
			if (il && (reinterpret_cast<uintptr_t>(d_out) & 15)) throw std::invalid_argument("get_region: an interleaved result must be 16-byte aligned");
			const size_t stride = il ? blosc2::batch::planar_stride(width * height, sizeof(T)) : plane;
			detail::device_store scratch;
			if (il) scratch.allocate(e, stride * m_NumChannels + 64);
			std::vector<cimg_window> w;
			for (size_t c = 0; c < m_NumChannels; ++c) w.push_back(channel_window(c, x, y, width, height, c * stride));
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_lock lock(e);
			detail::engine_call(e, cimg_decompress_windows_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base, m_Store->off.data(),
				m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)), static_cast<int32_t>(w.size()),
				w.data(), il ? static_cast<void*>(scratch.base) : static_cast<void*>(d_out), status.data()), "Decoding the region");
			if (il)
				detail::engine_call(e, cimg_interleave_device(e, scratch.base, static_cast<int64_t>(stride), static_cast<int32_t>(m_NumChannels),
					static_cast<int32_t>(sizeof(T)), static_cast<int64_t>(width * height), d_out), "Interleaving the region");
		}
		/// The rectangle of every channel subsampled (every step_y-th row, every step_x-th element of it) in ONE strided windows call:
		/// planes (C, oh, ow) with oh = ceil(height / step_y), ow = ceil(width / step_x), or with `interleaved` pixels (oh, ow, C).
		void get_region(T* d_out, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, bool interleaved = false) const
		{
			prototype().check_region(x, y, width, height);
			device_channel<T>::check_steps(step_x, step_y);
			if (m_NumChannels == 0 || width == 0 || height == 0) return;
			cimg_engine* e = m_Store->engine;
			const size_t ow = (width + step_x - 1) / step_x, oh = (height + step_y - 1) / step_y;
			const size_t plane = ow * oh * sizeof(T);
			detail::device_range(e, d_out, plane * m_NumChannels, "get_region");
			const bool il = interleaved && m_NumChannels > 1;                  // (one channel: planes and pixels are the same bytes)
			if (il && (reinterpret_cast<uintptr_t>(d_out) & 15)) throw std::invalid_argument("get_region: an interleaved result must be 16-byte aligned");
			const size_t stride = il ? blosc2::batch::planar_stride(ow * oh, sizeof(T)) : plane;
			detail::device_store scratch;
			if (il) scratch.allocate(e, stride * m_NumChannels + 64);
			std::vector<cimg_window_strided> w;
			for (size_t c = 0; c < m_NumChannels; ++c)
			{
				device_channel<T> p = prototype();
				p.m_First = c * chunks_per_channel();
				p.m_Count = chunks_per_channel();
				w.push_back(p.region_window(x, y, width, height, step_x, step_y, c * stride));
			}
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_lock lock(e);
			detail::engine_call(e, cimg_decompress_windows_strided_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base,
				m_Store->off.data(), m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)),
				static_cast<int32_t>(w.size()), w.data(), il ? static_cast<void*>(scratch.base) : static_cast<void*>(d_out), status.data()),
				"Decoding the subsampled region");
			if (il)
				detail::engine_call(e, cimg_interleave_device(e, scratch.base, static_cast<int64_t>(stride), static_cast<int32_t>(m_NumChannels),
					static_cast<int32_t>(sizeof(T)), static_cast<int64_t>(ow * oh), d_out), "Interleaving the region");
		}
		/// Many rectangles of every channel into device memory in ONE engine call that decodes every block once.  The results lie back
		/// to back in region order and, within a region, in channel order (region-major, channel-minor): (N, C, h', w') for N regions
		/// of one shape.  Every region is checked before anything runs; an empty list does nothing.
		void get_regions(T* d_out, std::span<const region> regions) const
		{
			const size_t per_channel = prototype().check_regions(regions);
			if (m_NumChannels == 0) return;
			std::vector<cimg_window_strided> w;
			size_t at = 0;
			for (const region& r : regions)
				for (size_t c = 0; c < m_NumChannels; ++c)
				{
					if (r.width && r.height)
					{
						device_channel<T> p = prototype();
						p.m_First = c * chunks_per_channel();
						p.m_Count = chunks_per_channel();
						w.push_back(p.region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, at * sizeof(T)));
					}
					at += r.out_elems();
				}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("get_regions: too many regions for one call");
			cimg_engine* e = m_Store->engine;
			detail::device_range(e, d_out, per_channel * m_NumChannels * sizeof(T), "get_regions");
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_lock lock(e);
			detail::engine_call(e, cimg_decompress_windows_grouped_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base,
				m_Store->off.data(), m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)),
				static_cast<int32_t>(w.size()), w.data(), d_out, status.data()), "Decoding the regions");
		}
		/// The rectangle of every channel (subsampled) as U = float, half or T, channel c converted with scales[c] and offsets[c] (a span
		/// of one value serves every channel) in the decode launch itself: planes (C, oh, ow) or, with `interleaved`, pixels (oh, ow, C)
		/// written in place by that one launch -- no scratch, no interleave launch, no alignment rule beyond U's own.
		template <typename U>
		void get_region(U* d_out, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, std::span<const float> scales,
			std::span<const float> offsets, bool interleaved = false) const
		{
			const region r{ x, y, width, height, step_x, step_y };
			get_regions(d_out, std::span<const region>(&r, 1), scales, offsets, interleaved);
		}
		/// Many rectangles of every channel, converted as above, in ONE engine call: (N, C, oh, ow) or, with `interleaved`, (N, oh, ow, C)
		/// for N regions of one shape (results back to back in region order otherwise).
		template <typename U>
		void get_regions(U* d_out, std::span<const region> regions, std::span<const float> scales, std::span<const float> offsets, bool interleaved = false) const
		{
			if ((scales.size() != 1 && scales.size() != m_NumChannels) || (offsets.size() != 1 && offsets.size() != m_NumChannels))
				throw std::invalid_argument(detail::text("get_regions: scales and offsets hold one value or one per channel (", m_NumChannels, ")"));
			for (size_t c = 0; c < std::max(scales.size(), offsets.size()); ++c)
				detail::check_typed_result<T, U>(scales[scales.size() == 1 ? 0 : c], offsets[offsets.size() == 1 ? 0 : c], "get_regions");
			const size_t per_channel = prototype().check_regions(regions);
			if (m_NumChannels == 0) return;
			std::vector<cimg_window_typed> w;
			size_t at = 0;                                                       // elements of U before this region
			for (const region& r : regions)
			{
				for (size_t c = 0; c < m_NumChannels && r.width && r.height; ++c)
				{
					device_channel<T> p = prototype();
					p.m_First = c * chunks_per_channel();
					p.m_Count = chunks_per_channel();
					const float sc = scales[scales.size() == 1 ? 0 : c], of = offsets[offsets.size() == 1 ? 0 : c];
					if (interleaved) w.push_back(p.template typed_window<U>(r, (at + c) * sizeof(U), m_NumChannels * sizeof(U), sc, of));
					else w.push_back(p.template typed_window<U>(r, (at + c * r.out_elems()) * sizeof(U), sizeof(U), sc, of));
				}
				at += r.out_elems() * m_NumChannels;
			}
			if (w.empty()) return;
			detail::device_range(m_Store->engine, d_out, per_channel * m_NumChannels * sizeof(U), "get_regions");
			device_channel<T>::run_typed(*m_Store, w, d_out);
		}
		/// Write planes (num_channels x height x width elements in device memory, channel-major) over the rectangle of every channel:
		/// one update call, one repack of the store.  Nothing changes unless the whole call succeeds.
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height)
		{
			prototype().check_region(x, y, width, height);
			if (m_NumChannels == 0 || width == 0 || height == 0) return;
			const size_t plane = width * height * sizeof(T);
			detail::device_range(m_Store->engine, d_src, plane * m_NumChannels, "set_region");
			std::vector<cimg_window> w;
			for (size_t c = 0; c < m_NumChannels; ++c) w.push_back(channel_window(c, x, y, width, height, c * plane));
			m_Store = device_channel<T>::updated_store(*m_Store, prototype().cparams(), m_ChunkSize, w, d_src);
		}

		/// Write every step_y-th row and every step_x-th element of the rectangle of every channel: d_src holds num_channels planes of
		/// ceil(height / step_y) x ceil(width / step_x) elements, channel-major.  A step of 0 throws std::invalid_argument.
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src);
		}
		/// Many rectangles of every channel in ONE engine call and one repack of the store.  The data is region-major, channel-minor,
		/// each piece row-major in its subsampled shape -- the layout get_regions returns.  Later regions win where two overlap.  Every
		/// region is checked before anything runs; an empty list does nothing; nothing changes unless the whole call succeeds.
		void set_regions(std::span<const region> regions, const T* d_src)
		{
			const size_t per_channel = prototype().check_regions(regions);
			if (m_NumChannels == 0) return;
			std::vector<device_channel<T>> per_ch;                    // one prototype a channel, made once
			for (size_t c = 0; c < m_NumChannels; ++c)
			{
				per_ch.push_back(prototype());
				per_ch.back().m_First = c * chunks_per_channel();
				per_ch.back().m_Count = chunks_per_channel();
			}
			std::vector<cimg_window_strided> w;
			size_t at = 0;
			for (const region& r : regions)
				for (size_t c = 0; c < m_NumChannels; ++c)
				{
					if (r.width && r.height) w.push_back(per_ch[c].region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, at * sizeof(T)));
					at += r.out_elems();
				}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("set_regions: too many regions for one call");
			detail::device_range(m_Store->engine, d_src, per_channel * m_NumChannels * sizeof(T), "set_regions");
			m_Store = device_channel<T>::updated_store(*m_Store, prototype().cparams(), m_ChunkSize, w, d_src);
		}

		/// Paint the (subsampled) rectangle of every channel: `values` holds one value for all channels or one a channel.  No source
		/// array exists anywhere; one engine call (cimg_update_windows_masked_device) and one repack of the store.
		void fill_region(std::span<const T> values, size_t x, size_t y, size_t width, size_t height, size_t step_x = 1, size_t step_y = 1)
		{
			const region r{ x, y, width, height, step_x, step_y };
			fill_regions(std::span<const region>(&r, 1), values);
		}
		void fill_regions(std::span<const region> regions, std::span<const T> values) { write_masked(regions, nullptr, values, nullptr, false, "fill_regions"); }
		/// fill_regions through mattes in device memory.  The channels share ONE mask: a byte an element of a region, back to back in
		/// region order, each region row-major in its subsampled shape.
		void fill_regions(std::span<const region> regions, std::span<const T> values, const uint8_t* d_mask)
		{
			if (!d_mask) throw std::invalid_argument("fill_regions: the mask is a null pointer");
			write_masked(regions, nullptr, values, d_mask, false, "fill_regions");
		}
		/// set_region of every channel through one shared matte (h', w'); d_src as set_regions takes it.  (The mask trails the steps.)
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, const uint8_t* d_mask)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src, d_mask);
		}
		/// set_regions through mattes: data region-major, channel-minor; ONE mask for all channels, region-major.
		void set_regions(std::span<const region> regions, const T* d_src, const uint8_t* d_mask)
		{
			if (!d_src || !d_mask) throw std::invalid_argument("set_regions: the source or the mask is a null pointer");
			write_masked(regions, d_src, std::span<const T>(), d_mask, true, "set_regions");
		}
		void write_masked(std::span<const region> regions, const T* d_src, std::span<const T> values, const uint8_t* d_mask, bool has_src, const char* what)
		{
			if (!has_src && values.size() != 1 && values.size() != m_NumChannels)
				throw std::invalid_argument(detail::text(what, ": got ", values.size(), " values for ", m_NumChannels, " channels (one, or one a channel)"));
			const size_t per_channel = prototype().check_regions(regions);
			if (m_NumChannels == 0) return;
			std::vector<device_channel<T>> per_ch;                    // one prototype a channel, made once
			for (size_t c = 0; c < m_NumChannels; ++c)
			{
				per_ch.push_back(prototype());
				per_ch.back().m_First = c * chunks_per_channel();
				per_ch.back().m_Count = chunks_per_channel();
			}
			std::vector<cimg_window_masked> w;
			size_t at = 0, mat = 0;
			for (const region& r : regions)
			{
				for (size_t c = 0; c < m_NumChannels; ++c)
				{
					if (r.width && r.height)
						w.push_back(per_ch[c].masked_window(r, !has_src, has_src ? T{} : values[values.size() == 1 ? 0 : c], d_mask != nullptr, at, mat));
					at += r.out_elems();
				}
				mat += r.out_elems();
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range(detail::text(what, ": too many regions for one call"));
			if (d_src) detail::device_range(m_Store->engine, d_src, per_channel * m_NumChannels * sizeof(T), what);
			if (d_mask) detail::device_range(m_Store->engine, d_mask, per_channel, what);
			m_Store = device_channel<T>::updated_store(*m_Store, prototype().cparams(), m_ChunkSize, w, d_src, d_mask);
		}

		/// Write U = float, half or T over the (subsampled) rectangle of every channel, channel c converted with the inverse of
		/// get_region<U> under scales[c] and offsets[c] (a span of one value serves every channel) in the patch launch itself.  d_src holds
		/// planes (C, oh, ow) or, with `interleaved`, pixels (oh, ow, C): the C windows of a region then read the channel slots of the
		/// same rows -- no permute, no stored-type copy.  One update call, one repack of the store.
		template <typename U>
		void set_region(const U* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, std::span<const float> scales,
			std::span<const float> offsets, bool interleaved = false)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src, scales, offsets, interleaved);
		}
		/// Many rectangles of every channel, converted as above, in ONE engine call and one repack: the source is region-major,
		/// channel-minor (N, C, oh, ow) or, with `interleaved`, (N, oh, ow, C).  Later regions win where two overlap.
		template <typename U>
		void set_regions(std::span<const region> regions, const U* d_src, std::span<const float> scales, std::span<const float> offsets, bool interleaved = false)
		{
			if ((scales.size() != 1 && scales.size() != m_NumChannels) || (offsets.size() != 1 && offsets.size() != m_NumChannels))
				throw std::invalid_argument(detail::text("set_regions: scales and offsets hold one value or one per channel (", m_NumChannels, ")"));
			for (size_t c = 0; c < std::max(scales.size(), offsets.size()); ++c)
				detail::check_typed_source<T, U>(scales[scales.size() == 1 ? 0 : c], offsets[offsets.size() == 1 ? 0 : c], "set_regions");
			const size_t per_channel = prototype().check_regions(regions);
			if (m_NumChannels == 0) return;
			std::vector<device_channel<T>> per_ch;                    // one prototype a channel, made once
			for (size_t c = 0; c < m_NumChannels; ++c)
			{
				per_ch.push_back(prototype());
				per_ch.back().m_First = c * chunks_per_channel();
				per_ch.back().m_Count = chunks_per_channel();
			}
			std::vector<cimg_window_typed> w;
			size_t at = 0;                                                       // elements of U before this region
			for (const region& r : regions)
			{
				for (size_t c = 0; c < m_NumChannels && r.width && r.height; ++c)
				{
					const float sc = scales[scales.size() == 1 ? 0 : c], of = offsets[offsets.size() == 1 ? 0 : c];
					if (interleaved) w.push_back(per_ch[c].template typed_window<U>(r, (at + c) * sizeof(U), m_NumChannels * sizeof(U), sc, of));
					else w.push_back(per_ch[c].template typed_window<U>(r, (at + c * r.out_elems()) * sizeof(U), sizeof(U), sc, of));
				}
				at += r.out_elems() * m_NumChannels;
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("set_regions: too many regions for one call");
			detail::device_range(m_Store->engine, d_src, per_channel * m_NumChannels * sizeof(U), "set_regions");
			m_Store = device_channel<T>::updated_store(*m_Store, prototype().cparams(), m_ChunkSize, w, d_src);
		}

		size_t width() const noexcept { return m_Width; }
		size_t height() const noexcept { return m_Height; }
		size_t num_channels() const noexcept { return m_NumChannels; }
		std::vector<std::string> channelnames() const noexcept { return m_ChannelNames; }
		void channelnames(std::vector<std::string> names)
		{
			if (names.size() != m_NumChannels)
				throw std::invalid_argument(detail::text("Invalid number of arguments received for setting channelnames. Expected vector size to be exactly ",
					m_NumChannels, " but instead got ", names.size()));
			m_ChannelNames = std::move(names);
		}
		enums::codec compression() const noexcept { return m_Codec; }
		std::optional<int> mantissa_bits() const noexcept { return m_MantissaBits; }
		uint8_t compression_level() const noexcept { return m_CompressionLevel; }
		size_t chunk_size() const
		{
			if (m_NumChannels == 0) throw std::runtime_error("Unable to get chunk size from image without channels");
			return m_ChunkSize;
		}
		size_t block_size() const
		{
			if (m_NumChannels == 0) throw std::runtime_error("Unable to get block size from image without channels");
			return m_BlockSize;
		}
		size_t compressed_bytes() const
		{
			size_t n = 0;
			if (m_Store) for (int32_t c : m_Store->cbytes) n += static_cast<size_t>(c);
			return n;
		}
		size_t uncompressed_size() const noexcept { return m_NumChannels * m_Width * m_Height; }
		size_t num_chunks() const noexcept { return m_Store ? m_Store->num_chunks() : 0; }
		size_t device_bytes() const noexcept { return m_Store ? m_Store->bytes : 0; }
		double compression_ratio() const noexcept
		{
			return static_cast<double>(1 + uncompressed_size() * sizeof(T)) / static_cast<double>(1 + compressed_bytes());
		}

	private:
		std::shared_ptr<detail::device_store> m_Store;
		std::vector<std::string> m_ChannelNames{};
		size_t m_NumChannels = 0;
		enums::codec m_Codec = enums::codec::lz4;
		uint8_t m_CompressionLevel = 9;
		std::optional<int> m_MantissaBits = std::nullopt;
		size_t m_BlockSize = s_default_blocksize;
		size_t m_ChunkSize = s_default_chunksize;
		size_t m_Width = 1;
		size_t m_Height = 1;

		void init(enums::codec codec, size_t level, size_t block_size, size_t chunk_size, size_t width, size_t height, size_t nchannels,
			const std::vector<std::string>& names)
		{
			m_Codec = codec;
			m_CompressionLevel = util::ensure_compression_level(level);
			m_BlockSize = block_size;
			m_Width = width; m_Height = height;
			m_NumChannels = nchannels;
			m_ChunkSize = util::align_chunk_to_scanlines_bytes<T>(width, chunk_size);
			util::validate_chunk_size<T>(m_ChunkSize, "device_image");
			if (names.size() != nchannels && !names.empty())
				std::cout << "Invalid number of channel names received, expected " << nchannels << " but instead got " << names.size()
					<< ". Ignoring channel names" << std::endl;
			else
				m_ChannelNames = names;
		}
		size_t chunks_per_channel() const noexcept
		{
			const size_t total = m_Width * m_Height * sizeof(T);
			return (total + m_ChunkSize - 1) / m_ChunkSize;
		}
		/// a store-less channel with this image's geometry and codec (region checks, windows, cparams)
		device_channel<T> prototype() const { return device_channel<T>(m_Codec, m_CompressionLevel, m_BlockSize, m_ChunkSize, m_Width, m_Height, m_MantissaBits); }
		cimg_window channel_window(size_t c, size_t x, size_t y, size_t width, size_t height, size_t out_off) const
		{
			device_channel<T> p = prototype();
			p.m_First = c * chunks_per_channel();
			p.m_Count = chunks_per_channel();
			return p.region_window(x, y, width, height, out_off);
		}
	};
}
