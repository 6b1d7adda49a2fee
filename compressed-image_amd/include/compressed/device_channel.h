// device_channel.h -- compressed::device_channel<T>: one planar image channel kept COMPRESSED IN DEVICE MEMORY.
//
// The counterpart of channel<T> (channel.h) for callers whose pixels live on the GPU: it is built from a device pointer, decodes
// into device pointers, and neither pixels nor chunks cross PCIe.  Names and argument order follow channel<T> where a counterpart
// exists; chunking is the same arithmetic, so chunk boundaries and num_chunks() agree with a channel<T> of the same geometry.
//
// Storage ("store"): ONE device allocation holding the chunks back to back at 64-byte boundaries at their real sizes
// (cimg_compress_batch_device_packed_begin / _fetch), with host-side tables of offsets and sizes.  A device_image<T> keeps one
// store for all its channels; the device_channel handles it hands out share that store and are read-only.
//
// Every address a caller passes is checked with cimg_device_range_check before a kernel sees it (std::invalid_argument).
// Stream ordering: the engine works on its own stream; a caller whose pixels are produced on another stream passes it to
// wait_stream() first.  Results need no counterpart: every call returns after the engine's stream has been synchronised.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "channel.h"

namespace NAMESPACE_COMPRESSED_IMAGE
{
	namespace detail
	{
		/// One device allocation of packed chunks and what the host knows about them.
		struct device_store
		{
			cimg_engine* engine = nullptr;
			std::byte* base = nullptr;
			size_t bytes = 0;                            // the allocation: sum of the 64-byte-rounded chunk sizes
			std::vector<int64_t> off;
			std::vector<int32_t> cbytes, nbytes, blocksize;

			device_store() = default;
			device_store(const device_store&) = delete;
			device_store& operator=(const device_store&) = delete;
			~device_store() { if (base) cimg_device_free(engine, base); }

			size_t num_chunks() const noexcept { return off.size(); }
			/// offsets of chunks of the given sizes packed at 64-byte boundaries; returns the total
			static size_t pack_offsets(const std::vector<int32_t>& sizes, std::vector<int64_t>& out)
			{
				out.resize(sizes.size());
				size_t at = 0;
				for (size_t i = 0; i < sizes.size(); ++i) { out[i] = static_cast<int64_t>(at); at += (static_cast<size_t>(sizes[i]) + 63) & ~size_t(63); }
				return at;
			}
			void allocate(cimg_engine* e, size_t total)
			{
				engine = e;
				bytes = total;
				base = static_cast<std::byte*>(cimg_device_malloc(e, total));
				if (!base) throw std::runtime_error(text("Unable to allocate ", total, " bytes of device memory: ", cimg_last_error(e)));
			}
		};

		struct engine_lock
		{
			cimg_engine* e;
			explicit engine_lock(cimg_engine* e_) : e(e_) { cimg_engine_lock(e); }
			~engine_lock() { cimg_engine_unlock(e); }
			engine_lock(const engine_lock&) = delete;
			engine_lock& operator=(const engine_lock&) = delete;
		};

		inline void device_range(cimg_engine* e, const void* p, size_t bytes, const char* what)
		{
			if (cimg_device_range_check(e, p, bytes) != 0)
				throw std::invalid_argument(text(what, ": ", bytes, " bytes at ", p, " are not device memory of the engine's device (", cimg_last_error(e), ")"));
		}
		inline void engine_call(cimg_engine* e, int rc, const char* what)
		{
			if (rc < 0) throw std::runtime_error(text(what, " failed with error code ", rc, ": ", cimg_last_error(e)));
		}
		/// the block size blosc2 writes into the header of a chunk of `nbytes` bytes compressed with `p`
		inline int32_t header_blocksize(const cimg_cparams& p, int32_t nbytes)
		{
			const int32_t ts = p.typesize > 255 ? 1 : p.typesize;
			if (nbytes < ts) return 1;
			int32_t bs = std::max<int32_t>(p.blocksize, 32);
			bs = std::min(bs, nbytes);
			if (bs > ts) bs = bs / ts * ts;
			return bs;
		}

		/// Compress device-resident pixels -- chunk i is nbytes[i] bytes at d_base + raw_off[i] -- into a new exact-size store.
		inline std::shared_ptr<device_store> compress_to_store(const cimg_cparams& cp, const void* d_base, const std::vector<int64_t>& raw_off,
			const std::vector<int32_t>& nbytes, size_t nominal_chunk_bytes)
		{
			cimg_engine* e = blosc2::batch::engine();
			auto store = std::make_shared<device_store>();
			const size_t n = nbytes.size();
			store->nbytes = nbytes;
			store->cbytes.assign(n, 0);
			store->blocksize.resize(n);
			for (size_t i = 0; i < n; ++i) store->blocksize[i] = header_blocksize(cp, nbytes[i]);
			std::vector<int32_t> destsize(n, static_cast<int32_t>(blosc2::min_compressed_size(nominal_chunk_bytes)));
			// _begin and _fetch belong together (the staging area is the engine's): its lock is held across the pair
			engine_lock pair_lock(e);
			engine_call(e, cimg_compress_batch_device_packed_begin(e, &cp, static_cast<int32_t>(n), d_base, raw_off.data(), nbytes.data(), destsize.data(),
				store->cbytes.data()), "Compressing device-resident chunks");
			for (size_t i = 0; i < n; ++i)
				if (store->cbytes[i] <= 0) throw std::runtime_error(text("Unable to compress chunk ", i, " (code ", store->cbytes[i], ")"));
			store->allocate(e, device_store::pack_offsets(store->cbytes, store->off));
			engine_call(e, cimg_compress_batch_device_packed_fetch(e, static_cast<int32_t>(n), store->base, store->off.data()), "Packing the compressed chunks");
			return store;
		}
	}

	namespace detail
	{
		/// The compressed chunks of a host channel, one byte vector each, appended to `out`.  Fill-value chunks are materialised the
		/// way the host table exports them (to_schunk: lz4, level 9); a short last fill-value chunk, which that export writes at the
		/// nominal chunk size, is compressed here at its real size instead.
		template <typename T>
		void host_chunks(const channel<T>& host, std::vector<std::vector<std::byte>>& out)
		{
			auto super = std::visit([](auto& table) { return table.to_schunk(); }, const_cast<blosc2::schunk_var<T>&>(host.chunks()));
			for (size_t i = 0; i < static_cast<size_t>(super->nchunks); ++i)
			{
				int32_t nb = 0, cb = 0, bs = 0;
				if (blosc2_cbuffer_sizes(super->data[i], &nb, &cb, &bs) < 0 || cb < 32)
					throw std::runtime_error(text("chunk ", i, " of the host channel has no valid header"));
				if (static_cast<size_t>(nb) == host.chunk_size(i))
				{
					const auto* c = reinterpret_cast<const std::byte*>(super->data[i]);
					out.emplace_back(c, c + cb);
					continue;
				}
				std::vector<T> pixels(host.chunk_elems(i));
				host.get_chunk(std::span<T>(pixels), i);
				auto ctx = blosc2::create_compression_context<T>(1, enums::codec::lz4, 9, host.block_size());
				std::vector<std::byte> scratch(blosc2::min_compressed_size(host.chunk_size()));
				scratch.resize(blosc2::compress<T>(ctx.get(), std::span<const T>(pixels), std::span<std::byte>(scratch)));
				out.push_back(std::move(scratch));
			}
		}
		/// Chunks in host memory -> a new store (one upload).
		inline std::shared_ptr<device_store> upload_store(const std::vector<std::vector<std::byte>>& chunks)
		{
			cimg_engine* e = blosc2::batch::engine();
			auto store = std::make_shared<device_store>();
			const size_t n = chunks.size();
			store->cbytes.resize(n); store->nbytes.resize(n); store->blocksize.resize(n);
			for (size_t i = 0; i < n; ++i)
			{
				int32_t cb = 0;
				if (chunks[i].size() < 32 || blosc2_cbuffer_sizes(chunks[i].data(), &store->nbytes[i], &cb, &store->blocksize[i]) < 0 || static_cast<size_t>(cb) != chunks[i].size())
					throw std::runtime_error(text("chunk ", i, " has no valid header"));
				store->cbytes[i] = cb;
			}
			const size_t total = device_store::pack_offsets(store->cbytes, store->off);
			std::vector<std::byte> staged(total);
			for (size_t i = 0; i < n; ++i) std::memcpy(staged.data() + store->off[i], chunks[i].data(), chunks[i].size());
			store->allocate(e, total);
			engine_call(e, cimg_memcpy_h2d(e, store->base, staged.data(), total), "Uploading the compressed chunks");
			return store;
		}
	}

	namespace detail
	{
		/// The CIMG_T_* code of an element type (typed region reads).
		template <typename U> constexpr int32_t typed_code()
		{
			if constexpr (std::is_same_v<U, uint8_t>) return CIMG_T_U8;
			else if constexpr (std::is_same_v<U, int8_t>) return CIMG_T_I8;
			else if constexpr (std::is_same_v<U, uint16_t>) return CIMG_T_U16;
			else if constexpr (std::is_same_v<U, int16_t>) return CIMG_T_I16;
			else if constexpr (std::is_same_v<U, uint32_t>) return CIMG_T_U32;
			else if constexpr (std::is_same_v<U, int32_t>) return CIMG_T_I32;
			else if constexpr (std::is_same_v<U, half>) return CIMG_T_F16;
			else if constexpr (std::is_same_v<U, float>) return CIMG_T_F32;
			else if constexpr (std::is_same_v<U, double>) return CIMG_T_F64;
			else return -1;
		}
		/// What a typed read may produce from pixels stored as T: float, half, or T itself with scale 1 and offset 0.
		template <typename T, typename U> void check_typed_result(float scale, float offset, const char* what)
		{
			static_assert(std::is_same_v<U, float> || std::is_same_v<U, half> || std::is_same_v<U, T>,
				"a typed region read produces float, half or the stored type");
			static_assert(typed_code<T>() >= 0, "typed region reads: unsupported element type");
			if constexpr (!std::is_same_v<U, float> && !std::is_same_v<U, half>)
				if (scale != 1.0f || offset != 0.0f)
					throw std::invalid_argument(text(what, ": a result of the stored type takes scale 1 and offset 0 (float and half results are converted)"));
		}
		/// What a typed write may take for pixels stored as T: float, half, or T itself with scale 1 and offset 0.  The scale is finite
		/// and not 0, the offset finite; float64 pixels are written from float64 only.
		template <typename T, typename U> void check_typed_source(float scale, float offset, const char* what)
		{
			static_assert(std::is_same_v<U, float> || std::is_same_v<U, half> || std::is_same_v<U, T>,
				"a typed region write takes float, half or the stored type");
			static_assert(typed_code<T>() >= 0, "typed region writes: unsupported element type");
			if (!std::isfinite(scale) || !std::isfinite(offset) || scale == 0.0f)
				throw std::invalid_argument(text(what, ": scale must be finite and not 0, offset must be finite"));
			if constexpr (!std::is_same_v<U, float> && !std::is_same_v<U, half>)
				if (scale != 1.0f || offset != 0.0f)
					throw std::invalid_argument(text(what, ": a source of the stored type takes scale 1 and offset 0 (float and half sources are converted)"));
			if constexpr (std::is_same_v<T, double> && !std::is_same_v<U, double>)
				throw std::invalid_argument(text(what, ": float64 pixels are written from float64 only"));
		}
	}

	template <typename T> struct device_image;

	template <typename T>
	struct device_channel
	{
		device_channel(device_channel&&) noexcept = default;
		device_channel& operator=(device_channel&&) noexcept = default;
		device_channel(const device_channel&) = delete;
		device_channel& operator=(const device_channel&) = delete;

		/// Compress `d_data` (width * height elements in device memory).  Chunks are aligned to whole scanlines, as channel<T>'s.
		/// mantissa_bits: as channel<T>'s (the caller's pixels are not modified; set_region truncates what it writes).
		device_channel(const T* d_data, size_t width, size_t height,
			enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
			: m_Codec(compression_codec), m_CompressionLevel(util::ensure_compression_level(compression_level)), m_MantissaBits(mantissa_bits), m_BlockSize(block_size),
			  m_ChunkSize(util::align_chunk_to_scanlines_bytes<T>(width, chunk_size)), m_Width(width), m_Height(height)
		{
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			util::validate_chunk_size<T>(m_ChunkSize, "device_channel");
			cimg_engine* e = blosc2::batch::engine();
			const size_t total = width * height * sizeof(T);
			detail::device_range(e, d_data, total, "device_channel");
			std::vector<int64_t> raw_off;
			std::vector<int32_t> nbytes;
			for (size_t off = 0; off < total; off += m_ChunkSize)
			{
				raw_off.push_back(static_cast<int64_t>(off));
				nbytes.push_back(static_cast<int32_t>(std::min(m_ChunkSize, total - off)));
			}
			m_Store = detail::compress_to_store(cparams(), d_data, raw_off, nbytes, m_ChunkSize);
			m_First = 0;
			m_Count = nbytes.size();
		}

		/// The compressed chunks of a host channel, moved over PCIe as they are (fill-value chunks are materialised).
		static device_channel from_channel(const channel<T>& host)
		{
			device_channel out(host.compression(), host.compression_level(), host.block_size(), host.chunk_size(), host.width(), host.height(), host.mantissa_bits());
			std::vector<std::vector<std::byte>> chunks;
			detail::host_chunks(host, chunks);
			const size_t n = chunks.size();
			auto store = detail::upload_store(chunks);
			out.m_Store = std::move(store);
			out.m_First = 0;
			out.m_Count = n;
			return out;
		}
		/// A channel whose every element is `value`, at 64 bytes of device memory a chunk: the store is built on the host from blosc2
		/// special-value chunks -- a header and the value; special-zero chunks where the value is all zero bytes -- and uploaded once.
		/// Nothing is launched and no pixel buffer exists anywhere.  Everything a device_channel does works on it; set_region makes the
		/// chunks it touches regular and leaves the others as they are.  mantissa_bits: the value is stored truncated.
		static device_channel full(T value, size_t width, size_t height, enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
		{
			blosc2::ensure_mantissa_bits<T>(mantissa_bits);
			if (width == 0 || height == 0) throw std::invalid_argument("device_channel::full: width and height must be at least 1");
			const size_t chunk_bytes = util::align_chunk_to_scanlines_bytes<T>(width, chunk_size);
			util::validate_chunk_size<T>(chunk_bytes, "device_channel");
			device_channel out(compression_codec, util::ensure_compression_level(compression_level), block_size, chunk_bytes, width, height, mantissa_bits);
			const blosc2_cparams p = blosc2::create_blosc2_cparams<T>(1, compression_codec, out.m_CompressionLevel, block_size, mantissa_bits);
			unsigned char raw[sizeof(T)];
			std::memcpy(raw, &value, sizeof(T));
			const bool zero = std::all_of(raw, raw + sizeof(T), [](unsigned char b) { return b == 0; });
			const size_t total = width * height * sizeof(T);
			std::vector<std::vector<std::byte>> chunks;
			for (size_t off = 0; off < total; off += chunk_bytes)
			{
				const int32_t nbytes = static_cast<int32_t>(std::min(chunk_bytes, total - off));
				std::vector<std::byte> c(BLOSC_EXTENDED_HEADER_LENGTH + sizeof(T));
				const int rc = zero ? blosc2_chunk_zeros(p, nbytes, c.data(), static_cast<int32_t>(c.size()))
					: blosc2_chunk_repeatval(p, nbytes, c.data(), static_cast<int32_t>(c.size()), raw);
				if (rc < 0) throw std::runtime_error(detail::text("Unable to write the fill chunk ", chunks.size(), ", error code ", rc));
				c.resize(static_cast<size_t>(rc));
				chunks.push_back(std::move(c));
			}
			out.m_Count = chunks.size();
			out.m_Store = detail::upload_store(chunks);
			out.m_First = 0;
			return out;
		}
		static device_channel zeros(size_t width, size_t height, enums::codec compression_codec = enums::codec::lz4, uint8_t compression_level = 9,
			size_t block_size = s_default_blocksize, size_t chunk_size = s_default_chunksize, std::optional<int> mantissa_bits = std::nullopt)
		{
			return full(T{}, width, height, compression_codec, compression_level, block_size, chunk_size, mantissa_bits);
		}
		/// full / zeros with the geometry and the codec parameters of `other`
		static device_channel full_like(const device_channel& other, T value)
		{
			return full(value, other.width(), other.height(), other.compression(), other.compression_level(), other.block_size(), other.chunk_size(),
				other.mantissa_bits());
		}
		static device_channel zeros_like(const device_channel& other) { return full_like(other, T{}); }

		/// The same chunks back in host memory, as a channel<T>.
		channel<T> to_channel() const
		{
			require();
			cimg_engine* e = m_Store->engine;
			const size_t a = static_cast<size_t>(m_Store->off[m_First]);
			const size_t last = m_First + m_Count - 1;
			const size_t b = static_cast<size_t>(m_Store->off[last]) + static_cast<size_t>(m_Store->cbytes[last]);
			std::vector<std::byte> staged(b - a);
			detail::engine_call(e, cimg_memcpy_d2h(e, staged.data(), m_Store->base + a, b - a), "Downloading the compressed chunks");
			blosc2::schunk<T> table(m_BlockSize, m_ChunkSize);
			for (size_t i = m_First; i <= last; ++i)
			{
				const std::byte* c = staged.data() + (static_cast<size_t>(m_Store->off[i]) - a);
				table.append_chunk(std::vector<std::byte>(c, c + m_Store->cbytes[i]));
			}
			return channel<T>(blosc2::schunk_var<T>(std::move(table)), m_Width, m_Height, m_Codec, m_CompressionLevel, m_MantissaBits);
		}

		/// The engine's stream waits for what `stream` (a hipStream_t; nullptr: the null stream) holds now.
		static void wait_stream(void* stream)
		{
			cimg_engine* e = blosc2::batch::engine();
			detail::engine_call(e, cimg_engine_wait_stream(e, stream), "Waiting for the caller's stream");
		}

		size_t width() const noexcept { return m_Width; }
		size_t height() const noexcept { return m_Height; }
		enums::codec compression() const noexcept { return m_Codec; }
		uint8_t compression_level() const noexcept { return m_CompressionLevel; }
		std::optional<int> mantissa_bits() const noexcept { return m_MantissaBits; }
		size_t compressed_bytes() const
		{
			require();
			size_t n = 0;
			for (size_t i = m_First; i < m_First + m_Count; ++i) n += static_cast<size_t>(m_Store->cbytes[i]);
			return n;
		}
		/// bytes of one compressed chunk (it occupies this rounded up to 64 in the store)
		size_t compressed_bytes(size_t chunk_index) const
		{
			(void)chunk_size(chunk_index);
			return static_cast<size_t>(m_Store->cbytes[m_First + chunk_index]);
		}
		size_t uncompressed_size() const noexcept { return m_Width * m_Height; }
		size_t num_chunks() const noexcept { return m_Count; }
		size_t block_size() const noexcept { return m_BlockSize; }
		size_t chunk_size() const noexcept { return m_ChunkSize; }
		size_t chunk_elems() const noexcept { return m_ChunkSize / sizeof(T); }
		size_t chunk_size(size_t chunk_index) const
		{
			if (chunk_index >= m_Count)
				throw std::out_of_range(detail::text("Cannot access index ", chunk_index, " in schunk. Total amount of chunks is ", m_Count));
			return static_cast<size_t>(m_Store->nbytes[m_First + chunk_index]);
		}
		size_t chunk_elems(size_t chunk_index) const { return chunk_size(chunk_index) / sizeof(T); }
		/// Bytes of device memory the store occupies (the whole image's, for a handle handed out by a device_image).
		size_t device_bytes() const { require(); return m_Store->bytes; }
		/// true for a handle handed out by device_image::channel(): edits go through the image
		bool read_only() const noexcept { return m_ReadOnly; }

		/// Decode into device memory (uncompressed_size() elements).
		void decompress_into(T* d_out) const
		{
			require();
			cimg_engine* e = m_Store->engine;
			detail::device_range(e, d_out, uncompressed_size() * sizeof(T), "decompress_into");
			std::vector<int64_t> raw_off(m_Count);
			int64_t at = 0;
			for (size_t i = 0; i < m_Count; ++i) { raw_off[i] = at; at += m_Store->nbytes[m_First + i]; }
			std::vector<int32_t> status(m_Count, 0);
			detail::engine_call(e, cimg_decompress_batch_device_sized(e, static_cast<int32_t>(m_Count), m_Store->base, m_Store->off.data() + m_First,
				m_Store->cbytes.data() + m_First, m_Store->nbytes.data() + m_First, m_Store->blocksize.data() + m_First, d_out, raw_off.data(),
				status.data()), "Decompressing the channel");
		}
		/// The rectangle [x, x + width) x [y, y + height), row-major (width elements a row), into device memory.  Only the blocks
		/// the rectangle meets are decoded.
		void get_region(T* d_out, size_t x, size_t y, size_t width, size_t height) const
		{
			check_region(x, y, width, height);
			require();
			if (width == 0 || height == 0) return;
			cimg_engine* e = m_Store->engine;
			detail::device_range(e, d_out, width * height * sizeof(T), "get_region");
			const cimg_window w = region_window(x, y, width, height, 0);
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_call(e, cimg_decompress_windows_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base, m_Store->off.data(),
				m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)), 1, &w, d_out, status.data()),
				"Decoding the region");
		}
		/// The rectangle subsampled into device memory: ceil(height / step_y) rows of ceil(width / step_x) elements, every step_y-th
		/// row and every step_x-th element of it.  Only the blocks that hold a sampled element are decoded.
		void get_region(T* d_out, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y) const
		{
			check_region(x, y, width, height);
			check_steps(step_x, step_y);
			require();
			if (width == 0 || height == 0) return;
			cimg_engine* e = m_Store->engine;
			const cimg_window_strided w = region_window(x, y, width, height, step_x, step_y, 0);
			detail::device_range(e, d_out, static_cast<size_t>(w.width) * static_cast<size_t>(w.height) * sizeof(T), "get_region");
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_call(e, cimg_decompress_windows_strided_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base,
				m_Store->off.data(), m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)), 1, &w,
				d_out, status.data()), "Decoding the subsampled region");
		}
		/// Many rectangles into device memory in ONE engine call that decodes every block once, however many of the regions meet it.
		/// The results lie back to back in region order, each row-major with its subsampled shape.  Every region is checked before
		/// anything runs; an empty list does nothing.
		void get_regions(T* d_out, std::span<const region> regions) const
		{
			const size_t total = check_regions(regions);
			require();
			std::vector<cimg_window_strided> w;
			size_t at = 0;
			for (const region& r : regions)
			{
				if (r.width && r.height) w.push_back(region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, at * sizeof(T)));
				at += r.out_elems();
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("get_regions: too many regions for one call");
			cimg_engine* e = m_Store->engine;
			detail::device_range(e, d_out, total * sizeof(T), "get_regions");
			std::vector<int32_t> status(m_Store->num_chunks(), 0);
			detail::engine_call(e, cimg_decompress_windows_grouped_device(e, static_cast<int32_t>(m_Store->num_chunks()), m_Store->base,
				m_Store->off.data(), m_Store->cbytes.data(), m_Store->nbytes.data(), m_Store->blocksize.data(), static_cast<int32_t>(sizeof(T)),
				static_cast<int32_t>(w.size()), w.data(), d_out, status.data()), "Decoding the regions");
		}
		/// The rectangle (subsampled) as U = float, half or T: y = fl32(fl32((float)v * scale) + offset), rounded once more for half --
		/// numpy's (v.astype(float32) * float32(scale) + float32(offset)).astype(U), bit for bit -- converted in the decode launch
		/// itself.  U = T takes scale 1 and offset 0 and copies the elements.
		template <typename U>
		void get_region(U* d_out, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, float scale, float offset) const
		{
			const region r{ x, y, width, height, step_x, step_y };
			get_regions(d_out, std::span<const region>(&r, 1), scale, offset);
		}
		/// get_regions with every element converted as above: one engine call (cimg_decompress_windows_typed_device), each block decoded once.
		template <typename U>
		void get_regions(U* d_out, std::span<const region> regions, float scale, float offset) const
		{
			detail::check_typed_result<T, U>(scale, offset, "get_regions");
			const size_t total = check_regions(regions);
			require();
			std::vector<cimg_window_typed> w;
			size_t at = 0;
			for (const region& r : regions)
			{
				if (r.width && r.height) w.push_back(typed_window<U>(r, at * sizeof(U), sizeof(U), scale, offset));
				at += r.out_elems();
			}
			if (w.empty()) return;
			detail::device_range(m_Store->engine, d_out, total * sizeof(U), "get_regions");
			run_typed(*m_Store, w, d_out);
		}
		/// A region as a typed window over this channel's chunks: element c of row r at out_off + (r * out_width + c) * elem_pitch.
		template <typename U>
		cimg_window_typed typed_window(const region& r, size_t out_off, size_t elem_pitch, float scale, float offset) const
		{
			const cimg_window_strided s = region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, out_off);
			cimg_window_typed w{};
			w.chunk_first = s.chunk_first; w.chunk_count = s.chunk_count;
			w.origin = s.origin; w.row_pitch = s.row_pitch; w.col_pitch = s.col_pitch;
			w.width = s.width; w.height = s.height;
			w.out_off = s.out_off;
			w.elem_pitch = static_cast<int64_t>(elem_pitch);
			w.out_pitch = static_cast<int64_t>(static_cast<size_t>(s.width) * elem_pitch);
			w.src_type = detail::typed_code<T>();
			w.out_type = detail::typed_code<U>();
			w.scale = scale; w.offset = offset;
			return w;
		}
		/// One typed windows call over a store.  (A member template's body: only code that asks for typed reads refers to the entry point.)
		template <typename Window = cimg_window_typed>
		static void run_typed(const detail::device_store& store, const std::vector<Window>& w, void* d_out)
		{
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("get_regions: too many regions for one call");
			cimg_engine* e = store.engine;
			std::vector<int32_t> status(store.num_chunks(), 0);
			detail::engine_lock lock(e);
			detail::engine_call(e, cimg_decompress_windows_typed_device(e, static_cast<int32_t>(store.num_chunks()), store.base, store.off.data(),
				store.cbytes.data(), store.nbytes.data(), store.blocksize.data(), static_cast<int32_t>(sizeof(T)), static_cast<int32_t>(w.size()), w.data(),
				d_out, status.data()), "Decoding the typed regions");
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
		/// Write `d_src` (width * height elements in device memory, row-major) over the rectangle.  Only the blocks it meets are decoded
		/// and re-encoded; the store is then repacked into a new exact-size allocation (untouched chunks from the old one).
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height)
		{
			if (m_ReadOnly) throw std::runtime_error("set_region: this device_channel shares the store of a device_image and is read-only; use device_image::set_region");
			check_region(x, y, width, height);
			require();
			if (width == 0 || height == 0) return;
			detail::device_range(m_Store->engine, d_src, width * height * sizeof(T), "set_region");
			const cimg_window w = region_window(x, y, width, height, 0);
			m_Store = updated_store(*m_Store, cparams(), m_ChunkSize, std::vector<cimg_window>{ w }, d_src);
		}

		/// Write `d_src` over every step_y-th row and every step_x-th element of the rectangle: d_src holds ceil(height / step_y) rows of
		/// ceil(width / step_x) elements, the layout get_region with the same steps returns.  Only the blocks that hold a written
		/// element are decoded and re-encoded.  A step of 0 throws std::invalid_argument.
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src);
		}
		/// Many rectangles in ONE engine call and one repack of the store.  The data lies back to back in region order, each region
		/// row-major in its subsampled shape -- the layout get_regions returns.  Later regions win where two overlap.  Every region is
		/// checked before anything runs; an empty list does nothing; nothing changes unless the whole call succeeds.
		void set_regions(std::span<const region> regions, const T* d_src)
		{
			if (m_ReadOnly) throw std::runtime_error("set_regions: this device_channel shares the store of a device_image and is read-only; use device_image::set_regions");
			const size_t total = check_regions(regions);
			require();
			std::vector<cimg_window_strided> w;
			size_t at = 0;
			for (const region& r : regions)
			{
				if (r.width && r.height) w.push_back(region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, at * sizeof(T)));
				at += r.out_elems();
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("set_regions: too many regions for one call");
			detail::device_range(m_Store->engine, d_src, total * sizeof(T), "set_regions");
			m_Store = updated_store(*m_Store, cparams(), m_ChunkSize, w, d_src);
		}

		/// Write `d_src` -- U = float, half or T, ceil(height / step_y) rows of ceil(width / step_x) elements -- over the (subsampled)
		/// rectangle, each element converted in the patch launch itself: the inverse of get_region<U> with the same scale and offset,
		/// t = fl32(fl32((float)y - offset) / scale), then rint saturated to T's range (NaN gives 0) for integer pixels, t rounded once
		/// for half pixels, t for float pixels -- numpy's answer bit for bit.  U = T takes scale 1 and offset 0 and copies the elements.
		template <typename U>
		void set_region(const U* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, float scale, float offset)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src, scale, offset);
		}
		/// set_regions with every element converted as above: ONE engine call (cimg_update_windows_typed_device) and one repack.
		template <typename U>
		void set_regions(std::span<const region> regions, const U* d_src, float scale, float offset)
		{
			if (m_ReadOnly) throw std::runtime_error("set_regions: this device_channel shares the store of a device_image and is read-only; use device_image::set_regions");
			detail::check_typed_source<T, U>(scale, offset, "set_regions");
			const size_t total = check_regions(regions);
			require();
			std::vector<cimg_window_typed> w;
			size_t at = 0;
			for (const region& r : regions)
			{
				if (r.width && r.height) w.push_back(typed_window<U>(r, at * sizeof(U), sizeof(U), scale, offset));
				at += r.out_elems();
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("set_regions: too many regions for one call");
			detail::device_range(m_Store->engine, d_src, total * sizeof(U), "set_regions");
			m_Store = updated_store(*m_Store, cparams(), m_ChunkSize, w, d_src);
		}

		/// Paint the (subsampled) rectangle with one value: np.copyto(view, value) without a source array.  Only the blocks that hold a
		/// written element are re-encoded, and a block the rectangle covers whole (steps of 1) is not even decoded; nothing but the
		/// window table reaches the device.  With trunc-prec storage the value is truncated like any written pixel.
		void fill_region(T value, size_t x, size_t y, size_t width, size_t height, size_t step_x = 1, size_t step_y = 1)
		{
			const region r{ x, y, width, height, step_x, step_y };
			fill_regions(std::span<const region>(&r, 1), std::span<const T>(&value, 1));
		}
		/// Many rectangles painted in ONE engine call (cimg_update_windows_masked_device) and one repack: `values` holds one value for
		/// all regions or one per region.  Later regions win where two overlap.
		void fill_regions(std::span<const region> regions, std::span<const T> values) { write_masked(regions, nullptr, values, nullptr, "fill_regions"); }
		/// fill_regions through a matte: d_mask holds one uint8 an element in device memory, back to back in region order, each
		/// region row-major in its subsampled shape; an element is painted where its mask byte is not 0 and keeps its value elsewhere.
		void fill_regions(std::span<const region> regions, std::span<const T> values, const uint8_t* d_mask)
		{
			if (!d_mask) throw std::invalid_argument("fill_regions: the mask is a null pointer");
			write_masked(regions, nullptr, values, d_mask, "fill_regions");
		}
		/// set_region through a matte: np.copyto(view, src, where=mask).  d_src and d_mask (uint8, any nonzero byte writes) have the
		/// subsampled shape, in device memory.  One engine call, every touched block decoded once.
		/// (The mask trails the steps, which have no defaults here: a literal 0 must never be taken for a null mask.)
		void set_region(const T* d_src, size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, const uint8_t* d_mask)
		{
			const region r{ x, y, width, height, step_x, step_y };
			set_regions(std::span<const region>(&r, 1), d_src, d_mask);
		}
		/// set_regions through mattes: data and masks lie back to back in region order, both in the subsampled shapes.
		void set_regions(std::span<const region> regions, const T* d_src, const uint8_t* d_mask)
		{
			if (!d_src || !d_mask) throw std::invalid_argument("set_regions: the source or the mask is a null pointer");
			write_masked(regions, d_src, std::span<const T>(), d_mask, "set_regions");
		}

		void check_region(size_t x, size_t y, size_t width, size_t height) const
		{
			if (x > m_Width || y > m_Height || width > m_Width - x || height > m_Height - y)
				throw std::out_of_range(detail::text("Region (x ", x, ", y ", y, ", width ", width, ", height ", height, ") is out of bounds for a channel of ",
					m_Width, " x ", m_Height));
		}
		static void check_steps(size_t step_x, size_t step_y)
		{
			if (step_x == 0 || step_y == 0) throw std::invalid_argument("get_region: step_x and step_y must be at least 1");
		}
		/// The codec parameters the chunks were made with (what set_region hands the engine).
		cimg_cparams cparams() const
		{
			auto ctx = blosc2::create_compression_context<T>(1, m_Codec, m_CompressionLevel, m_BlockSize, m_MantissaBits);
			cimg_cparams out{};
			const int rc = cimg_context_cparams(ctx.get(), &out);
			if (rc < 0) throw std::runtime_error(detail::text("Unable to read the compression parameters, error code ", rc));
			return out;
		}
		/// The rectangle as a window over this channel's chunks of the store; `out_off` is where its first element goes / comes from.
		cimg_window region_window(size_t x, size_t y, size_t width, size_t height, size_t out_off) const
		{
			cimg_window w{};
			w.chunk_first = static_cast<int32_t>(m_First);
			w.chunk_count = static_cast<int32_t>(m_Count);
			w.origin = static_cast<int64_t>(y * m_Width + x);
			w.row_pitch = static_cast<int64_t>(m_Width);
			w.width = static_cast<int32_t>(width);
			w.height = static_cast<int32_t>(height);
			w.out_off = static_cast<int64_t>(out_off);
			w.out_pitch = static_cast<int64_t>(width * sizeof(T));
			return w;
		}

		/// The rectangle subsampled, as a strided window: ceil(height / step_y) rows of ceil(width / step_x) elements, dense in the output.
		cimg_window_strided region_window(size_t x, size_t y, size_t width, size_t height, size_t step_x, size_t step_y, size_t out_off) const
		{
			cimg_window_strided w{};
			w.chunk_first = static_cast<int32_t>(m_First);
			w.chunk_count = static_cast<int32_t>(m_Count);
			w.origin = static_cast<int64_t>(y * m_Width + x);
			w.row_pitch = static_cast<int64_t>(step_y * m_Width);
			w.col_pitch = static_cast<int64_t>(step_x);
			w.width = static_cast<int32_t>((width + step_x - 1) / step_x);
			w.height = static_cast<int32_t>((height + step_y - 1) / step_y);
			w.out_off = static_cast<int64_t>(out_off);
			w.out_pitch = static_cast<int64_t>(static_cast<size_t>(w.width) * sizeof(T));
			return w;
		}

		/// The region as a masked window: a constant (d_src null: `value`) or source elements at out_off, under the mask bytes at mask_off
		/// when there is a mask.
		cimg_window_masked masked_window(const region& r, bool constant, T value, bool masked, size_t out_elems_before, size_t mask_elems_before) const
		{
			const cimg_window_strided s = region_window(r.x, r.y, r.width, r.height, r.step_x, r.step_y, out_elems_before * sizeof(T));
			cimg_window_masked w{};
			w.chunk_first = s.chunk_first; w.chunk_count = s.chunk_count;
			w.origin = s.origin; w.row_pitch = s.row_pitch; w.col_pitch = s.col_pitch;
			w.width = s.width; w.height = s.height;
			if (constant)
			{
				static_assert(sizeof(T) <= sizeof(w.value), "a constant has at most 8 bytes");
				w.flags |= CIMG_WM_CONST;
				std::memcpy(w.value, &value, sizeof(T));
			}
			else { w.out_off = s.out_off; w.out_pitch = s.out_pitch; }
			if (masked)
			{
				w.flags |= CIMG_WM_MASK;
				w.mask_off = static_cast<int64_t>(mask_elems_before);
				w.mask_pitch = s.width;
			}
			return w;
		}
		/// fill_regions and the masked set_regions: ONE engine call (cimg_update_windows_masked_device) and one repack.  Every region is
		/// checked before anything runs; nothing changes unless the whole call succeeds.
		void write_masked(std::span<const region> regions, const T* d_src, std::span<const T> values, const uint8_t* d_mask, const char* what)
		{
			if (m_ReadOnly) throw std::runtime_error(detail::text(what, ": this device_channel shares the store of a device_image and is read-only; use the device_image's"));
			const bool constant = d_src == nullptr;
			if (constant && values.size() != 1 && values.size() != regions.size())
				throw std::invalid_argument(detail::text(what, ": got ", values.size(), " values for ", regions.size(), " regions (one, or one per region)"));
			const size_t total = check_regions(regions);
			require();
			std::vector<cimg_window_masked> w;
			size_t at = 0;
			for (size_t k = 0; k < regions.size(); ++k)
			{
				const region& r = regions[k];
				if (r.width && r.height) w.push_back(masked_window(r, constant, constant ? values[values.size() == 1 ? 0 : k] : T{}, d_mask != nullptr, at, at));
				at += r.out_elems();
			}
			if (w.empty()) return;
			if (w.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range(detail::text(what, ": too many regions for one call"));
			if (d_src) detail::device_range(m_Store->engine, d_src, total * sizeof(T), what);
			if (d_mask) detail::device_range(m_Store->engine, d_mask, total, what);
			m_Store = updated_store(*m_Store, cparams(), m_ChunkSize, w, d_src, d_mask);
		}

		/// Apply window writes to a store: the update's output goes to a scratch allocation, then ONE pack launch gathers the new
		/// store -- untouched chunks from the old one, touched ones from the scratch.  The old store is left as it was.
		/// (Window: cimg_window through cimg_update_windows_device, cimg_window_strided through cimg_update_windows_strided_device,
		/// cimg_window_typed through cimg_update_windows_typed_device, cimg_window_masked through cimg_update_windows_masked_device with
		/// d_mask beside d_src -- each instantiation refers to its own entry point only)
		template <typename Window>
		static std::shared_ptr<detail::device_store> updated_store(const detail::device_store& old, const cimg_cparams& cp, size_t nominal_chunk_bytes,
			const std::vector<Window>& windows, const void* d_src, const void* d_mask = nullptr)
		{
			constexpr bool typed = std::is_same_v<Window, cimg_window_typed>;
			constexpr bool masked = std::is_same_v<Window, cimg_window_masked>;
			constexpr bool strided = std::is_same_v<Window, cimg_window_strided> || typed || masked;
			cimg_engine* e = old.engine;
			const size_t n = old.num_chunks();
			const int32_t dest = static_cast<int32_t>(blosc2::min_compressed_size(nominal_chunk_bytes));
			// room only for the chunks a window can meet: those of the windows' chunk ranges that their rows reach
			std::vector<int32_t> destsize(n, dest), new_cbytes(n, 0), status(n, 0);
			std::vector<int64_t> new_off(n, 0);
			std::vector<char> may(n, 0);
			for (const auto& w : windows)
			{
				if (w.width <= 0 || w.height <= 0) continue;
				const int64_t lo = w.origin * static_cast<int64_t>(sizeof(T));
				int64_t span = w.width;
				if constexpr (strided) span = static_cast<int64_t>(w.width - 1) * w.col_pitch + 1;
				const int64_t hi = (w.origin + (w.height - 1) * w.row_pitch + span) * static_cast<int64_t>(sizeof(T));
				int64_t at = 0;
				for (int32_t k = w.chunk_first; k < w.chunk_first + w.chunk_count; ++k)
				{
					if (at < hi && at + old.nbytes[static_cast<size_t>(k)] > lo) may[static_cast<size_t>(k)] = 1;
					at += old.nbytes[static_cast<size_t>(k)];
				}
			}
			size_t scratch_bytes = 0;
			for (size_t i = 0; i < n; ++i)
				if (may[i]) { new_off[i] = static_cast<int64_t>(scratch_bytes); scratch_bytes += (static_cast<size_t>(dest) + 63) & ~size_t(63); }
			detail::device_store scratch;
			scratch.allocate(e, scratch_bytes + 64);
			detail::engine_lock lock(e);
			if constexpr (masked)
				detail::engine_call(e, cimg_update_windows_masked_device(e, &cp, static_cast<int32_t>(n), old.base, old.off.data(), old.cbytes.data(),
					old.nbytes.data(), old.blocksize.data(), destsize.data(), static_cast<int32_t>(windows.size()), windows.data(), d_src, d_mask,
					scratch.base, new_off.data(), new_cbytes.data(), status.data()), "Writing the masked regions");
			else if constexpr (typed)
				detail::engine_call(e, cimg_update_windows_typed_device(e, &cp, static_cast<int32_t>(n), old.base, old.off.data(), old.cbytes.data(),
					old.nbytes.data(), old.blocksize.data(), destsize.data(), static_cast<int32_t>(windows.size()), windows.data(), d_src, scratch.base,
					new_off.data(), new_cbytes.data(), status.data()), "Writing the typed regions");
			else if constexpr (strided)
				detail::engine_call(e, cimg_update_windows_strided_device(e, &cp, static_cast<int32_t>(n), old.base, old.off.data(), old.cbytes.data(),
					old.nbytes.data(), old.blocksize.data(), destsize.data(), static_cast<int32_t>(windows.size()), windows.data(), d_src, scratch.base,
					new_off.data(), new_cbytes.data(), status.data()), "Writing the regions");
			else
				detail::engine_call(e, cimg_update_windows_device(e, &cp, static_cast<int32_t>(n), old.base, old.off.data(), old.cbytes.data(), old.nbytes.data(),
					old.blocksize.data(), destsize.data(), static_cast<int32_t>(windows.size()), windows.data(), d_src, scratch.base, new_off.data(),
					new_cbytes.data(), status.data()), "Writing the region");
			auto fresh = std::make_shared<detail::device_store>();
			fresh->nbytes = old.nbytes;
			fresh->blocksize = old.blocksize;
			fresh->cbytes = old.cbytes;
			std::vector<const void*> src(n);
			for (size_t i = 0; i < n; ++i)
			{
				if (new_cbytes[i] > 0) { fresh->cbytes[i] = new_cbytes[i]; src[i] = scratch.base + new_off[i]; }
				else src[i] = old.base + old.off[i];
			}
			fresh->allocate(e, detail::device_store::pack_offsets(fresh->cbytes, fresh->off));
			detail::engine_call(e, cimg_pack_chunks_device(e, static_cast<int32_t>(n), src.data(), fresh->cbytes.data(), fresh->base, fresh->off.data()),
				"Repacking the store");
			return fresh;
		}

	private:
		friend struct device_image<T>;
		std::shared_ptr<detail::device_store> m_Store;
		size_t m_First = 0, m_Count = 0;              // this channel's chunks of the store
		bool m_ReadOnly = false;
		enums::codec m_Codec = enums::codec::lz4;
		uint8_t m_CompressionLevel = 9;
		std::optional<int> m_MantissaBits = std::nullopt;
		size_t m_BlockSize = s_default_blocksize;
		size_t m_ChunkSize = s_default_chunksize;
		size_t m_Width = 1;
		size_t m_Height = 1;

		device_channel(enums::codec codec, uint8_t level, size_t block_size, size_t chunk_size, size_t width, size_t height, std::optional<int> mantissa_bits = std::nullopt)
			: m_Codec(codec), m_CompressionLevel(level), m_MantissaBits(mantissa_bits), m_BlockSize(block_size), m_ChunkSize(chunk_size), m_Width(width), m_Height(height) {}
		void require() const
		{
			if (!m_Store || m_Count == 0)
				throw std::runtime_error("Internal Error: device_channel instance is not properly initialized, unable to access its data");
		}
	};
}
