// blosc2/wrapper.h -- host-side seam onto the codec.  Same names and error behaviour as the reference's
// compressed/blosc2/wrapper.h (codec mapping :74-119, compress :134-223, decompress :236-277,
// context factories :313-413, size helpers :416-468), served by libcimg_hip.so through
// include/blosc2.h, plus the *batched* helpers the re-shaped chunk loops use (include/cimg_hip.h).
#pragma once
#include <unordered_map>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <memory>
#include <mutex>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

#include "blosc2.h"
#include "cimg_hip.h"
#include "../detail/pinned_pool.h"

#include "../macros.h"
#include "../enums.h"
#include "../detail/text.h"
#include "../half.h"
#include <optional>
#include <type_traits>

namespace NAMESPACE_COMPRESSED_IMAGE
{
	namespace blosc2
	{
		inline std::string map_error_code(int rc) { return std::string(print_error(rc)); }   // reference blosc2/util.h:16-19

		template <typename S> struct deleter;
		template <> struct deleter<blosc2_schunk> { void operator()(blosc2_schunk* s) const { blosc2_schunk_free(s); } };
		template <> struct deleter<blosc2_context> { void operator()(blosc2_context* c) const { blosc2_free_ctx(c); } };

		using schunk_ptr = std::unique_ptr<blosc2_schunk, deleter<blosc2_schunk>>;
		using schunk_raw_ptr = blosc2_schunk*;
		using chunk_raw_ptr = void*;
		using context_ptr = std::unique_ptr<blosc2_context, deleter<blosc2_context>>;
		using context_raw_ptr = blosc2_context*;

		inline uint8_t codec_to_blosc2(enums::codec c)
		{
			switch (c)
			{
			case enums::codec::lz4: return BLOSC_LZ4;
			case enums::codec::lz4hc: return BLOSC_LZ4HC;
			case enums::codec::zstd: return BLOSC_ZSTD;
			default: return BLOSC_BLOSCLZ;
			}
		}
		inline enums::codec blosc2_to_codec(uint8_t c)
		{
			switch (c)
			{
			case BLOSC_LZ4: return enums::codec::lz4;
			case BLOSC_LZ4HC: return enums::codec::lz4hc;
			case BLOSC_ZSTD: return enums::codec::zstd;
			default: return enums::codec::blosclz;
			}
		}

		// ---- single chunk (one blosc2_*_ctx call, host pointers) ----------------------------------------------
		template <typename T>
		size_t compress(context_raw_ptr context, std::span<const T> data, std::span<std::byte> chunk)
		{
			const int cbytes = blosc2_compress_ctx(context, data.data(), static_cast<int32_t>(data.size() * sizeof(T)),
				chunk.data(), static_cast<int32_t>(chunk.size()));
			if (cbytes < 0)
				throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", cbytes));
			return static_cast<size_t>(cbytes);
		}
		template <typename T> size_t compress(context_raw_ptr context, std::span<T> data, std::span<std::byte> chunk) requires(!std::is_const_v<T>)
		{
			return compress<T>(context, std::span<const T>(data.data(), data.size()), chunk);
		}
		template <typename T> size_t compress(context_ptr& context, std::span<T> data, std::span<std::byte> chunk) { return compress<std::remove_const_t<T>>(context.get(), std::span<const std::remove_const_t<T>>(data.data(), data.size()), chunk); }

		template <typename T>
		size_t decompress(context_raw_ptr context, std::span<T> buffer, std::span<const std::byte> chunk)
		{
			if (buffer.size() * sizeof(T) > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
				throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", buffer.size() * sizeof(T), " which would exceed that"));
			const int n = blosc2_decompress_ctx(context, chunk.data(), std::numeric_limits<int32_t>::max(), buffer.data(),
				static_cast<int32_t>(buffer.size() * sizeof(T)));
			if (n < 0)
				throw std::runtime_error(detail::text("Error code ", n, " while decompressing blosc2 chunk"));
			return static_cast<size_t>(n);
		}
		template <typename T> size_t decompress(context_ptr& context, std::span<T> buffer, std::span<const std::byte> chunk) { return decompress(context.get(), buffer, chunk); }

		inline size_t append_chunk(schunk_ptr& schunk, std::span<std::byte> chunk)
		{
			const auto n = blosc2_schunk_append_chunk(schunk.get(), reinterpret_cast<uint8_t*>(chunk.data()), true);
			if (n < 0)
				throw std::runtime_error(detail::text("Unable to append chunk into super-chunk with the following blosc2 error code ", n));
			return static_cast<size_t>(n);
		}

		inline schunk_ptr create_default_schunk()
		{
			auto cparams = BLOSC2_CPARAMS_DEFAULTS;
			auto dparams = BLOSC2_DPARAMS_DEFAULTS;
			blosc2_storage storage = BLOSC2_STORAGE_DEFAULTS;
			storage.cparams = &cparams;
			storage.dparams = &dparams;
			return schunk_ptr(blosc2_schunk_new(&storage));
		}

		// ---- contexts -----------------------------------------------------------------------------------------
		/// Lossy float storage (blosc2's trunc-prec filter, slot 4): the mantissa bits KEPT, 1 .. M with M = 10 / 23 / 52 for
		/// half / float / double.  std::invalid_argument for any other element type or a value out of range.
		template <typename T>
		inline constexpr int mantissa_width = std::is_same_v<T, half> ? 10 : std::is_same_v<T, float> ? 23 : std::is_same_v<T, double> ? 52 : 0;
		template <typename T>
		void ensure_mantissa_bits(const std::optional<int>& mantissa_bits)
		{
			if (!mantissa_bits) return;
			if (mantissa_width<T> == 0)
				throw std::invalid_argument("mantissa_bits is only available for floating-point element types (half, float, double)");
			if (*mantissa_bits < 1 || *mantissa_bits > mantissa_width<T>)
				throw std::invalid_argument(detail::text("mantissa_bits must lie in 1 .. ", mantissa_width<T>, " for this element type, got ", *mantissa_bits));
		}
		template <typename T>
		blosc2_cparams create_blosc2_cparams(size_t nthreads, enums::codec codec, uint8_t compression_level, size_t block_size,
			std::optional<int> mantissa_bits = std::nullopt)
		{
			ensure_mantissa_bits<T>(mantissa_bits);
			if (nthreads > static_cast<size_t>(std::numeric_limits<int16_t>::max()))
				throw std::out_of_range(detail::text("Number of threads may not exceed ", std::numeric_limits<int16_t>::max(), ", got ", nthreads));
			blosc2_cparams p = BLOSC2_CPARAMS_DEFAULTS;
			p.blocksize = static_cast<int32_t>(block_size);
			p.typesize = sizeof(T);
			p.splitmode = BLOSC_AUTO_SPLIT;
			p.clevel = compression_level;
			p.nthreads = static_cast<int16_t>(nthreads == 0 ? 1 : nthreads);    // accepted, ignored: the parallelism is the GPU's
			p.compcode = codec_to_blosc2(codec);
			if (mantissa_bits)
			{
				p.filters[BLOSC2_MAX_FILTERS - 2] = BLOSC_TRUNC_PREC;
				p.filters_meta[BLOSC2_MAX_FILTERS - 2] = static_cast<uint8_t>(*mantissa_bits);
			}
			// All four codecs of the reference construct (enums.h:18-24).  lz4 and blosclz chunks are the reference's bytes; lz4hc
			// and zstd chunks are FORMAT-VALID -- every LZ4 / zstd decoder, c-blosc2 included, reads them -- but not liblz4-HC's /
			// libzstd's bytes (csrc/plan.h, csrc/zstd_encode.h).
			return p;
		}
		template <typename T>
		context_ptr create_compression_context(size_t nthreads, enums::codec codec, uint8_t compression_level, size_t block_size,
			std::optional<int> mantissa_bits = std::nullopt)
		{
			return context_ptr(blosc2_create_cctx(create_blosc2_cparams<T>(nthreads, codec, compression_level, block_size, mantissa_bits)));
		}
		template <typename T>
		context_ptr create_compression_context(schunk_ptr& schunk, size_t nthreads, enums::codec codec, uint8_t compression_level, size_t block_size,
			std::optional<int> mantissa_bits = std::nullopt)
		{
			auto p = create_blosc2_cparams<T>(nthreads, codec, compression_level, block_size, mantissa_bits);
			p.schunk = schunk.get();
			return context_ptr(blosc2_create_cctx(p));
		}
		inline context_ptr create_decompression_context(size_t nthreads)
		{
			if (nthreads > static_cast<size_t>(std::numeric_limits<int16_t>::max()))
				throw std::out_of_range(detail::text("Number of threads may not exceed ", std::numeric_limits<int16_t>::max(), ", got ", nthreads));
			auto d = BLOSC2_DPARAMS_DEFAULTS;
			d.nthreads = 1;
			return context_ptr(blosc2_create_dctx(d));
		}
		inline context_ptr create_decompression_context(schunk_ptr& schunk, size_t nthreads)
		{
			auto ctx = create_decompression_context(nthreads);
			(void)schunk;
			return ctx;
		}

		// ---- sizes -----------------------------------------------------------------------------------------------
		template <size_t ChunkSize> constexpr size_t min_compressed_size() { return ChunkSize + BLOSC2_MAX_OVERHEAD; }
		inline constexpr size_t min_compressed_size(size_t chunk_size) { return chunk_size + BLOSC2_MAX_OVERHEAD; }
		template <size_t ChunkSize> constexpr size_t min_decompressed_size() { return ChunkSize; }
		inline constexpr size_t min_decompressed_size(size_t chunk_size) { return chunk_size; }

		inline size_t chunk_num_bytes(const std::byte* chunk)
		{
			int32_t nbytes{}, cbytes{}, blocksize{};
			const int rc = blosc2_cbuffer_sizes(chunk, &nbytes, &cbytes, &blocksize);
			if (rc < 0)
				throw std::runtime_error(detail::text("Unable to find buffer sizes due to blosc2 error: ", map_error_code(rc)));
			return static_cast<size_t>(nbytes);
		}
		template <typename T> size_t chunk_num_elements(const std::vector<std::byte>& chunk) { return chunk_num_bytes(chunk.data()) / sizeof(T); }
		template <typename T> size_t chunk_num_elements(std::span<const std::byte> chunk) { return chunk_num_bytes(chunk.data()) / sizeof(T); }

		// ---- batches: what replaces the reference's serial chunk loops --------------------------------------------
		/// The bytes of one compressed chunk: immutable, cheap to move, either a view into the arena a whole batch of
		/// chunks was fetched into (shared ownership) or a vector adopted from the caller.
		class byte_buffer
		{
		public:
			byte_buffer() = default;
			byte_buffer(std::vector<std::byte> bytes)
			{
				auto held = std::make_shared<std::vector<std::byte>>(std::move(bytes));
				m_Data = held->data();
				m_Size = held->size();
				m_Owner = std::move(held);
			}
			byte_buffer(std::shared_ptr<const void> owner, const std::byte* data, size_t size) : m_Owner(std::move(owner)), m_Data(data), m_Size(size) {}

			const std::byte* data() const noexcept { return m_Data; }
			size_t size() const noexcept { return m_Size; }
			bool empty() const noexcept { return m_Size == 0; }
			const std::byte* begin() const noexcept { return m_Data; }
			const std::byte* end() const noexcept { return m_Data + m_Size; }
			const std::byte& operator[](size_t i) const noexcept { return m_Data[i]; }

		private:
			std::shared_ptr<const void> m_Owner;
			const std::byte* m_Data = nullptr;
			size_t m_Size = 0;
		};

		namespace batch
		{
			inline cimg_engine* engine()
			{
				cimg_engine* e = cimg_shared_engine();
				if (!e)
					throw std::runtime_error(detail::text("compressed-image MI355X engine unavailable: ", cimg_last_error(nullptr)));
				return e;
			}

			struct piece { const std::byte* data; size_t nbytes; };          // one chunk's pixels (host memory)

			// Compress many chunks in one engine call.  Every chunk gets destsize = nominal chunk size +
			// BLOSC2_MAX_OVERHEAD, as the reference passes it (schunk.h:73, :200, :225).
			inline std::vector<byte_buffer> compress(context_raw_ptr cctx, const std::vector<piece>& pieces, size_t nominal_chunk_bytes)
			{
				std::vector<byte_buffer> out(pieces.size());
				if (pieces.empty()) return out;
				cimg_cparams cp;
				int rc = cimg_context_cparams(cctx, &cp);
				if (rc < 0) throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", rc));
				const size_t n = pieces.size();
				std::vector<int64_t> raw_off(n), comp_off(n);
				std::vector<int32_t> nbytes(n), destsize(n), cbytes(n);
				const std::byte* base = pieces[0].data;
				for (const auto& p : pieces) if (p.data < base) base = p.data;
				for (size_t i = 0; i < n; ++i)
				{
					if (pieces[i].nbytes > static_cast<size_t>(BLOSC2_MAX_BUFFERSIZE))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", pieces[i].nbytes));
					raw_off[i] = pieces[i].data - base;
					nbytes[i] = static_cast<int32_t>(pieces[i].nbytes);
					destsize[i] = static_cast<int32_t>(min_compressed_size(nominal_chunk_bytes));
				}
				// _begin and _fetch belong together: the engine's own (recursive) lock is held across the pair, so no other
				// user of the shared engine -- batch::decompress, the blosc2_*_ctx shim, another thread's compress -- can
				// reuse its staging area in between
				struct engine_guard
				{
					cimg_engine* e;
					explicit engine_guard(cimg_engine* e_) : e(e_) { cimg_engine_lock(e); }
					~engine_guard() { cimg_engine_unlock(e); }
				} pair_lock(engine());
				// ONE call: upload, compress and bring the chunks back group by group -- as soon as the sizes of a group are known the
				// engine asks for a block of exactly that size (recycled, page-locked: detail/pinned_pool.h) and sends the group's
				// chunks there while the next group is being compressed; the chunks are views into those blocks -- no staging area of
				// nominal size, no second copy.  (Round 3 fetched all chunks behind the last group: 4.2 against 3.0 ms for an image of
				// 4 x 4096^2 float16.)
				struct arenas_t
				{
					std::vector<std::pair<std::shared_ptr<std::byte>, size_t>> blocks;
					static void* take(void* user, size_t bytes)
					{
						auto* self = static_cast<arenas_t*>(user);
						try
						{
							self->blocks.emplace_back(NAMESPACE_COMPRESSED_IMAGE::detail::pinned_pool::get().arena(bytes), bytes);
						}
						catch (...) { return nullptr; }
						return self->blocks.back().first.get();
					}
				} arenas;
				std::vector<void*> where(n, nullptr);
				rc = cimg_compress_batch_host_packed(engine(), &cp, static_cast<int32_t>(n), base, raw_off.data(), nbytes.data(), destsize.data(), cbytes.data(),
					&arenas_t::take, &arenas, where.data());
				if (rc < 0)
					throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", rc, " (", cimg_last_error(engine()), ")"));
				for (size_t i = 0; i < n; ++i)
				{
					if (cbytes[i] <= 0 || !where[i])
						throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", cbytes[i]));
					std::byte* at = static_cast<std::byte*>(where[i]);
					const std::shared_ptr<std::byte>* owner = nullptr;
					for (const auto& blk : arenas.blocks)
						if (at >= blk.first.get() && at < blk.first.get() + blk.second) { owner = &blk.first; break; }
					if (!owner)
						throw std::runtime_error("compressed chunk arrived outside the blocks handed to the engine");
					out[i] = byte_buffer(*owner, at, static_cast<size_t>(cbytes[i]));
				}
				return out;
			}

			// The same for pixels that arrive INTERLEAVED (R G B A R G B A ...) in host memory: uploaded once, split into planes on
			// the device (the reference's image_algo::deinterleave, a host loop between reading and compressing, image.h:1880),
			// compressed from there.  A piece names its bytes in the PLANAR layout: channel c occupies
			// [c * plane_stride, c * plane_stride + npixels * typesize), plane_stride = that size rounded up to 16.
			struct planar_piece { size_t offset; size_t nbytes; };
			inline size_t planar_stride(size_t npixels, size_t typesize) { return (npixels * typesize + 15) & ~size_t{ 15 }; }
			inline std::vector<byte_buffer> compress_interleaved(context_raw_ptr cctx, const std::byte* interleaved, size_t nchannels, size_t npixels,
				const std::vector<planar_piece>& pieces, size_t nominal_chunk_bytes)
			{
				std::vector<byte_buffer> out(pieces.size());
				if (pieces.empty()) return out;
				cimg_cparams cp;
				int rc = cimg_context_cparams(cctx, &cp);
				if (rc < 0) throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", rc));
				const size_t n = pieces.size();
				std::vector<int64_t> raw_off(n), comp_off(n);
				std::vector<int32_t> nbytes(n), destsize(n), cbytes(n);
				for (size_t i = 0; i < n; ++i)
				{
					if (pieces[i].nbytes > static_cast<size_t>(BLOSC2_MAX_BUFFERSIZE))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", pieces[i].nbytes));
					raw_off[i] = static_cast<int64_t>(pieces[i].offset);
					nbytes[i] = static_cast<int32_t>(pieces[i].nbytes);
					destsize[i] = static_cast<int32_t>(min_compressed_size(nominal_chunk_bytes));
				}
				struct engine_guard
				{
					cimg_engine* e;
					explicit engine_guard(cimg_engine* e_) : e(e_) { cimg_engine_lock(e); }
					~engine_guard() { cimg_engine_unlock(e); }
				} pair_lock(engine());
				rc = cimg_compress_batch_host_interleaved_begin(engine(), &cp, static_cast<int32_t>(nchannels), static_cast<int64_t>(npixels), interleaved,
					static_cast<int32_t>(n), raw_off.data(), nbytes.data(), destsize.data(), cbytes.data());
				if (rc < 0)
					throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", rc, " (", cimg_last_error(engine()), ")"));
				size_t total = 0;
				for (size_t i = 0; i < n; ++i)
				{
					if (cbytes[i] <= 0)
						throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", cbytes[i]));
					comp_off[i] = static_cast<int64_t>(total);
					total += (static_cast<size_t>(cbytes[i]) + 63) & ~size_t{ 63 };
				}
				std::shared_ptr<std::byte> arena = NAMESPACE_COMPRESSED_IMAGE::detail::pinned_pool::get().arena(total);
				rc = cimg_compress_batch_host_fetch(engine(), static_cast<int32_t>(n), arena.get(), comp_off.data());
				if (rc < 0)
					throw std::runtime_error(detail::text("Unable to compress context using Blosc2 with error code ", rc, " (", cimg_last_error(engine()), ")"));
				for (size_t i = 0; i < n; ++i)
					out[i] = byte_buffer(arena, arena.get() + comp_off[i], static_cast<size_t>(cbytes[i]));
				return out;
			}

			// Windows of several planes in one engine call (cimg_decompress_windows_host): only the blocks the windows meet are decoded
			// and only the windows' bytes come back.  windows[i] names chunks by their index in `chunks`; its out_off is filled in
			// here from outs[i], where its first element goes.
			// (Window: cimg_window, or cimg_window_strided for subsampled regions -- cimg_decompress_windows_strided_host decodes only
			// the blocks that hold a sampled element.)
			template <typename Window>
			struct window_job_of
			{
				std::vector<const std::byte*> chunks;
				std::vector<size_t> held;               // bytes each chunk buffer holds
				std::vector<Window> windows;
				std::vector<std::byte*> outs;
				// share_runs (get_regions): a run of chunks that an earlier region of the job queued is not queued again -- first_of
				// finds it by its first chunk (a table always queues a run whole) -- so that windows of different regions name the
				// same batch chunks: the condition for the grouped call to stage a shared block once and upload a shared chunk once
				bool share_runs = false;
				std::unordered_map<const std::byte*, int32_t> runs;     // a queued run's first chunk -> its index in `chunks`
				/// Index in `chunks` of the run [first, first + count) of `chunk_at(k)` = {bytes, size}, queued now unless shared
				template <typename ChunkAt>
				int32_t queue_run(size_t first, size_t count, ChunkAt&& chunk_at)
				{
					const std::byte* key = chunk_at(first).first;
					if (share_runs)
						if (auto it = runs.find(key); it != runs.end()) return it->second;
					if (chunks.size() + count > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range("too many chunks for one window call");
					const int32_t at = static_cast<int32_t>(chunks.size());
					for (size_t k = first; k < first + count; ++k) { auto c = chunk_at(k); chunks.push_back(c.first); held.push_back(c.second); }
					if (share_runs) runs.emplace(key, at);
					return at;
				}
			};
			using window_job = window_job_of<cimg_window>;
			using strided_window_job = window_job_of<cimg_window_strided>;

			inline int decompress_windows_call(int32_t n, const void* comp, const int64_t* comp_off, const int32_t* held, int32_t nwindows,
				const cimg_window* w, void* out, int32_t* status)
			{
				return cimg_decompress_windows_host(engine(), n, comp, comp_off, held, nwindows, w, out, status);
			}
			inline int decompress_windows_call(int32_t n, const void* comp, const int64_t* comp_off, const int32_t* held, int32_t nwindows,
				const cimg_window_strided* w, void* out, int32_t* status)
			{
				return cimg_decompress_windows_strided_host(engine(), n, comp, comp_off, held, nwindows, w, out, status);
			}

			// (grouped: cimg_decompress_windows_grouped_host -- every block staged once for all the windows that meet it)
			inline int decompress_windows_grouped_call(int32_t n, const void* comp, const int64_t* comp_off, const int32_t* held, int32_t nwindows,
				const cimg_window_strided* w, void* out, int32_t* status)
			{
				return cimg_decompress_windows_grouped_host(engine(), n, comp, comp_off, held, nwindows, w, out, status);
			}

			template <typename Window, typename Call>
			inline void decompress_windows_with(window_job_of<Window>& job, Call&& call)
			{
				if (job.windows.empty()) return;
				const std::byte* cbase = job.chunks.empty() ? nullptr : job.chunks[0];
				for (const auto* c : job.chunks) if (c < cbase) cbase = c;
				std::byte* obase = job.outs[0];
				for (auto* o : job.outs) if (o < obase) obase = o;
				const size_t n = job.chunks.size();
				if (n > static_cast<size_t>(std::numeric_limits<int32_t>::max()) || job.windows.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
					throw std::out_of_range(detail::text("too many chunks or windows for one call: ", n, " chunks, ", job.windows.size(), " windows"));
				std::vector<int64_t> comp_off(n);
				std::vector<int32_t> held(n), status(n);
				for (size_t i = 0; i < n; ++i)
				{
					if (job.held[i] > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", job.held[i]));
					comp_off[i] = job.chunks[i] - cbase;
					held[i] = static_cast<int32_t>(job.held[i]);
				}
				for (size_t k = 0; k < job.windows.size(); ++k) job.windows[k].out_off = job.outs[k] - obase;
				const int rc = call(static_cast<int32_t>(n), cbase, comp_off.data(), held.data(),
					static_cast<int32_t>(job.windows.size()), job.windows.data(), obase, status.data());
				if (rc < 0)
					throw std::runtime_error(detail::text("Error code ", rc, " while decompressing a region of blosc2 chunks (", cimg_last_error(engine()), ")"));
			}
			template <typename Window>
			inline void decompress_windows(window_job_of<Window>& job)
			{
				decompress_windows_with(job, [](auto... a) { return decompress_windows_call(a...); });
			}

			// Many regions in one grouped call (cimg_decompress_windows_grouped_host).  The job was planned with share_runs, so the
			// regions' windows name the same batch chunks wherever they read the same table.
			inline void decompress_windows_grouped(strided_window_job& job)
			{
				decompress_windows_with(job, [](auto... a) { return decompress_windows_grouped_call(a...); });
			}

			// Window writes of several planes in one engine call (cimg_update_windows_host): only the blocks the windows meet are decoded
			// and re-encoded, and only the touched chunks and the windows' bytes travel.  windows[i] names chunks by their index in
			// `chunks`; its out_off is filled in here from srcs[i], where its first source element lies.  Every new chunk gets destsize[i]
			// (what set_chunk passes: min_compressed_size of the nominal chunk size).  Returns the new form of every chunk, empty where
			// no window row meets it; throws on any error, and the caller's chunks stay as they were.
			struct update_job
			{
				std::vector<const std::byte*> chunks;
				std::vector<size_t> held;               // bytes each chunk buffer holds
				std::vector<int32_t> destsize;
				std::vector<cimg_window> windows;
				std::vector<const std::byte*> srcs;
				cimg_cparams cparams{};
			};

			inline std::vector<std::vector<std::byte>> update_windows(update_job& job)
			{
				const size_t n = job.chunks.size();
				std::vector<std::vector<std::byte>> out(n);
				if (job.windows.empty()) return out;
				const std::byte* cbase = job.chunks.empty() ? nullptr : job.chunks[0];
				for (const auto* c : job.chunks) if (c < cbase) cbase = c;
				const std::byte* sbase = job.srcs[0];
				for (const auto* s : job.srcs) if (s < sbase) sbase = s;
				std::vector<int64_t> comp_off(n);
				std::vector<int32_t> held(n), status(n), ncb(n);
				std::vector<void*> made(n, nullptr);
				for (size_t i = 0; i < n; ++i)
				{
					if (job.held[i] > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", job.held[i]));
					comp_off[i] = job.chunks[i] - cbase;
					held[i] = static_cast<int32_t>(job.held[i]);
				}
				for (size_t k = 0; k < job.windows.size(); ++k) job.windows[k].out_off = job.srcs[k] - sbase;
				const auto alloc = [](void*, size_t bytes) -> void* { return std::malloc(bytes ? bytes : 1); };
				const int rc = cimg_update_windows_host(engine(), &job.cparams, static_cast<int32_t>(n), cbase, comp_off.data(), held.data(),
					job.destsize.data(), static_cast<int32_t>(job.windows.size()), job.windows.data(), sbase, alloc, nullptr, made.data(),
					ncb.data(), status.data());
				for (size_t i = 0; i < n; ++i)
				{
					if (!made[i]) continue;
					const auto* b = static_cast<const std::byte*>(made[i]);
					out[i].assign(b, b + ncb[i]);
					std::free(made[i]);
				}
				if (rc < 0)
					throw std::runtime_error(detail::text("Error code ", rc, " while writing a region into blosc2 chunks (", cimg_last_error(engine()), ")"));
				return out;
			}

			// The same over cimg_window_strided (cimg_update_windows_strided_host): set_region with steps, set_regions.  A template, so
			// that only code that instantiates it refers to the strided entry point.
			struct update_job_strided
			{
				std::vector<const std::byte*> chunks;
				std::vector<size_t> held;
				std::vector<int32_t> destsize;
				std::vector<cimg_window_strided> windows;
				std::vector<const std::byte*> srcs;
				cimg_cparams cparams{};
			};

			template <typename Job = update_job_strided>
			inline std::vector<std::vector<std::byte>> update_windows_strided(Job& job)
			{
				const size_t n = job.chunks.size();
				std::vector<std::vector<std::byte>> out(n);
				if (job.windows.empty()) return out;
				if (job.windows.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("set_regions: too many windows for one call");
				const std::byte* cbase = job.chunks[0];
				for (const auto* c : job.chunks) if (c < cbase) cbase = c;
				const std::byte* sbase = job.srcs[0];
				for (const auto* s : job.srcs) if (s < sbase) sbase = s;
				std::vector<int64_t> comp_off(n);
				std::vector<int32_t> held(n), status(n), ncb(n);
				std::vector<void*> made(n, nullptr);
				for (size_t i = 0; i < n; ++i)
				{
					if (job.held[i] > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", job.held[i]));
					comp_off[i] = job.chunks[i] - cbase;
					held[i] = static_cast<int32_t>(job.held[i]);
				}
				for (size_t k = 0; k < job.windows.size(); ++k) job.windows[k].out_off = job.srcs[k] - sbase;
				const auto alloc = [](void*, size_t bytes) -> void* { return std::malloc(bytes ? bytes : 1); };
				const int rc = cimg_update_windows_strided_host(engine(), &job.cparams, static_cast<int32_t>(n), cbase, comp_off.data(), held.data(),
					job.destsize.data(), static_cast<int32_t>(job.windows.size()), job.windows.data(), sbase, alloc, nullptr, made.data(),
					ncb.data(), status.data());
				for (size_t i = 0; i < n; ++i)
				{
					if (!made[i]) continue;
					const auto* b = static_cast<const std::byte*>(made[i]);
					out[i].assign(b, b + ncb[i]);
					std::free(made[i]);
				}
				if (rc < 0)
					throw std::runtime_error(detail::text("Error code ", rc, " while writing regions into blosc2 chunks (", cimg_last_error(engine()), ")"));
				return out;
			}

			// The same over cimg_window_masked (cimg_update_windows_masked_host): fill_region / fill_regions and the masked set_region /
			// set_regions.  srcs[k] is null for a constant window, masks[k] for an unmasked one; a call of constant windows names no
			// source at all, so nothing but the touched chunks (and the mask rows) travels.  A template, so that only code that
			// instantiates it refers to the masked entry point.
			struct update_job_masked
			{
				std::vector<const std::byte*> chunks;
				std::vector<size_t> held;
				std::vector<int32_t> destsize;
				std::vector<cimg_window_masked> windows;
				std::vector<const std::byte*> srcs;
				std::vector<const uint8_t*> masks;
				cimg_cparams cparams{};
			};

			template <typename Job = update_job_masked>
			inline std::vector<std::vector<std::byte>> update_windows_masked(Job& job)
			{
				const size_t n = job.chunks.size();
				std::vector<std::vector<std::byte>> out(n);
				if (job.windows.empty()) return out;
				if (job.windows.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) throw std::out_of_range("fill_regions: too many windows for one call");
				const std::byte* cbase = job.chunks[0];
				for (const auto* c : job.chunks) if (c < cbase) cbase = c;
				const std::byte* sbase = nullptr;
				for (const auto* s : job.srcs) if (s && (!sbase || s < sbase)) sbase = s;
				const uint8_t* mbase = nullptr;
				for (const auto* m : job.masks) if (m && (!mbase || m < mbase)) mbase = m;
				std::vector<int64_t> comp_off(n);
				std::vector<int32_t> held(n), status(n), ncb(n);
				std::vector<void*> made(n, nullptr);
				for (size_t i = 0; i < n; ++i)
				{
					if (job.held[i] > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", job.held[i]));
					comp_off[i] = job.chunks[i] - cbase;
					held[i] = static_cast<int32_t>(job.held[i]);
				}
				for (size_t k = 0; k < job.windows.size(); ++k)
				{
					if (job.srcs[k]) job.windows[k].out_off = job.srcs[k] - sbase;
					if (job.masks[k]) job.windows[k].mask_off = job.masks[k] - mbase;
				}
				const auto alloc = [](void*, size_t bytes) -> void* { return std::malloc(bytes ? bytes : 1); };
				const int rc = cimg_update_windows_masked_host(engine(), &job.cparams, static_cast<int32_t>(n), cbase, comp_off.data(), held.data(),
					job.destsize.data(), static_cast<int32_t>(job.windows.size()), job.windows.data(), sbase, mbase, alloc, nullptr, made.data(),
					ncb.data(), status.data());
				for (size_t i = 0; i < n; ++i)
				{
					if (!made[i]) continue;
					const auto* b = static_cast<const std::byte*>(made[i]);
					out[i].assign(b, b + ncb[i]);
					std::free(made[i]);
				}
				if (rc < 0)
					throw std::runtime_error(detail::text("Error code ", rc, " while writing masked regions into blosc2 chunks (", cimg_last_error(engine()), ")"));
				return out;
			}

			// one chunk -> its pixels; chunk_bytes = what the chunk buffer really holds (0: unknown, trust the header)
			struct target { const std::byte* chunk; std::byte* out; size_t capacity; size_t chunk_bytes = 0; };

			inline void decompress(const std::vector<target>& items)
			{
				if (items.empty()) return;
				const size_t n = items.size();
				const std::byte* cbase = items[0].chunk;
				std::byte* rbase = items[0].out;
				for (const auto& t : items) { if (t.chunk < cbase) cbase = t.chunk; if (t.out < rbase) rbase = t.out; }
				std::vector<int64_t> comp_off(n), raw_off(n);
				std::vector<int32_t> cap(n), status(n), held(n);
				bool sized = true;
				for (size_t i = 0; i < n; ++i)
				{
					sized = sized && items[i].chunk_bytes > 0 && items[i].chunk_bytes <= static_cast<size_t>(std::numeric_limits<int32_t>::max());
					held[i] = static_cast<int32_t>(items[i].chunk_bytes);
					if (items[i].capacity > static_cast<size_t>(std::numeric_limits<int32_t>::max()))
						throw std::out_of_range(detail::text("Blosc2 chunk size may not exceed numeric limit of int32_t, got ", items[i].capacity, " which would exceed that"));
					comp_off[i] = items[i].chunk - cbase;
					raw_off[i] = items[i].out - rbase;
					cap[i] = static_cast<int32_t>(items[i].capacity);
				}
				const int rc = cimg_decompress_batch_host_sized(engine(), static_cast<int32_t>(n), cbase, comp_off.data(), sized ? held.data() : nullptr,
					rbase, raw_off.data(), cap.data(), status.data());
				if (rc < 0)
					throw std::runtime_error(detail::text("Error code ", rc, " while decompressing blosc2 chunk"));
			}
		}
	}
}
