// blosc2/schunk.h -- host bookkeeping of a channel's chunks: `schunk<T>` (every chunk compressed) and
// `lazy_schunk<T>` (a chunk is either compressed bytes or a single fill value), with the public
// surface of the reference's compressed/blosc2/{schunk.h, lazyschunk.h, schunk_mixin.h}.
//
// What is different from the reference is the shape of the hot loops: the constructor from pixels
// (reference schunk.h:65-105, one blosc2_compress_ctx per chunk, serially) and to_uncompressed
// (schunk.h:123-141 / lazyschunk.h:176-194, one blosc2_decompress_ctx per chunk on one thread) hand
// ALL chunks to the GPU engine in one batched call (blosc2/wrapper.h: batch::compress / decompress).
// Both flavours share one implementation: a table of slots {bytes | fill value, element count}.
#pragma once
#include <algorithm>
#include <cstddef>
#include <span>
#include <stdexcept>
#include <variant>
#include <vector>

#include "../constants.h"
#include "../macros.h"
#include "../util.h"
#include "wrapper.h"

namespace NAMESPACE_COMPRESSED_IMAGE
{
	namespace blosc2
	{
		namespace detail
		{
			template <typename T>
			struct lazy_chunk
			{
				std::variant<byte_buffer, T> value;
				size_t num_elements = 0;
				size_t byte_size() const noexcept { return num_elements * sizeof(T); }
				bool is_lazy() const noexcept { return std::holds_alternative<T>(value); }
				const byte_buffer& bytes() const { return std::get<byte_buffer>(value); }
			};

			// Lazy == false: slots always hold bytes and the element count is read from the chunk header
			// (as the reference's schunk does); Lazy == true: slots may hold a fill value.
			template <typename T, bool Lazy>
			struct chunk_table
			{
				using slot = lazy_chunk<T>;

				chunk_table() = default;

				// ---- geometry ------------------------------------------------------------------------------------
				size_t chunk_bytes() const { return m_ChunkSize; }
				size_t chunk_bytes(size_t index) const
				{
					validate_chunk_index(index);
					return m_Chunks[index].num_elements * sizeof(T);
				}
				size_t chunk_elements() const { return elements_of(chunk_bytes()); }
				size_t chunk_elements(size_t index) const { return elements_of(chunk_bytes(index)); }
				size_t num_chunks() const noexcept { return m_Chunks.size(); }
				size_t max_chunk_size() const { return m_ChunkSize; }
				size_t max_block_size() const { return m_BlockSize; }
				size_t byte_size() const noexcept { return size() * sizeof(T); }

				// total elements
				size_t size() const noexcept
				{
					size_t n = 0;
					for (const auto& c : m_Chunks) n += c.num_elements;
					return n;
				}
				// total stored bytes (a lazy slot costs sizeof(T), reference lazyschunk.h csize())
				size_t csize() const noexcept
				{
					size_t n = 0;
					for (const auto& c : m_Chunks) n += c.is_lazy() ? sizeof(T) : c.bytes().size();
					return n;
				}

				// ---- export to a blosc2 super-chunk (reference schunk.h:107-121, lazyschunk.h:122-172) -----------
				schunk_ptr to_schunk()
				{
					schunk_ptr out = create_default_schunk();
					std::vector<std::byte> filler;        // one compressed chunk of the fill value, lz4 level 9 as the reference does
					for (auto& c : m_Chunks)
					{
						if (!c.is_lazy())
						{
							blosc2_schunk_append_chunk(out.get(), reinterpret_cast<uint8_t*>(const_cast<std::byte*>(c.bytes().data())), true);
							continue;
						}
						if (filler.empty())
						{
							std::vector<T> pixels(chunk_elements(), std::get<T>(c.value));
							auto ctx = create_compression_context<T>(out, 1, enums::codec::lz4, 9, m_BlockSize);
							filler.resize(min_compressed_size(m_ChunkSize));
							const size_t n = blosc2::compress<T>(ctx.get(), std::span<const T>(pixels), std::span<std::byte>(filler));
							filler.resize(n);
						}
						blosc2_schunk_append_chunk(out.get(), reinterpret_cast<uint8_t*>(filler.data()), true);
					}
					return out;
				}

				// ---- decode ---------------------------------------------------------------------------------------
				// all chunks -> one vector, ONE engine call for every compressed chunk
				std::vector<T> to_uncompressed(context_ptr& /*decompression_ctx*/) const
				{
					std::vector<T> pixels(size(), fill_value());
					std::vector<batch::target> work;
					work.reserve(m_Chunks.size());
					size_t offset = 0;
					for (const auto& c : m_Chunks)
					{
						if (!c.is_lazy())
							work.push_back({ c.bytes().data(), reinterpret_cast<std::byte*>(pixels.data() + offset), c.num_elements * sizeof(T), c.bytes().size() });
						offset += c.num_elements;
					}
					batch::decompress(work);
					return pixels;
				}

				/// Batch building block: fill the lazy chunks of `pixels` (size() elements) and queue the decode of
				/// every compressed chunk, so that a caller can decode MANY tables with one engine call.
				void plan_decode(T* pixels, std::vector<batch::target>& work) const
				{
					size_t offset = 0;
					for (const auto& c : m_Chunks)
					{
						if (c.is_lazy()) std::fill(pixels + offset, pixels + offset + c.num_elements, std::get<T>(c.value));
						else work.push_back({ c.bytes().data(), reinterpret_cast<std::byte*>(pixels + offset), c.num_elements * sizeof(T), c.bytes().size() });
						offset += c.num_elements;
					}
				}

				/// Same for the chunks [first, first + count): `pixels` receives them back to back.
				void plan_decode_range(T* pixels, size_t first, size_t count, std::vector<batch::target>& work) const
				{
					size_t offset = 0;
					for (size_t i = first; i < first + count; ++i)
					{
						validate_chunk_index(i);
						const auto& c = m_Chunks[i];
						if (c.is_lazy()) std::fill(pixels + offset, pixels + offset + c.num_elements, std::get<T>(c.value));
						else work.push_back({ c.bytes().data(), reinterpret_cast<std::byte*>(pixels + offset), c.num_elements * sizeof(T), c.bytes().size() });
						offset += c.num_elements;
					}
				}

				/// Batch building block of get_region: the rectangle (x, y, w, h) of this table seen as rows of `row_len` elements goes to
				/// `out` (w elements a row, rows `out_pitch` elements apart).  Lazy chunks are filled here for the part of the rectangle
				/// they hold; every run of compressed chunks becomes up to three windows of `job` (a partial first row, the rows wholly
				/// inside the run, a partial last row), so that one engine call serves many tables.
				void plan_region(T* out, size_t out_pitch, size_t row_len, size_t x, size_t y, size_t w, size_t h, batch::window_job& job) const
				{
					if (w == 0 || h == 0) return;
					auto row_start = [&](size_t r) { return (y + r) * row_len + x; };
					size_t cs = 0;
					for (size_t i = 0; i < m_Chunks.size();)
					{
						const bool lazy = m_Chunks[i].is_lazy();
						size_t j = i, ce = cs;
						while (j < m_Chunks.size() && m_Chunks[j].is_lazy() == lazy) { ce += m_Chunks[j].num_elements; ++j; if (lazy) break; }
						// rows [r0, r1) meet the run [cs, ce)
						const size_t r0 = row_start(0) + w > cs ? 0 : (cs - row_start(0) - w) / row_len + 1;
						size_t r1 = h;
						if (row_start(0) >= ce) r1 = 0;
						else if (row_start(h - 1) >= ce) r1 = (ce - row_start(0) + row_len - 1) / row_len;
						if (lazy)
						{
							const T v = std::get<T>(m_Chunks[i].value);
							for (size_t r = r0; r < r1; ++r)
							{
								const size_t a = std::max(row_start(r), cs), b = std::min(row_start(r) + w, ce);
								if (a < b) std::fill(out + r * out_pitch + (a - row_start(r)), out + r * out_pitch + (b - row_start(r)), v);
							}
						}
						else if (r0 < r1)
						{
							const int32_t first = static_cast<int32_t>(job.chunks.size());
							for (size_t k = i; k < j; ++k) { job.chunks.push_back(m_Chunks[k].bytes().data()); job.held.push_back(m_Chunks[k].bytes().size()); }
							auto add = [&](size_t ra, size_t rb, bool partial) {
								if (ra >= rb) return;
								const size_t a = partial ? std::max(row_start(ra), cs) : row_start(ra);
								const size_t b = partial ? std::min(row_start(ra) + w, ce) : a + w;
								cimg_window win{};
								win.chunk_first = first;
								win.chunk_count = static_cast<int32_t>(j - i);
								win.origin = static_cast<int64_t>(a - cs);
								win.row_pitch = static_cast<int64_t>(row_len);
								win.width = static_cast<int32_t>(b - a);
								win.height = static_cast<int32_t>(rb - ra);
								win.out_pitch = static_cast<int64_t>(out_pitch * sizeof(T));
								job.windows.push_back(win);
								job.outs.push_back(reinterpret_cast<std::byte*>(out + ra * out_pitch + (a - row_start(ra))));
							};
							size_t ra = r0, rb = r1;
							if (row_start(ra) < cs) { add(ra, ra + 1, true); ++ra; }
							if (rb > ra && row_start(rb - 1) + w > ce) { --rb; add(rb, rb + 1, true); }
							add(ra, rb, false);
						}
						cs = ce;
						i = j;
					}
				}

				/// The subsampled form: of the rectangle (x, y, w, h), every sy-th row and every sx-th element of those rows (sx, sy >= 1)
				/// go to `out`, ceil(w / sx) elements a row, rows `out_pitch` elements apart.  Runs of chunks become windows as above,
				/// with col_pitch = sx and row_pitch = sy * row_len; a partial row is cut at the first and last sample inside its run.
				void plan_region(T* out, size_t out_pitch, size_t row_len, size_t x, size_t y, size_t w, size_t h, size_t sx, size_t sy,
					batch::strided_window_job& job) const
				{
					if (w == 0 || h == 0) return;
					const size_t ow = (w + sx - 1) / sx, oh = (h + sy - 1) / sy;
					const size_t span = (ow - 1) * sx + 1, rp = sy * row_len;           // elements a sampled row reaches over; between rows
					auto row_start = [&](size_t r) { return (y + r * sy) * row_len + x; };
					size_t cs = 0;
					for (size_t i = 0; i < m_Chunks.size();)
					{
						const bool lazy = m_Chunks[i].is_lazy();
						size_t j = i, ce = cs;
						while (j < m_Chunks.size() && m_Chunks[j].is_lazy() == lazy) { ce += m_Chunks[j].num_elements; ++j; if (lazy) break; }
						// sampled rows [r0, r1) meet the run [cs, ce); of row r, the samples [ca, cb) lie inside it
						const size_t r0 = row_start(0) + span > cs ? 0 : (cs - row_start(0) - span) / rp + 1;
						size_t r1 = oh;
						if (row_start(0) >= ce) r1 = 0;
						else if (row_start(oh - 1) >= ce) r1 = (ce - row_start(0) + rp - 1) / rp;
						auto samples = [&](size_t r, size_t& ca, size_t& cb) {
							const size_t s = row_start(r);
							ca = s >= cs ? 0 : (cs - s + sx - 1) / sx;
							cb = s + span <= ce ? ow : (ce > s ? (ce - s + sx - 1) / sx : 0);
						};
						if (lazy)
						{
							const T v = std::get<T>(m_Chunks[i].value);
							for (size_t r = r0; r < r1; ++r)
							{
								size_t ca, cb;
								samples(r, ca, cb);
								if (ca < cb) std::fill(out + r * out_pitch + ca, out + r * out_pitch + cb, v);
							}
						}
						else if (r0 < r1)
						{
							const int32_t first = job.queue_run(i, j - i, [&](size_t k) { return std::pair(m_Chunks[k].bytes().data(), m_Chunks[k].bytes().size()); });
							auto add = [&](size_t ra, size_t rb, bool partial) {
								if (ra >= rb) return;
								size_t ca = 0, cb = ow;
								if (partial) samples(ra, ca, cb);
								if (ca >= cb) return;                                       // (no sample of the partial row lies in this run)
								cimg_window_strided win{};
								win.chunk_first = first;
								win.chunk_count = static_cast<int32_t>(j - i);
								win.origin = static_cast<int64_t>(row_start(ra) + ca * sx - cs);
								win.row_pitch = static_cast<int64_t>(rp);
								win.col_pitch = static_cast<int64_t>(sx);
								win.width = static_cast<int32_t>(cb - ca);
								win.height = static_cast<int32_t>(rb - ra);
								win.out_pitch = static_cast<int64_t>(out_pitch * sizeof(T));
								job.windows.push_back(win);
								job.outs.push_back(reinterpret_cast<std::byte*>(out + ra * out_pitch + ca));
							};
							size_t ra = r0, rb = r1;
							if (row_start(ra) < cs) { add(ra, ra + 1, true); ++ra; }
							if (rb > ra && row_start(rb - 1) + span > ce) { --rb; add(rb, rb + 1, true); }
							add(ra, rb, false);
						}
						cs = ce;
						i = j;
					}
				}

				/// What set_region changes in a table: the compressed chunks it queued (job index -> chunk index) and the lazy chunks
				/// the rectangle meets, filled and patched on the host.
				struct region_write
				{
					size_t job_first = 0;
					std::vector<size_t> compressed;
					std::vector<size_t> lazy;
					std::vector<std::vector<T>> lazy_pixels;
					std::vector<byte_buffer> new_bytes;              // prepare_region_write: the compressed chunks' new forms (empty: unchanged)
					std::vector<byte_buffer> lazy_bytes;             // ... and the lazy chunks' compressed forms
				};

				/// Batch building block of set_region: the rectangle (x, y, w, h) of this table seen as rows of `row_len` elements is
				/// taken from `src` (w elements a row, rows `src_pitch` elements apart).  Runs of compressed chunks become windows of
				/// `job` as in plan_region; a lazy chunk the rectangle meets is filled with its value and the rectangle's part written in.
				void plan_region_write(const T* src, size_t src_pitch, size_t row_len, size_t x, size_t y, size_t w, size_t h,
					batch::update_job& job, region_write& rw) const
				{
					rw.job_first = job.chunks.size();
					if (w == 0 || h == 0) return;
					auto row_start = [&](size_t r) { return (y + r) * row_len + x; };
					size_t cs = 0;
					for (size_t i = 0; i < m_Chunks.size();)
					{
						const bool lazy = m_Chunks[i].is_lazy();
						size_t j = i, ce = cs;
						while (j < m_Chunks.size() && m_Chunks[j].is_lazy() == lazy) { ce += m_Chunks[j].num_elements; ++j; if (lazy) break; }
						const size_t r0 = row_start(0) + w > cs ? 0 : (cs - row_start(0) - w) / row_len + 1;
						size_t r1 = h;
						if (row_start(0) >= ce) r1 = 0;
						else if (row_start(h - 1) >= ce) r1 = (ce - row_start(0) + row_len - 1) / row_len;
						bool met = false;
						for (size_t r = r0; r < r1 && !met; ++r) met = std::max(row_start(r), cs) < std::min(row_start(r) + w, ce);
						if (lazy && met)
						{
							std::vector<T> px(m_Chunks[i].num_elements, std::get<T>(m_Chunks[i].value));
							for (size_t r = r0; r < r1; ++r)
							{
								const size_t a = std::max(row_start(r), cs), b = std::min(row_start(r) + w, ce);
								if (a < b) std::copy(src + r * src_pitch + (a - row_start(r)), src + r * src_pitch + (b - row_start(r)), px.begin() + (a - cs));
							}
							rw.lazy.push_back(i);
							rw.lazy_pixels.push_back(std::move(px));
						}
						else if (!lazy && met)
						{
							const int32_t first = static_cast<int32_t>(job.chunks.size());
							for (size_t k = i; k < j; ++k)
							{
								job.chunks.push_back(m_Chunks[k].bytes().data());
								job.held.push_back(m_Chunks[k].bytes().size());
								job.destsize.push_back(static_cast<int32_t>(min_compressed_size(m_ChunkSize)));
								rw.compressed.push_back(k);
							}
							auto add = [&](size_t ra, size_t rb, bool partial) {
								if (ra >= rb) return;
								const size_t a = partial ? std::max(row_start(ra), cs) : row_start(ra);
								const size_t b = partial ? std::min(row_start(ra) + w, ce) : a + w;
								cimg_window win{};
								win.chunk_first = first;
								win.chunk_count = static_cast<int32_t>(j - i);
								win.origin = static_cast<int64_t>(a - cs);
								win.row_pitch = static_cast<int64_t>(row_len);
								win.width = static_cast<int32_t>(b - a);
								win.height = static_cast<int32_t>(rb - ra);
								win.out_pitch = static_cast<int64_t>(src_pitch * sizeof(T));
								job.windows.push_back(win);
								job.srcs.push_back(reinterpret_cast<const std::byte*>(src + ra * src_pitch + (a - row_start(ra))));
							};
							size_t ra = r0, rb = r1;
							if (row_start(ra) < cs) { add(ra, ra + 1, true); ++ra; }
							if (rb > ra && row_start(rb - 1) + w > ce) { --rb; add(rb, rb + 1, true); }
							add(ra, rb, false);
						}
						cs = ce;
						i = j;
					}
				}

				/// One subsampled rectangle of set_regions: nx x ny samples, sx / sy apart, from (x, y); its data (nx elements a row) starts
				/// at element src_off of the call's source.
				struct strided_rect { size_t x, y, nx, ny, sx, sy, src_off; };

				/// Batch building block of set_regions: the rectangles, in order, written into this table seen as rows of `row_len`
				/// elements.  Every run of compressed chunks that holds a sample becomes a plane of `job` with strided windows in region
				/// order (a later region wins); a lazy chunk that holds a sample is filled with its value and patched on the host, with
				/// stride and in region order.  (Template over the job so that only callers refer to the strided entry point's types.)
				template <typename Job>
				void plan_regions_write(const T* src, const std::vector<strided_rect>& rects, size_t row_len, Job& job, region_write& rw) const
				{
					rw.job_first = job.chunks.size();
					size_t cs = 0;
					for (size_t i = 0; i < m_Chunks.size();)
					{
						const bool lazy = m_Chunks[i].is_lazy();
						size_t j = i, ce = cs;
						while (j < m_Chunks.size() && m_Chunks[j].is_lazy() == lazy) { ce += m_Chunks[j].num_elements; ++j; if (lazy) break; }
						const int32_t first = static_cast<int32_t>(job.chunks.size());
						std::vector<T> px;
						bool met = false;
						std::vector<cimg_window_strided> wins;
						std::vector<const std::byte*> srcs;
						for (const strided_rect& q : rects)
						{
							if (q.nx == 0 || q.ny == 0 || ce == cs) continue;
							const size_t base = q.y * row_len + q.x, stride = q.sy * row_len, reach = (q.nx - 1) * q.sx;   // a row's samples: [rs, rs + reach]
							const size_t r_lo = cs <= base + reach ? 0 : (cs - base - reach + stride - 1) / stride;
							const size_t r_hi = base >= ce ? 0 : std::min(q.ny, (ce - 1 - base) / stride + 1);
							// rows r_lo .. r_hi - 1 may hold samples of the run; only the first and the last of them can be cut by its ends
							auto cols = [&](size_t r, size_t& c_lo, size_t& c_hi) {
								const size_t rs = base + r * stride;
								c_lo = rs >= cs ? 0 : (cs - rs + q.sx - 1) / q.sx;
								c_hi = std::min(q.nx - 1, (ce - 1 - rs) / q.sx);
								return c_lo <= c_hi && c_lo < q.nx;
							};
							auto emit = [&](size_t ra, size_t rb, size_t c_lo, size_t c_hi) {
								met = true;
								if (lazy)
								{
									if (px.empty()) px.assign(m_Chunks[i].num_elements, std::get<T>(m_Chunks[i].value));
									for (size_t r = ra; r < rb; ++r)
										for (size_t c = c_lo; c <= c_hi; ++c) px[base + r * stride + c * q.sx - cs] = src[q.src_off + r * q.nx + c];
									return;
								}
								cimg_window_strided win{};
								win.chunk_first = first;
								win.chunk_count = static_cast<int32_t>(j - i);
								win.origin = static_cast<int64_t>(base + ra * stride + c_lo * q.sx - cs);
								win.row_pitch = static_cast<int64_t>(stride);
								win.col_pitch = static_cast<int64_t>(q.sx);
								win.width = static_cast<int32_t>(c_hi - c_lo + 1);
								win.height = static_cast<int32_t>(rb - ra);
								win.out_pitch = static_cast<int64_t>(q.nx * sizeof(T));
								wins.push_back(win);
								srcs.push_back(reinterpret_cast<const std::byte*>(src + q.src_off + ra * q.nx + c_lo));
							};
							size_t ra = r_lo, rb = r_hi, c_lo = 0, c_hi = 0;
							if (ra < rb) { if (cols(ra, c_lo, c_hi)) { if (c_lo > 0 || c_hi < q.nx - 1 || rb - ra == 1) { emit(ra, ra + 1, c_lo, c_hi); ++ra; } } else ++ra; }
							if (ra < rb) { if (cols(rb - 1, c_lo, c_hi)) { if (c_lo > 0 || c_hi < q.nx - 1) { emit(rb - 1, rb, c_lo, c_hi); --rb; } } else --rb; }
							if (ra < rb) emit(ra, rb, 0, q.nx - 1);
						}
						if (met && lazy)
						{
							rw.lazy.push_back(i);
							rw.lazy_pixels.push_back(std::move(px));
						}
						else if (met)
						{
							for (size_t k = i; k < j; ++k)
							{
								job.chunks.push_back(m_Chunks[k].bytes().data());
								job.held.push_back(m_Chunks[k].bytes().size());
								job.destsize.push_back(static_cast<int32_t>(min_compressed_size(m_ChunkSize)));
								rw.compressed.push_back(k);
							}
							job.windows.insert(job.windows.end(), wins.begin(), wins.end());
							job.srcs.insert(job.srcs.end(), srcs.begin(), srcs.end());
						}
						cs = ce;
						i = j;
					}
				}

				/// One rectangle of fill_regions / the masked set_regions: a strided_rect whose data (if the call has a source) starts at
				/// r.src_off, whose mask bytes (if the call has a mask) start at mask_off, and whose value (if the call has no source) is
				/// `value`.  An image's channels share the mask: their rects differ in src_off and value, not in mask_off.
				struct masked_rect { strided_rect r; size_t mask_off; T value; };

				/// Batch building block of fill_regions and the masked set_regions: plan_regions_write over cimg_window_masked.  src null:
				/// every rectangle is painted with its value and no source is named; mask null: every sample is written.  A lazy chunk
				/// that holds a sample is filled with its value and patched on the host under the same mask, in region order.  (Template
				/// over the job so that only callers refer to the masked entry point's types.)
				template <typename Job>
				void plan_regions_write_masked(const T* src, const uint8_t* mask, const std::vector<masked_rect>& rects, size_t row_len, Job& job,
					region_write& rw) const
				{
					rw.job_first = job.chunks.size();
					size_t cs = 0;
					for (size_t i = 0; i < m_Chunks.size();)
					{
						const bool lazy = m_Chunks[i].is_lazy();
						size_t j = i, ce = cs;
						while (j < m_Chunks.size() && m_Chunks[j].is_lazy() == lazy) { ce += m_Chunks[j].num_elements; ++j; if (lazy) break; }
						const int32_t first = static_cast<int32_t>(job.chunks.size());
						std::vector<T> px;
						bool met = false;
						std::vector<cimg_window_masked> wins;
						std::vector<const std::byte*> srcs;
						std::vector<const uint8_t*> masks;
						for (const masked_rect& mr : rects)
						{
							const strided_rect& q = mr.r;
							if (q.nx == 0 || q.ny == 0 || ce == cs) continue;
							const size_t base = q.y * row_len + q.x, stride = q.sy * row_len, reach = (q.nx - 1) * q.sx;   // a row's samples: [rs, rs + reach]
							const size_t r_lo = cs <= base + reach ? 0 : (cs - base - reach + stride - 1) / stride;
							const size_t r_hi = base >= ce ? 0 : std::min(q.ny, (ce - 1 - base) / stride + 1);
							auto cols = [&](size_t r, size_t& c_lo, size_t& c_hi) {
								const size_t rs = base + r * stride;
								c_lo = rs >= cs ? 0 : (cs - rs + q.sx - 1) / q.sx;
								c_hi = std::min(q.nx - 1, (ce - 1 - rs) / q.sx);
								return c_lo <= c_hi && c_lo < q.nx;
							};
							auto emit = [&](size_t ra, size_t rb, size_t c_lo, size_t c_hi) {
								met = true;
								if (lazy)
								{
									if (px.empty()) px.assign(m_Chunks[i].num_elements, std::get<T>(m_Chunks[i].value));
									for (size_t r = ra; r < rb; ++r)
										for (size_t c = c_lo; c <= c_hi; ++c)
											if (!mask || mask[mr.mask_off + r * q.nx + c]) px[base + r * stride + c * q.sx - cs] = src ? src[q.src_off + r * q.nx + c] : mr.value;
									return;
								}
								cimg_window_masked win{};
								win.chunk_first = first;
								win.chunk_count = static_cast<int32_t>(j - i);
								win.origin = static_cast<int64_t>(base + ra * stride + c_lo * q.sx - cs);
								win.row_pitch = static_cast<int64_t>(stride);
								win.col_pitch = static_cast<int64_t>(q.sx);
								win.width = static_cast<int32_t>(c_hi - c_lo + 1);
								win.height = static_cast<int32_t>(rb - ra);
								if (src) win.out_pitch = static_cast<int64_t>(q.nx * sizeof(T));
								else
								{
									static_assert(sizeof(T) <= sizeof(win.value), "a constant has at most 8 bytes");
									win.flags |= CIMG_WM_CONST;
									std::memcpy(win.value, &mr.value, sizeof(T));
								}
								if (mask) { win.flags |= CIMG_WM_MASK; win.mask_pitch = static_cast<int64_t>(q.nx); }
								wins.push_back(win);
								srcs.push_back(src ? reinterpret_cast<const std::byte*>(src + q.src_off + ra * q.nx + c_lo) : nullptr);
								masks.push_back(mask ? mask + mr.mask_off + ra * q.nx + c_lo : nullptr);
							};
							size_t ra = r_lo, rb = r_hi, c_lo = 0, c_hi = 0;
							if (ra < rb) { if (cols(ra, c_lo, c_hi)) { if (c_lo > 0 || c_hi < q.nx - 1 || rb - ra == 1) { emit(ra, ra + 1, c_lo, c_hi); ++ra; } } else ++ra; }
							if (ra < rb) { if (cols(rb - 1, c_lo, c_hi)) { if (c_lo > 0 || c_hi < q.nx - 1) { emit(rb - 1, rb, c_lo, c_hi); --rb; } } else --rb; }
							if (ra < rb) emit(ra, rb, 0, q.nx - 1);
						}
						if (met && lazy)
						{
							rw.lazy.push_back(i);
							rw.lazy_pixels.push_back(std::move(px));
						}
						else if (met)
						{
							for (size_t k = i; k < j; ++k)
							{
								job.chunks.push_back(m_Chunks[k].bytes().data());
								job.held.push_back(m_Chunks[k].bytes().size());
								job.destsize.push_back(static_cast<int32_t>(min_compressed_size(m_ChunkSize)));
								rw.compressed.push_back(k);
							}
							job.windows.insert(job.windows.end(), wins.begin(), wins.end());
							job.srcs.insert(job.srcs.end(), srcs.begin(), srcs.end());
							job.masks.insert(job.masks.end(), masks.begin(), masks.end());
						}
						cs = ce;
						i = j;
					}
				}

				/// After the engine call succeeded: take this table's new chunks out of the call's results and compress the patched lazy
				/// chunks (one batch call).  May throw; nothing of the table has changed yet.
				void prepare_region_write(context_raw_ptr cctx, region_write& rw, std::vector<std::vector<std::byte>>& made) const
				{
					for (size_t k = 0; k < rw.compressed.size(); ++k)
					{
						auto& b = made[rw.job_first + k];
						rw.new_bytes.push_back(b.empty() ? byte_buffer() : byte_buffer(std::move(b)));
					}
					if (rw.lazy.empty()) return;
					std::vector<batch::piece> pieces;
					for (const auto& px : rw.lazy_pixels) pieces.push_back({ reinterpret_cast<const std::byte*>(px.data()), px.size() * sizeof(T) });
					rw.lazy_bytes = batch::compress(cctx, pieces, m_ChunkSize);
				}

				/// Replace every touched chunk: moves only, so a caller that prepared every table commits them all.
				void commit_region_write(region_write& rw) noexcept
				{
					for (size_t k = 0; k < rw.compressed.size(); ++k)
						if (rw.new_bytes[k].size() > 0) m_Chunks[rw.compressed[k]].value = std::move(rw.new_bytes[k]);
					for (size_t k = 0; k < rw.lazy.size(); ++k) m_Chunks[rw.lazy[k]].value = std::move(rw.lazy_bytes[k]);
				}

				std::vector<T> chunk(context_ptr& ctx, size_t index) const { return chunk(ctx.get(), index); }
				std::vector<T> chunk(context_raw_ptr ctx, size_t index) const
				{
					validate_chunk_index(index);
					std::vector<T> pixels(chunk_elements(index));
					chunk(ctx, std::span<T>(pixels), index);
					return pixels;
				}
				void chunk(context_ptr& ctx, std::span<T> buffer, size_t index) const { chunk(ctx.get(), buffer, index); }
				void chunk(context_raw_ptr ctx, std::span<T> buffer, size_t index) const
				{
					validate_chunk_index(index);
					const auto& c = m_Chunks[index];
					if (buffer.size() < c.num_elements)
						throw std::invalid_argument(compressed::detail::text("Unable to decompress chunk at idx ", index,
							" into buffer as the buffer needs to at least have the size ", c.num_elements, ". Instead got ", buffer.size()));
					if (c.is_lazy())
						std::fill(buffer.begin(), buffer.end(), std::get<T>(c.value));
					else
						blosc2::decompress(ctx, buffer, std::span<const std::byte>(c.bytes().data(), c.bytes().size()));
				}

				// ---- replace / append -----------------------------------------------------------------------------
				void set_chunk(std::vector<std::byte> compressed, size_t index)
				{
					validate_chunk_index(index);
					const size_t n = chunk_num_elements<T>(compressed);
					m_Chunks[index].value = byte_buffer(std::move(compressed));
					m_Chunks[index].num_elements = n;
					validate_chunk_sizes();
				}
				void set_chunk(byte_buffer compressed, size_t index)
				{
					validate_chunk_index(index);
					const size_t n = chunk_num_elements<T>(std::span<const std::byte>(compressed.data(), compressed.size()));
					m_Chunks[index].value = std::move(compressed);
					m_Chunks[index].num_elements = n;
					validate_chunk_sizes();
				}
				void set_chunk(std::span<const std::byte> compressed, size_t index)
				{
					set_chunk(std::vector<std::byte>(compressed.begin(), compressed.end()), index);
				}
				void set_chunk(context_ptr& compression_ctx, std::span<T> uncompressed, size_t index)
				{
					validate_chunk_index(index);
					util::default_init_vector<std::byte> scratch(min_compressed_size(m_ChunkSize));
					const size_t n = blosc2::compress<T>(compression_ctx.get(), std::span<const T>(uncompressed.data(), uncompressed.size()), std::span<std::byte>(scratch.data(), scratch.size()));
					m_Chunks[index].value = byte_buffer(std::vector<std::byte>(scratch.begin(), scratch.begin() + n));
					m_Chunks[index].num_elements = uncompressed.size();
					validate_chunk_sizes();
				}

				void append_chunk(std::vector<std::byte> compressed)
				{
					const size_t n = chunk_num_elements<T>(compressed);
					m_Chunks.push_back(slot{ byte_buffer(std::move(compressed)), n });
					validate_chunk_sizes();
				}
				void append_chunk(byte_buffer compressed)
				{
					const size_t n = chunk_num_elements<T>(std::span<const std::byte>(compressed.data(), compressed.size()));
					m_Chunks.push_back(slot{ std::move(compressed), n });
					validate_chunk_sizes();
				}
				void append_chunk(context_ptr& compression_ctx, std::span<T> uncompressed)
				{
					util::default_init_vector<std::byte> scratch(min_compressed_size(m_ChunkSize));
					append_chunk(compression_ctx, uncompressed, std::span<std::byte>(scratch.data(), scratch.size()));
				}
				void append_chunk(context_ptr& compression_ctx, std::span<T> uncompressed, std::span<std::byte> compression_buff)
				{
					if (compression_buff.size() < min_compressed_size(m_ChunkSize))
						throw std::runtime_error(compressed::detail::text("Error while appending chunk to super-chunk. Expected compression buffer to be at least ",
							min_compressed_size(m_ChunkSize), " bytes but instead we got ", compression_buff.size(), " bytes"));
					const size_t n = blosc2::compress<T>(compression_ctx.get(), std::span<const T>(uncompressed.data(), uncompressed.size()), compression_buff);
					m_Chunks.push_back(slot{ byte_buffer(std::vector<std::byte>(compression_buff.begin(), compression_buff.begin() + n)), uncompressed.size() });
					validate_chunk_sizes();
				}
				// many chunks at once (one engine call): what image::read-style producers should use
				void append_chunks(context_ptr& compression_ctx, std::span<const T> pixels)
				{
					auto made = compress_pieces(compression_ctx.get(), pixels);
					for (auto& m : made) m_Chunks.push_back(std::move(m));
					validate_chunk_sizes();
				}

			protected:
				std::vector<slot> m_Chunks{};
				size_t m_ChunkSize = s_default_chunksize;
				size_t m_BlockSize = s_default_blocksize;

				static size_t elements_of(size_t bytes)
				{
					if (bytes % sizeof(T) != 0)
						throw std::runtime_error(compressed::detail::text("Internal Error: The chunk byte size is not cleanly divisible by the sizeof T."
							" Chunk size is ", bytes, " while sizeof(T) is ", sizeof(T)));
					return bytes / sizeof(T);
				}

				T fill_value() const noexcept
				{
					for (const auto& c : m_Chunks) if (c.is_lazy()) return std::get<T>(c.value);
					return T{};
				}

				void validate_chunk_index(size_t index) const
				{
					if (index >= m_Chunks.size())
						throw std::out_of_range(compressed::detail::text("Cannot access index ", index, " in schunk. Total amount of chunks is ", m_Chunks.size()));
				}

				// all chunks but the last hold exactly m_ChunkSize bytes; the last at most that (reference schunk_mixin.h:216-246)
				void validate_chunk_sizes() const
				{
					if (m_Chunks.empty()) return;
					for (size_t i = 0; i + 1 < m_Chunks.size(); ++i)
						if (m_Chunks[i].byte_size() != m_ChunkSize)
							throw std::invalid_argument(compressed::detail::text("Error while validating chunk sizes; Expected all chunks to have a size equivalent to ",
								m_ChunkSize, " (m_ChunkSize). However, chunk ", i, " instead has a chunk size of ", m_Chunks[i].byte_size(),
								". Having a size different from the rest of the chunks is only supported for the last chunk (blosc2 limitation)."));
					if (m_Chunks.back().byte_size() > m_ChunkSize)
						throw std::runtime_error(compressed::detail::text("Error while validating chunk sizes; Expected the last chunk to be at most ",
							m_ChunkSize, " bytes, instead got ", m_Chunks.back().byte_size(), " bytes."));
				}

				// cut `pixels` into full chunks + remainder (reference schunk.h:79-104) and compress them in one call
				std::vector<slot> compress_pieces(context_raw_ptr cctx, std::span<const T> pixels) const
				{
					const size_t total = pixels.size() * sizeof(T);
					const auto* base = reinterpret_cast<const std::byte*>(pixels.data());
					std::vector<batch::piece> pieces;
					for (size_t off = 0; off < total; off += m_ChunkSize)
						pieces.push_back({ base + off, std::min(m_ChunkSize, total - off) });
					auto bytes = batch::compress(cctx, pieces, m_ChunkSize);
					std::vector<slot> out;
					out.reserve(bytes.size());
					for (size_t i = 0; i < bytes.size(); ++i)
						out.push_back(slot{ std::move(bytes[i]), pieces[i].nbytes / sizeof(T) });
					return out;
				}
			};
		} // detail

		/// Every chunk compressed (reference: compressed/blosc2/schunk.h).
		template <typename T>
		struct schunk final : public detail::chunk_table<T, false>
		{
			schunk() = default;
			/// empty table with a geometry, to be filled with append_chunk (reference schunk.h:50-55)
			schunk(size_t block_size, size_t chunk_size)
			{
				util::validate_chunk_size<T>(chunk_size, "schunk");
				this->m_ChunkSize = chunk_size;
				this->m_BlockSize = block_size;
			}
			/// compress `data` (reference schunk.h:65-105); one batched engine call for all chunks
			schunk(std::span<const T> data, size_t block_size, size_t chunk_size, context_ptr& compression_ctx)
			{
				util::validate_chunk_size<T>(chunk_size, "schunk");
				this->m_BlockSize = block_size;
				this->m_ChunkSize = chunk_size;
				this->m_Chunks = this->compress_pieces(compression_ctx.get(), data);
			}
		};

		/// Chunks start as a single fill value and become real on set_chunk (reference: compressed/blosc2/lazyschunk.h).
		template <typename T>
		struct lazy_schunk final : public detail::chunk_table<T, true>
		{
			lazy_schunk() = default;
			lazy_schunk(T value, size_t num_elements, size_t block_size, size_t chunk_size)
			{
				util::validate_chunk_size<T>(chunk_size, "lazy_schunk");
				this->m_BlockSize = block_size;
				this->m_ChunkSize = chunk_size;
				const size_t total = num_elements * sizeof(T);
				for (size_t off = 0; off < total; off += chunk_size)
					this->m_Chunks.push_back(detail::lazy_chunk<T>{ value, std::min(chunk_size, total - off) / sizeof(T) });
			}
		};

		template <typename T> using schunk_var = std::variant<schunk<T>, lazy_schunk<T>>;
		template <typename T> using schunk_var_ptr = std::shared_ptr<schunk_var<T>>;
	} // blosc2
} // NAMESPACE_COMPRESSED_IMAGE
