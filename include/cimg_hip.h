/*
 * cimg_hip.h -- C ABI of libcimg_hip.so, the MI355X (gfx950) chunk codec engine.
 *
 * Two groups of entry points:
 *
 *  (1) include/blosc2.h -- the eleven c-blosc2 symbols the reference binds
 *      (compressed/blosc2/wrapper.h, blosc2/util.h, blosc2/schunk.h:113), same names and argument
 *      meaning, so the reference's own headers link against this library instead of c-blosc2.
 *
 *  (2) this header -- the *batched* extension.  One blosc2_compress_ctx call is one <= 4 MiB chunk
 *      (wrapper.h:139,172), far too little to fill 256 CUs; the reference's loops over chunks
 *      (schunk.h:85-104, schunk.h:130-138) and over channels (image.h:119-159, 1307-1315) become one
 *      call here.  Plain pointers and sizes only; no HIP or torch types.
 *
 * All functions return 0 (or a non-negative size) on success and a negative c-blosc2 error code
 * (include/blosc2.h, BLOSC2_ERROR_*) on failure; cimg_last_error() gives the text.  Every call takes
 * the engine's own (recursive) lock, so calls from several threads are serialised, not interleaved;
 * a _begin / _fetch pair is made one unit by holding cimg_engine_lock() across it.  (The reference's
 * contexts are not thread-safe at all, channel.h:511-513.)
 */
#ifndef CIMG_HIP_H
#define CIMG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cimg_engine cimg_engine;

/* Mirrors the blosc2_cparams fields the reference sets (wrapper.h:325-332, 350-356) plus the filter
 * pipeline it inherits from BLOSC2_CPARAMS_DEFAULTS. */
typedef struct cimg_cparams {
    int32_t typesize;        /* sizeof(T) */
    int32_t clevel;          /* 0..9 */
    int32_t blocksize;       /* bytes; constants.h:11 default 32768 */
    int32_t compcode;        /* BLOSC_LZ4 = 1, BLOSC_BLOSCLZ = 0: the CPU codec's bytes; BLOSC_LZ4HC = 2, BLOSC_ZSTD = 5: format-valid
                              * streams (any LZ4 / zstd decoder reads them), NOT liblz4-HC's / libzstd's bytes.  BLOSC_ZLIB: refused. */
    int32_t splitmode;       /* BLOSC_AUTO_SPLIT = 3 */
    uint8_t filters[6];      /* default {0,0,0,0,0,BLOSC_SHUFFLE}.  filters[5]: none / shuffle / bitshuffle.  filters[4] may be
                              * BLOSC_TRUNC_PREC = 4 (filters[0..3] == 0): every compress call then zeroes the low mantissa bits of the
                              * pixels first (a caller's device pixels are left alone: the truncated copy lives in engine scratch) */
    uint8_t filters_meta[6]; /* filters_meta[4], as int8 m: m > 0 mantissa bits kept, m < 0 bits zeroed; typesize 2 / 4 / 8 = IEEE
                              * binary16 / 32 / 64.  m == 0, |m| above the mantissa width, nothing kept, or another typesize:
                              * BLOSC2_ERROR_INVALID_PARAM before anything runs */
} cimg_cparams;

void cimg_cparams_init(cimg_cparams* p, int32_t typesize);   /* the reference's defaults: lz4, level 9, 32 KiB blocks */

/* ---- engine ---------------------------------------------------------------------------------------- */
int  cimg_engine_create(int device, cimg_engine** out);      /* device < 0: current device */
void cimg_engine_destroy(cimg_engine* e);
const char* cimg_last_error(const cimg_engine* e);            /* e may be NULL: last create() failure */
int  cimg_engine_synchronize(cimg_engine* e);
/* Every batch call takes the engine's (recursive) lock for its own duration.  A caller that needs two calls to act as
 * one -- _begin followed by _fetch below -- brackets them with these, on the same thread. */
void cimg_engine_lock(cimg_engine* e);
void cimg_engine_unlock(cimg_engine* e);
/* The hipStream_t the engine's work is ordered on.  A batch call behaves as if everything it does were enqueued there, in order:
 * work the caller put on this stream before the call (a kernel producing the pixels, cimg_deinterleave_device) is seen by the
 * batch, work put there after a _begin call follows the batch.  (Internally a batch may run one of its launches on a second
 * stream beside the first -- the leftover blocks of chunks that are no multiple of the block size --; that stream is made to
 * wait for everything this one holds when the batch is enqueued, and this one for it before the batch ends.)
 * An encode launch is persistent: it is sized to fill the device, and it completes with any number of its workgroups resident
 * (two engines, or two processes, sharing one card slow each other down; they do not wait for each other). */
void* cimg_engine_stream(cimg_engine* e);

/* ---- device-resident batches -----------------------------------------------------------------------
 * Chunk i's pixels live at d_raw + raw_off[i] (nbytes[i] bytes), its blosc2 chunk at
 * d_comp + comp_off[i] with capacity destsize[i] (what the reference passes as the dest span:
 * nominal chunk size + BLOSC2_MAX_OVERHEAD, schunk.h:73).  Offset / size arrays are HOST arrays.
 * cbytes[i] receives what blosc2_compress_ctx would return for that chunk (0 = does not fit).
 * One encode launch per kind of block (split into byte planes / unsplit) does everything: the waves that encoded a chunk also
 * lay it out and copy it into place.
 * The call returns after the results are on the host (one stream sync). */
int cimg_compress_batch_device(cimg_engine* e, const cimg_cparams* p, int32_t nchunks,
                               const void* d_raw, const int64_t* raw_off, const int32_t* nbytes,
                               void* d_comp, const int64_t* comp_off, const int32_t* destsize,
                               int32_t* cbytes);
/* nbytes[i] / blocksize[i] are the values in chunk i's header (blosc2_cbuffer_sizes); status[i]
 * receives 0 or the blosc2 error code of that chunk. Returns the first non-zero status, or 0.
 * Chunks of codec format 0 (blosclz), 1 (lz4, lz4hc) and 4 (zstd: a slow path, launched only when such a
 * chunk is in the batch) decode; any other format is BLOSC2_ERROR_CODEC_SUPPORT for that chunk. */
int cimg_decompress_batch_device(cimg_engine* e, int32_t nchunks,
                                 const void* d_comp, const int64_t* comp_off,
                                 const int32_t* nbytes, const int32_t* blocksize,
                                 void* d_raw, const int64_t* raw_off, int32_t* status);

/* The same in two steps: _begin enqueues the kernels on the engine's stream and returns at once, _fetch waits for them
 * and hands over the results.  ONE compress batch and ONE decompress batch may be in flight together, and a decompress
 * _begin may follow the compress _begin of the chunks it reads directly (stream order: it sees them finished; nbytes /
 * blocksize are the caller's, nothing of the compress results is needed on the host) -- so the host's share of a round
 * trip (planning, launches, the wait) hides behind the kernels instead of leaving the GPU idle between the calls.
 * Each _fetch refers to the most recent _begin of its kind and delivers it once.  The engine keeps ONE result area per kind, so
 * a call in between that does work of the same kind overwrites it and voids the pending _begin (its _fetch then fails with
 * BLOSC2_ERROR_INVALID_PARAM and writes nothing):
 *   - a pending compress _begin is voided by every call that compresses: cimg_compress_batch_device, the host-resident
 *     compress calls (cimg_compress_batch_host, _host_begin, _host_packed, _host_interleaved_begin),
 *     cimg_compress_batch_device_packed_begin and the window writes (cimg_update_windows_*);
 *   - a pending decompress _begin by every call that decompresses: cimg_decompress_batch_device(_sized),
 *     cimg_decompress_batch_host(_sized), the window reads (cimg_decompress_windows_*) and the window writes.
 * A call of the other kind leaves it valid, and so do the calls that do neither (deinterleave, interleave, pack, wait_stream,
 * timing, stamps).  A _begin ALWAYS replaces what its slot held, also when it is refused or has nchunks <= 0 (then a batch of no
 * chunks is in flight: a _fetch naming the earlier count fails).  Of the other calls, only these refused ones are promised to
 * void nothing: a plain device call (cimg_compress_batch_device, cimg_decompress_batch_device(_sized)) with nchunks <= 0 or a
 * missing array argument, and a host-resident call with nchunks <= 0 or without its destination (h_comp / comp_off, alloc /
 * chunk_ptr).  Any other refused call -- by the planner, by a header check, for a missing p or size array of a host-resident
 * call, which has claimed the staging area by then -- may void like a call of its kind.  A compress _fetch that names
 * another chunk count than the batch in flight fails and leaves it in flight.
 * Threads sharing an engine hold cimg_engine_lock from _begin to _fetch. */
int cimg_compress_batch_device_begin(cimg_engine* e, const cimg_cparams* p, int32_t nchunks,
                                     const void* d_raw, const int64_t* raw_off, const int32_t* nbytes,
                                     void* d_comp, const int64_t* comp_off, const int32_t* destsize);
int cimg_compress_batch_device_fetch(cimg_engine* e, int32_t nchunks, int32_t* cbytes);
int cimg_decompress_batch_device_begin(cimg_engine* e, int32_t nchunks,
                                       const void* d_comp, const int64_t* comp_off,
                                       const int32_t* nbytes, const int32_t* blocksize,
                                       void* d_raw, const int64_t* raw_off);
int cimg_decompress_batch_device_fetch(cimg_engine* e, int32_t* status);
/* Device-resident decode for callers that know how many bytes each compressed buffer really holds (comp_size[i]; at least 32).
 * The reference passes INT32_MAX as srcsize (blosc2/wrapper.h:249), so the callee is the one that must be careful: a header
 * whose cbytes exceeds comp_size[i] gets BLOSC2_ERROR_READ_BUFFER for that chunk and the kernels read nothing of it behind
 * the 32-byte header (the unsized calls above trust the header's cbytes).  Otherwise as the unsized calls. */
int cimg_decompress_batch_device_sized(cimg_engine* e, int32_t nchunks,
                                       const void* d_comp, const int64_t* comp_off, const int32_t* comp_size,
                                       const int32_t* nbytes, const int32_t* blocksize,
                                       void* d_raw, const int64_t* raw_off, int32_t* status);
int cimg_decompress_batch_device_begin_sized(cimg_engine* e, int32_t nchunks,
                                             const void* d_comp, const int64_t* comp_off, const int32_t* comp_size,
                                             const int32_t* nbytes, const int32_t* blocksize,
                                             void* d_raw, const int64_t* raw_off);

/* ---- interleaved pixels -> planes (reference: image_algo::deinterleave, compressed/image_algo.h:84-111, the step between
 * reading scanlines and compressing them in the read path, image.h:1880) -------------------------------------------
 * d_interleaved holds npixels * nchannels elements of `typesize` bytes (R G B A R G B A ...); channel c comes out as
 * npixels elements at d_planar + c * plane_stride.  plane_stride is in bytes, a multiple of 16, at least npixels * typesize;
 * both buffers are 16-byte aligned device memory.  typesize is 1, 2, 4 or 8.  Returns when the kernel is enqueued on the
 * engine's stream (later calls on the same engine see its result). */
int cimg_deinterleave_device(cimg_engine* e, const void* d_interleaved, int32_t nchannels, int32_t typesize, int64_t npixels,
                             void* d_planar, int64_t plane_stride);
/* The producer path in one call: interleaved scanlines in HOST memory are uploaded once, split into planes on the device
 * and compressed from there.  Chunk i covers nbytes[i] bytes at offset raw_off[i] of the PLANAR layout, in which channel c
 * occupies [c * plane_stride, c * plane_stride + npixels * typesize) with plane_stride = npixels * typesize rounded up to
 * 16.  Otherwise as cimg_compress_batch_host_begin: the chunks stay on the device, cbytes[] comes back, and
 * cimg_compress_batch_host_fetch delivers them. */
int cimg_compress_batch_host_interleaved_begin(cimg_engine* e, const cimg_cparams* p, int32_t nchannels, int64_t npixels,
                                               const void* h_interleaved, int32_t nchunks, const int64_t* raw_off,
                                               const int32_t* nbytes, const int32_t* destsize, int32_t* cbytes);

/* ---- host-resident batches (H2D + kernels + D2H inside) ------------------------------------------ */
int cimg_compress_batch_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks,
                             const void* h_raw, const int64_t* raw_off, const int32_t* nbytes,
                             void* h_comp, const int64_t* comp_off, const int32_t* destsize,
                             int32_t* cbytes);
/* The same in two steps, for host code that wants to allocate the chunks' final storage with their exact sizes:
 * _begin uploads and compresses (the chunks stay in the engine's device staging area) and reports cbytes[];
 * _fetch copies chunk i (cbytes[i] bytes) to h_comp + comp_off[i] and synchronizes.  _fetch refers to the most
 * recent _begin on this engine that staged a batch -- this one, _host_interleaved_begin or
 * cimg_compress_batch_device_packed_begin: they share one staging area -- and delivers it once.  A call in between that
 * reuses the staging area voids it (the _fetch fails with BLOSC2_ERROR_INVALID_PARAM and writes nothing): every
 * host-resident batch call (compress or decompress), every host-resident window read or write, and
 * cimg_compress_batch_device_packed_begin.  The device-resident calls (cimg_compress_batch_device and its _begin / _fetch,
 * cimg_decompress_batch_device*, the device window reads and writes, pack, interleave, deinterleave) do not touch the staging
 * area: the staged chunks are intact and the _fetch stays valid.  A staging _begin always replaces the staged batch, also with
 * nchunks <= 0 or when it is refused (nothing is staged then); which other refused calls void nothing is said with the device
 * pair above.  A _fetch that names another chunk count than the staged batch fails and leaves it staged. */
int cimg_compress_batch_host_begin(cimg_engine* e, const cimg_cparams* p, int32_t nchunks,
                                   const void* h_raw, const int64_t* raw_off, const int32_t* nbytes,
                                   const int32_t* destsize, int32_t* cbytes);
int cimg_compress_batch_host_fetch(cimg_engine* e, int32_t nchunks, void* h_comp, const int64_t* comp_off);
/* The same in ONE call, for a caller that wants the chunks in host memory at exactly their compressed sizes (the host mirror's
 * schunk / image constructors: chunks are std::vector-like buffers of cbytes): the batch runs as a pipeline of groups of about
 * 16 MiB of pixels, and as soon as the sizes of a group are known the engine asks `alloc(user, bytes)` for a block of host memory
 * (page-locked for full PCIe speed: cimg_host_malloc) and sends the group's chunks there, packed back to back at 64-byte
 * boundaries, while the next group is being compressed.  chunk_ptr[i] = where chunk i went (NULL for a chunk that does not fit, cbytes
 * 0).  Returns when every chunk has arrived.  (cimg_compress_batch_host_begin + _fetch move the chunks only after the LAST group:
 * 4.2 against 3.0 ms for 4 x 4096^2 float16.) */
typedef void* (*cimg_alloc_fn)(void* user, size_t bytes);
int cimg_compress_batch_host_packed(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_raw, const int64_t* raw_off,
                                    const int32_t* nbytes, const int32_t* destsize, int32_t* cbytes, cimg_alloc_fn alloc, void* user, void** chunk_ptr);
/* Sizes are read from the chunk headers in host memory (the reference passes INT32_MAX as srcsize, wrapper.h:249,
 * so the header is all there is). */
int cimg_decompress_batch_host(cimg_engine* e, int32_t nchunks,
                               const void* h_comp, const int64_t* comp_off,
                               void* h_raw, const int64_t* raw_off, const int32_t* raw_capacity,
                               int32_t* status);
/* The same for callers that know how many bytes each chunk buffer really holds: a header that claims more
 * (truncated or hostile chunk) is refused with BLOSC2_ERROR_READ_BUFFER before anything is read past the buffer. */
int cimg_decompress_batch_host_sized(cimg_engine* e, int32_t nchunks,
                                     const void* h_comp, const int64_t* comp_off, const int32_t* comp_size,
                                     void* h_raw, const int64_t* raw_off, const int32_t* raw_capacity,
                                     int32_t* status);

/* ---- windows: random access into compressed planes -------------------------------------------------
 * A window is a strided 2-D view over the element space of one PLANE: chunks chunk_first .. chunk_first + chunk_count - 1 of the
 * batch, read back to back (what to_uncompressed concatenates).  Row r of the window is the `width` elements starting at plane
 * element origin + r * row_pitch; it goes to out + out_off + r * out_pitch.  Only the blocks that meet some window row are decoded,
 * and nothing outside the window's rows is written (the gaps between output rows are the caller's).  Examples: a rectangle of a
 * W-wide channel (origin = y0 * W + x0, row_pitch = W), an item range of one chunk (height 1), one window per channel of an image.
 * Every window is checked before anything runs; a window outside its plane, width or height < 0, row_pitch < width with height > 1,
 * out_pitch < width * typesize, chunks of one plane with different typesizes, a chunk other than the plane's last whose nbytes is no
 * multiple of the typesize, or a chunk range outside the batch is BLOSC2_ERROR_INVALID_PARAM, and the engine stays usable.  A window
 * of width or height 0 does nothing.  status[i] receives chunk i's code; chunks no window row meets get 0 and are not read.  zstd
 * chunks and chunks with blocks beyond the normal decoder's LDS are decoded whole on the device (engine scratch) and the window is
 * cut from there.  Both calls return the first failing chunk's code (or 0), take the engine's lock, and void a pending
 * cimg_decompress_batch_device_begin (its _fetch then fails); the host call reuses the staging area as well, so it also voids a
 * pending cimg_compress_batch_host_begin / _fetch. */
typedef struct cimg_window {
    int32_t chunk_first, chunk_count;   /* the batch's chunks that form this window's plane, in order */
    int64_t origin;                     /* element index (within that plane) of the window's first element */
    int64_t row_pitch;                  /* elements between the starts of consecutive window rows in the plane */
    int32_t width, height;              /* elements per row, rows */
    int64_t out_off, out_pitch;         /* byte offset of the first element in the output; bytes between output rows */
} cimg_window;

/* Device-resident chunks (offsets and sizes as cimg_decompress_batch_device_sized; comp_size may be NULL) and a device-resident
 * output.  nbytes[i] / blocksize[i] are the values in chunk i's header; every chunk must say `typesize`. */
int cimg_decompress_windows_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                   const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                   int32_t typesize, int32_t nwindows, const cimg_window* w, void* d_out, int32_t* status);
/* Host-resident chunks and output: the headers are read on the host, only the chunks some window row meets go over PCIe (through
 * the engine's staging area), and only the windows' bytes come back, to h_out at the callers' offsets and pitches.  comp_size may
 * be NULL (the headers' cbytes are trusted). */
int cimg_decompress_windows_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                 const int32_t* comp_size, int32_t nwindows, const cimg_window* w, void* h_out, int32_t* status);
/* The last window call on this engine: blocks decoded by the window launch, chunks decoded whole, compressed bytes uploaded (host
 * call only).  Any pointer may be NULL. */
void cimg_engine_window_stats(cimg_engine* e, int64_t* blocks_decoded, int64_t* chunks_whole, int64_t* comp_bytes_uploaded);

/* Strided windows: a window whose rows take every col_pitch-th element -- a subsampled region, a[y0:y1:sy, x0:x1:sx] of a W-wide
 * channel being origin = y0 * W + x0, row_pitch = sy * W, col_pitch = sx.  Element c of row r is plane element
 * origin + r * row_pitch + c * col_pitch and goes to out + out_off + r * out_pitch + c * typesize: output rows are dense.  Only the
 * blocks that hold a byte of a sampled element are decoded (with col_pitch * typesize >= blocksize, most blocks between a row's
 * first and last sample are not), and only chunks that hold such a block are read or, by the host call, uploaded.  The rules of
 * cimg_window hold, with these in place of "row_pitch < width": col_pitch < 1 is BLOSC2_ERROR_INVALID_PARAM; with
 * span = (width - 1) * col_pitch + 1, a window of height > 1 needs row_pitch >= span (rows run forward and do not interleave), and
 * origin + (height - 1) * row_pitch + span must lie inside the plane.  A window with col_pitch 1 gives the bytes, status and stats
 * of the same cimg_window.  Locking, the voiding of pending _begin calls, status and return values are those of the two calls
 * above, and cimg_engine_window_stats reports on these calls too. */
typedef struct cimg_window_strided {
    int32_t chunk_first, chunk_count;
    int64_t origin;
    int64_t row_pitch;
    int64_t col_pitch;                  /* elements between consecutive elements of a window row in the plane; >= 1 */
    int32_t width, height;              /* elements per OUTPUT row, rows */
    int64_t out_off, out_pitch;
} cimg_window_strided;
int cimg_decompress_windows_strided_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                           const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                           int32_t typesize, int32_t nwindows, const cimg_window_strided* w, void* d_out,
                                           int32_t* status);
int cimg_decompress_windows_strided_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                         const int32_t* comp_size, int32_t nwindows, const cimg_window_strided* w, void* h_out,
                                         int32_t* status);
/* Grouped windows: many windows a call, every block staged once.  The strided calls above run one workgroup per (window, block), so a
 * block that several windows meet -- blocks are runs of whole scanlines: regions that share rows share blocks wherever they lie in x
 * -- is decoded once per window.  These two take the same arguments and give the same output bytes, status[] and return value as
 * the strided call with the same windows (col_pitch 1 is the plain window), with the same locking and the same voiding of pending
 * _begin calls; the host call uploads the same chunks.  They run one workgroup per distinct block, which writes every window that
 * meets it, and cimg_engine_window_stats reports blocks_decoded as the number of distinct blocks staged.  A call whose work items
 * do not fit the launch tables' int32 fields is refused with BLOSC2_ERROR_INVALID_PARAM. */
int cimg_decompress_windows_grouped_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                           const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize,
                                           int32_t typesize, int32_t nwindows, const cimg_window_strided* w, void* d_out,
                                           int32_t* status);
int cimg_decompress_windows_grouped_host(cimg_engine* e, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                         const int32_t* comp_size, int32_t nwindows, const cimg_window_strided* w, void* h_out,
                                         int32_t* status);
/* Typed windows: convert, scale and place each element in the launch.  A typed window is a cimg_window_strided plus the memory
 * side: element c of row r goes to d_out + out_off + r * out_pitch + c * elem_pitch as out_type; the bytes between elements are
 * not written, so the windows of C planes can fill pixel-major rows (elem_pitch = C * size of out_type) in one launch.  For a
 * stored value v, each step rounded to nearest even: x = (float)v (exact for 8 / 16-bit integers and float16; int32, uint32 and
 * float64 take one rounding), y = fl32(fl32(x * scale) + offset) -- two roundings, not a fused multiply-add, float32 denormals
 * kept --, and the output is y (CIMG_T_F32) or y rounded once to float16 (CIMG_T_F16: overflow gives inf, subnormals are kept).
 * That is numpy's (v.astype(float32) * float32(scale) + float32(offset)).astype(out), bit for bit.  A window with
 * out_type == src_type, scale 1 and offset 0 copies each element's bytes unchanged (NaN payloads and -0 survive); any other window
 * with an integer or CIMG_T_F64 out_type is refused.
 * Grouping, locking, voiding of pending _begin calls, status[], the return value and cimg_engine_window_stats are those of
 * cimg_decompress_windows_grouped_device: one workgroup per distinct block, each block staged once however many windows meet it;
 * a call whose windows are all identity with elem_pitch == typesize gives that call's bytes, status and stats.  The launch is
 * cimg_decode_window_typed (CIMG_K_DECODE_WINDOW_TYPED).  Nothing runs, and the call returns BLOSC2_ERROR_INVALID_PARAM, unless
 * every window passes the checks of the strided windows -- but for out_pitch, which here must be at least
 * (width - 1) * elem_pitch + the size of out_type when height > 1 -- and: both types are known; the size of src_type is
 * `typesize`; elem_pitch is at least the size of out_type; out_off, out_pitch (height > 1), elem_pitch and d_out are multiples of
 * the size of out_type (every element is one naturally aligned store); and, for every chunk of the window's plane, blocksize -- and
 * nbytes unless it is the plane's last chunk -- is a multiple of typesize (a converted element must not straddle two blocks).
 * There is no _host form: converting uint8 to float32 before PCIe would quadruple the traffic, and the host-resident classes
 * return one array per channel; host callers read windows in the stored type and convert where the pixels land. */
enum { CIMG_T_U8 = 0, CIMG_T_I8 = 1, CIMG_T_U16 = 2, CIMG_T_I16 = 3, CIMG_T_U32 = 4, CIMG_T_I32 = 5, CIMG_T_F16 = 6, CIMG_T_F32 = 7,
       CIMG_T_F64 = 8 };
typedef struct cimg_window_typed {
    int32_t chunk_first, chunk_count;
    int64_t origin, row_pitch, col_pitch;
    int32_t width, height;
    int64_t out_off, out_pitch;      /* bytes */
    int64_t elem_pitch;              /* bytes; >= size of out_type */
    int32_t src_type, out_type;      /* CIMG_T_* */
    float scale, offset;
} cimg_window_typed;
int cimg_decompress_windows_typed_device(cimg_engine* e, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                                         const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, int32_t typesize,
                                         int32_t nwindows, const cimg_window_typed* w, void* d_out, int32_t* status);

/* ---- window writes: edit compressed planes in place of get_chunk + set_chunk ------------------------
 * The windows are cimg_window, with out_off / out_pitch describing the SOURCE: row r of a window is taken from
 * src + out_off + r * out_pitch.  Windows apply in call order (a later window wins where two overlap).  Every touched chunk's new
 * bytes equal what cimg_compress_batch_* with `p` and destsize[i] produces from the chunk's decoded pixels with the windows
 * written in (for lz4 and blosclz: blosc2_compress_ctx's bytes).  Only the blocks a window row meets are decoded and re-encoded;
 * the other blocks' streams are copied from the old chunk.  zstd chunks, blocks beyond the normal kernels' LDS, memcpyed and
 * special chunks (zero, NaN, repeated value, uninitialised) are decoded, patched and compressed whole on the device.  The input chunks are never modified.
 * Nothing runs, and the call returns BLOSC2_ERROR_INVALID_PARAM, unless every window passes the checks of the window reads, every
 * touched chunk's header agrees with `p` (typesize, codec, filters -- trunc-prec and its meta included: written pixels are truncated
 * like the chunk's own --, split decision, effective blocksize for its nbytes) and every
 * destsize[i] >= 32.  A damaged touched chunk gets its decode error in status[i] and new_cbytes[i] = 0; the others are still
 * written; the call returns the first failing code.  clevel is not in the header: passing the one the chunks were made with is
 * the caller's job, as it is for compress.
 * Every window write takes the engine's lock, decodes and encodes, and so voids a pending cimg_decompress_batch_device_begin AND a
 * pending cimg_compress_batch_device_begin (their _fetch then fails); the host calls reuse the staging area as well and void a
 * pending cimg_compress_batch_host_begin / _device_packed_begin. */
/* Device-resident chunks in, device-resident new chunks out.  Chunk i is read at d_comp + comp_off[i] (comp_size may be NULL);
 * if some window row meets it, its new form is written to d_new + new_off[i] (capacity destsize[i]) and new_cbytes[i] > 0;
 * otherwise new_cbytes[i] = 0 and neither area is touched.  d_new must not overlap the input chunks. */
int cimg_update_windows_device(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* d_comp, const int64_t* comp_off,
                               const int32_t* comp_size, const int32_t* nbytes, const int32_t* blocksize, const int32_t* destsize,
                               int32_t nwindows, const cimg_window* w, const void* d_src, void* d_new, const int64_t* new_off,
                               int32_t* new_cbytes, int32_t* status);
/* Host-resident: headers read on the host, only the touched chunks and the window bytes go up; each touched chunk's new form comes
 * back in memory from `alloc` (as cimg_compress_batch_host_packed does), new_chunks[i] = NULL for the rest. */
int cimg_update_windows_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                             const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window* w,
                             const void* h_src, cimg_alloc_fn alloc, void* user, void** new_chunks, int32_t* new_cbytes,
                             int32_t* status);
/* Strided window writes: the two calls above over cimg_window_strided.  Element c of window row r is written to plane element
 * origin + r * row_pitch + c * col_pitch; the source rows are dense (width * typesize bytes at src + out_off + r * out_pitch).  The
 * window checks are those of the strided reads (col_pitch >= 1, row_pitch >= span for height > 1, every sampled element inside the
 * plane), the other checks, the order (a later window wins on every byte two windows share), new bytes, status and return values
 * those of the calls above.  A block is staged and re-encoded only if it holds a byte of a written element: blocks and chunks
 * between samples are copied as they are or not named at all (new_cbytes[i] = 0; the host call does not upload them).  A block counts
 * as covered -- not staged -- only through windows with col_pitch 1.  With col_pitch 1 everywhere a call gives the new chunks,
 * new_cbytes, status, return value and cimg_engine_update_stats of the plain call with the same windows.  The patch launch is
 * cimg_update_patch_strided (CIMG_K_UPDATE_PATCH_STRIDED); a call whose work items do not fit the tables' int32 fields is
 * BLOSC2_ERROR_INVALID_PARAM before anything runs (a theoretical limit: more than 2^31 (window, block) pairs). */
int cimg_update_windows_strided_device(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* d_comp,
                                       const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                       const int32_t* blocksize, const int32_t* destsize, int32_t nwindows,
                                       const cimg_window_strided* w, const void* d_src, void* d_new, const int64_t* new_off,
                                       int32_t* new_cbytes, int32_t* status);
int cimg_update_windows_strided_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                     const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window_strided* w,
                                     const void* h_src, cimg_alloc_fn alloc, void* user, void** new_chunks, int32_t* new_cbytes,
                                     int32_t* status);
/* Typed window writes: unscale, round and re-encode in the patch launch -- the inverse of cimg_decompress_windows_typed_device,
 * over the same cimg_window_typed with every field in the same role: src_type is the PLANE's stored type, out_type the type IN
 * MEMORY, and out_off / out_pitch / elem_pitch describe the memory side, which here is the SOURCE.  Element c of window row r is
 * loaded from d_src + out_off + r * out_pitch + c * elem_pitch as out_type and written to plane element
 * origin + r * row_pitch + c * col_pitch; the bytes between source elements are not read, so the C windows of a pixel-major source
 * (elem_pitch = C * size of out_type) write C planes in one call.  scale and offset keep the READ convention (stored -> memory is
 * y = v * scale + offset) and the write applies the inverse, so a caller passes the same pair both ways.  For a memory value y,
 * each step rounded to nearest even and float32 denormals kept: x = (float)y (exact), t = fl32(fl32(x - offset) / scale) -- two
 * roundings, the division IEEE correctly rounded: not a multiply by a reciprocal, not a fast divide, not an FMA form.  An integer
 * plane stores rint(t), ties to even, saturated to the type's range (+inf max, -inf min), and 0 for NaN: numpy's
 * clip(rint(where(isnan(t), 0, t)), min, max).astype(type).  A CIMG_T_F16 plane stores t rounded once to half (overflow gives inf,
 * subnormals are kept, a NaN stays a NaN), a CIMG_T_F32 plane t.  A window with out_type == src_type, scale 1 and offset 0 copies
 * each element's bytes unchanged (NaN payloads and -0 survive); CIMG_T_F64 planes and integer or CIMG_T_F64 memory types take only
 * that.  The chunk's trunc-prec filter applies after the conversion.
 * The checks, the order (a later window wins on every byte two windows share), new bytes (every touched chunk equals what
 * cimg_compress_batch_* with `p` gives for the decoded pixels with the CONVERTED windows written in), status[], the return value,
 * locking and cimg_engine_update_stats are those of cimg_update_windows_strided_device; a call whose windows are all identity with
 * elem_pitch == typesize gives that call's new chunks, new_cbytes, status, return value and stats.  The patch launch is
 * cimg_update_patch_typed (CIMG_K_UPDATE_PATCH_TYPED).  Added checks, made before status[] or new_cbytes[] are touched
 * (BLOSC2_ERROR_INVALID_PARAM, nothing runs): scale is finite and not 0, offset is finite; both types are known and the size of
 * src_type is p->typesize; elem_pitch is at least the size of out_type; out_pitch >= (width - 1) * elem_pitch + that size when
 * height > 1 (a source row need not be dense); out_off, out_pitch (height > 1), elem_pitch and d_src are multiples of that size
 * (every element is one naturally aligned load); and, for every chunk of the window's plane, blocksize -- and nbytes unless it is
 * the plane's last chunk -- is a multiple of typesize (a converted element never straddles two blocks).
 * There is no _host form, for the reason the typed reads have none: float32 pixels would cross PCIe at four times the size of the
 * uint8 they become, and the host-resident classes take arrays of the stored type; host callers convert where the pixels are. */
int cimg_update_windows_typed_device(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* d_comp,
                                     const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                     const int32_t* blocksize, const int32_t* destsize, int32_t nwindows,
                                     const cimg_window_typed* w, const void* d_src, void* d_new, const int64_t* new_off,
                                     int32_t* new_cbytes, int32_t* status);
/* Masked and constant window writes: np.copyto(view, src_or_scalar, where=mask) on compressed planes.  The windows are
 * cimg_window_strided with flags, a mask and a value.  For element c of window row r: if the window has CIMG_WM_MASK and the byte at
 * mask + mask_off + r * mask_pitch + c is 0, the plane element keeps its value (any nonzero byte writes); otherwise the element
 * becomes `value` (the first `typesize` bytes) under CIMG_WM_CONST, or the source element at src + out_off + r * out_pitch +
 * c * typesize without it.  Windows apply in call order: a later window wins on every byte it actually writes; where its mask is
 * 0 the earlier window's byte stands.  Every touched chunk's new bytes equal what cimg_compress_batch_* with `p` gives for the
 * decoded pixels with the windows written in (trunc-prec included: a constant is truncated like any written pixel).
 * The checks, status[], the return value, locking, the routes (splice; whole for zstd, wide blocks, memcpyed and special chunks) and
 * cimg_engine_update_stats are those of cimg_update_windows_strided_*; a call whose windows all have flags == 0 gives that call's
 * new chunks, new_cbytes, status, return value and stats.  The patch launch is cimg_update_patch_masked
 * (CIMG_K_UPDATE_PATCH_MASKED).  A block counts as covered -- not staged -- only through windows with col_pitch 1 and no mask,
 * constant or not; a masked window never covers.  A block whose mask bytes are all 0 is still a touched block: staged, re-encoded
 * and byte for byte the old block -- no call reads the mask on the host to prune.  The host call uploads the touched chunks, the
 * rows of the windows without CIMG_WM_CONST and the mask rows of the windows with CIMG_WM_MASK, nothing else (bytes_uploaded says
 * so): a constant unmasked call uploads chunks only.
 * Added refusals (BLOSC2_ERROR_INVALID_PARAM before status[] or new_cbytes[] are touched, nothing runs): unknown flag bits;
 * CIMG_WM_CONST with typesize > 8; a masked window with mask_off < 0, mask_pitch < 0, or height > 1 and mask_pitch < width; a NULL
 * mask pointer while some window has CIMG_WM_MASK; a NULL source pointer while some window lacks CIMG_WM_CONST.  The source pointer
 * may be NULL when every window is constant, the mask pointer when none is masked. */
enum { CIMG_WM_CONST = 1, CIMG_WM_MASK = 2 };
typedef struct cimg_window_masked {
    int32_t chunk_first, chunk_count;
    int64_t origin, row_pitch, col_pitch;   /* plane side: as cimg_window_strided */
    int32_t width, height;
    int64_t out_off, out_pitch;             /* SOURCE rows (dense, width * typesize bytes); ignored with CIMG_WM_CONST */
    int64_t mask_off, mask_pitch;           /* MASK: one byte an element, row r at mask + mask_off + r * mask_pitch; ignored without CIMG_WM_MASK */
    int32_t flags;                          /* CIMG_WM_* */
    int32_t pad_;
    uint8_t value[8];                       /* CIMG_WM_CONST: the element's bytes, the first `typesize` used */
} cimg_window_masked;
int cimg_update_windows_masked_device(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* d_comp,
                                      const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
                                      const int32_t* blocksize, const int32_t* destsize, int32_t nwindows,
                                      const cimg_window_masked* w, const void* d_src, const void* d_mask, void* d_new,
                                      const int64_t* new_off, int32_t* new_cbytes, int32_t* status);
int cimg_update_windows_masked_host(cimg_engine* e, const cimg_cparams* p, int32_t nchunks, const void* h_comp, const int64_t* comp_off,
                                    const int32_t* comp_size, const int32_t* destsize, int32_t nwindows, const cimg_window_masked* w,
                                    const void* h_src, const void* h_mask, cimg_alloc_fn alloc, void* user, void** new_chunks,
                                    int32_t* new_cbytes, int32_t* status);
/* The last update call on this engine: blocks staged from their old streams, blocks re-encoded on the splice route, chunks decoded
 * and compressed whole, bytes uploaded (host call only: touched chunks and window bytes).  Any pointer may be NULL. */
void cimg_engine_update_stats(cimg_engine* e, int64_t* blocks_decoded, int64_t* blocks_encoded, int64_t* chunks_whole,
                              int64_t* bytes_uploaded);

/* ---- packed device storage: what an object that keeps an image compressed in device memory is made of ----------------
 * cimg_compress_batch_device gives chunk i room for destsize[i], so a plane that compresses 2 : 1 still occupies its full size.
 * The pair below is shaped like cimg_compress_batch_host_begin / _fetch with pixels AND destination on the device: _begin
 * compresses into the engine's device staging area and reports cbytes[]; the caller allocates exactly what it needs and _fetch
 * moves chunk i (cbytes[i] bytes; nothing for a chunk that did not fit) to d_dst + dst_off[i] with one launch of the pack kernel.
 * The chunk bytes are those cimg_compress_batch_device writes for the same input and parameters.  _fetch refers to the most recent
 * _begin (of this kind or of the host kind: both leave their chunks in the same staging area); any other batch call that reuses the
 * staging area (the host-resident calls) voids it, and _fetch then fails with BLOSC2_ERROR_INVALID_PARAM.  _begin is a compress
 * call: it voids a pending cimg_compress_batch_device_begin like any other.  Both return after the engine's stream has been
 * synchronised. */
int cimg_compress_batch_device_packed_begin(cimg_engine* e, const cimg_cparams* p, int32_t nchunks,
                                            const void* d_raw, const int64_t* raw_off, const int32_t* nbytes, const int32_t* destsize,
                                            int32_t* cbytes);
int cimg_compress_batch_device_packed_fetch(cimg_engine* e, int32_t nchunks, void* d_dst, const int64_t* dst_off);
/* The pack kernel on its own: a batched gather copy.  Piece i is bytes[i] bytes at the device address d_src[i] (d_src[] is a HOST
 * array of device addresses) and goes to d_dst + dst_off[i]; any alignment of either; bytes[i] == 0 pieces are skipped.  One launch
 * whatever the sizes: the work is cut into 16 KiB tiles, so the time follows the total bytes.  No destination range may overlap a
 * source range or another destination range of the call (checked on the host: BLOSC2_ERROR_INVALID_PARAM, nothing runs).  Returns
 * after the engine's stream has been synchronised. */
int cimg_pack_chunks_device(cimg_engine* e, int32_t nchunks, const void* const* d_src, const int32_t* bytes,
                            void* d_dst, const int64_t* dst_off);
/* Planes -> interleaved pixels: the inverse of cimg_deinterleave_device, same argument meaning and constraints (typesize 1, 2, 4
 * or 8; both buffers 16-byte aligned; plane_stride in bytes, a multiple of 16, at least npixels * typesize).  Returns after the
 * engine's stream has been synchronised. */
int cimg_interleave_device(cimg_engine* e, const void* d_planar, int64_t plane_stride, int32_t nchannels,
                           int32_t typesize, int64_t npixels, void* d_interleaved);
/* Records an event on `stream` (a hipStream_t; NULL: the null stream) and makes the engine's stream wait for it: pixels produced
 * on the caller's stream before this call are seen by the next batch.  (Results need no counterpart: the device calls of this
 * section, the window calls and the plain batch calls return after the engine's stream has been synchronised.) */
int cimg_engine_wait_stream(cimg_engine* e, void* stream);
/* 0 only if [p, p + bytes) is device memory of the engine's device and lies inside one allocation (a sub-range of a larger
 * allocation is fine); else BLOSC2_ERROR_INVALID_PARAM and a message.  Nothing is launched.  For layers that take addresses from
 * their callers: a host pointer handed to a kernel is a GPU fault, so they ask here first. */
int cimg_device_range_check(cimg_engine* e, const void* p, size_t bytes);

/* ---- glue between the blosc2 shim and the batched calls ----------------------------------------------
 * The single-chunk blosc2_*_ctx calls run on one process-wide engine (device $CIMG_DEVICE, else the
 * current HIP device); cimg_shared_engine() hands it out so that host code holding blosc2 contexts
 * (the re-shaped schunk / image loops) can batch on the same stream.  NULL + cimg_last_error(NULL) on
 * failure.  cimg_context_cparams() copies the codec parameters a compression context was created with. */
struct blosc2_context_s;
cimg_engine* cimg_shared_engine(void);
int cimg_context_cparams(const struct blosc2_context_s* context, cimg_cparams* out);

/* ---- device memory without HIP headers ------------------------------------------------------------ */
void* cimg_device_malloc(cimg_engine* e, size_t bytes);
void  cimg_device_free(cimg_engine* e, void* p);
int   cimg_memcpy_h2d(cimg_engine* e, void* d_dst, const void* h_src, size_t bytes);
int   cimg_memcpy_d2h(cimg_engine* e, void* h_dst, const void* d_src, size_t bytes);

/* ---- page-locked host memory ---------------------------------------------------------------------------
 * The host-buffer batch calls move pixels and chunks over PCIe; from / to ordinary (pageable) memory the copy
 * is staged by the runtime and a freshly allocated destination is page-faulted in on the way (measured: 64 MiB
 * of pixels into a new numpy array 22 ms, into a recycled page-locked buffer 2 ms).  Host code that owns its
 * buffers (the Python binding's result arrays, the compress staging area) takes them from here.  NULL on failure. */
void* cimg_host_malloc(size_t bytes);
void  cimg_host_free(void* p);

/* ---- kernel timing (HIP events on the engine's stream) ------------------------------------------- */
enum { CIMG_K_ENCODE = 0, CIMG_K_LAYOUT = 1, CIMG_K_EMIT = 2, CIMG_K_DECODE = 3, CIMG_K_DEINTERLEAVE = 4, CIMG_K_DECODE_ZSTD = 5, CIMG_K_ENCODE_ZSTD = 6,
       /* CIMG_K_DECODE_ZSTD is the whole zstd read path of a batch; its launches are also timed one by one: */
       CIMG_K_ZSTD_WALK = 7, CIMG_K_ZSTD_REPLAY = 8, CIMG_K_ZSTD_FUSED = 9, CIMG_K_ZSTD_SEQ = 10, CIMG_K_ZSTD_LIT = 11,
       /* blocks beyond the normal kernels' LDS (up to 256 KiB): */
       CIMG_K_ENCODE_WIDE = 12, CIMG_K_DECODE_WIDE = 13,
       /* zstd blocks beyond the normal kernels' LDS: the wide encoder's zstd instance, the replay out of device-memory slots */
       CIMG_K_ENCODE_WIDE_ZSTD = 14, CIMG_K_ZSTD_REPLAY_WIDE = 15,
       /* the window launch of cimg_decompress_windows_device / _host */
       CIMG_K_DECODE_WINDOW = 16,
       /* window writes: stage-and-patch, splice layout, splice copy */
       CIMG_K_UPDATE_PATCH = 17, CIMG_K_UPDATE_LAYOUT = 18, CIMG_K_UPDATE_EMIT = 19,
       /* packed device storage: the batched gather copy, planes -> interleaved pixels */
       CIMG_K_PACK = 20, CIMG_K_INTERLEAVE = 21,
       /* the window launch of cimg_decompress_windows_strided_device / _host */
       CIMG_K_DECODE_WINDOW_STRIDED = 22,
       /* trunc-prec (filters[4] == 4): the masked copy in front of a compress batch */
       CIMG_K_TRUNC_PREC = 23,
       /* the window launch of cimg_decompress_windows_grouped_device / _host */
       CIMG_K_DECODE_WINDOW_GROUPED = 24,
       /* BloscLZ streams beyond 65 535 bytes (blocks up to 256 KiB): the wide encoder's BloscLZ instance */
       CIMG_K_ENCODE_WIDE_BLOSCLZ = 25,
       /* the patch launch of cimg_update_windows_strided_device / _host */
       CIMG_K_UPDATE_PATCH_STRIDED = 26,
       /* the window launch of cimg_decompress_windows_typed_device */
       CIMG_K_DECODE_WINDOW_TYPED = 27,
       /* the patch launch of cimg_update_windows_typed_device */
       CIMG_K_UPDATE_PATCH_TYPED = 28,
       /* the patch launch of cimg_update_windows_masked_device / _host */
       CIMG_K_UPDATE_PATCH_MASKED = 29, CIMG_K_COUNT = 30 };
/* on = 0: off; on = n > 0: the kernels of every n-th batch call are bracketed by events (1 = every call).  Each
 * event record costs about 5 us of stream time, so a throughput run samples (bench.py: every 4th batch). */
void cimg_engine_enable_timing(cimg_engine* e, int on);
void cimg_engine_reset_timing(cimg_engine* e);
/* total milliseconds and launch count of one kernel since the last reset (syncs the stream) */
int  cimg_engine_kernel_time(cimg_engine* e, int kernel, double* total_ms, int64_t* launches);
/* the duration of every timed launch since the last reset, in milliseconds, oldest first (for medians); returns how many were
 * copied (at most max_samples), < 0 on error */
int  cimg_engine_kernel_samples(cimg_engine* e, int kernel, float* ms, int max_samples);
/* decode batches since the engine was created: how many went through the lean launch (cimg_decode_lean), how many blocks of
 * those batches it left to cimg_decode_blocks (leftover blocks included), their block total, and how many batches needed
 * cimg_decode_zstd.  Any pointer may be NULL. */
void cimg_engine_decode_stats(cimg_engine* e, int64_t* lean_batches, int64_t* blocks_left_to_general, int64_t* blocks_total, int64_t* zstd_batches);
/* the zstd read path since the engine was created: batches that needed it, and blocks whose plan did not fit its slot (the walk
 * refused them and cimg_decode_zstd decoded them behind the other launches).  Any pointer may be NULL. */
void cimg_engine_zstd_stats(cimg_engine* e, int64_t* zstd_batches, int64_t* blocks_refused);
const char* cimg_kernel_name(int kernel);

/* ---- diagnostics: per-workgroup clock stamps of the most recent encode (0) / decode (1) launch ------
 * 16 uint64 per workgroup: four stamps of {shader clock, 100 MHz clock, HW_ID, XCC_ID} (start, stream 0
 * staged, stream 1 staged, end).  Off by
 * default; when on, the NEXT launches stamp (the dbg pointer is null otherwise and the kernels skip it). */
void cimg_engine_debug_stamps(cimg_engine* e, int on);
int  cimg_engine_read_stamps(cimg_engine* e, int which, uint64_t* out, int max_workgroups);

#ifdef __cplusplus
}
#endif
#endif
