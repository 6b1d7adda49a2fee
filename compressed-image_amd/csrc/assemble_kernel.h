// assemble_kernel.h -- turn per-stream records + scratch payloads into finished blosc2 chunks.
//
//   layout_chunks  one wave per chunk.  Wave-wide prefix sum over the chunk's stream records gives
//                  every block its bstart and the chunk its cbytes, and re-applies blosc2's
//                  running-destsize rule (the reference always passes the
//                  NOMINAL chunk size + 32 as destsize, schunk.h:73): a stream that would not fit
//                  turns the whole chunk into a memcpyed chunk; a chunk whose streams are all zero
//                  runs becomes the 32-byte special-zero chunk.  Writes header + bstarts.
//   emit_blocks    one 256-thread workgroup per block: writes the csize words and copies the
//                  payloads from the scratch slot to their final place (or the raw pixels for a
//                  memcpyed chunk).
// The CPU twin of this split is oracle/chunk.c: orc_blosc2_compress_2phase.
#pragma once
#include "codec_types.h"
#include "wave.h"
#include "decode_kernel.h"

namespace cimg {

#ifdef CIMG_EMULATE
// test-side statistics only: streams the encoder left as REC_RAW_SRC, streams placed from the source
inline long g_emu_src_left = 0, g_emu_src_placed = 0;
// ... and of the streams placed from the source: by the wave that encoded them, by another wave (a helper), and those their owner
// skipped because the block's mark said a helper had placed them
inline long g_emu_src_by_owner = 0, g_emu_src_by_helper = 0, g_emu_src_owner_skipped = 0;
#define CIMG_EMU_COUNT(x) (++(x))
#else
#define CIMG_EMU_COUNT(x) ((void)0)
#endif

struct AssembleArgs {
    const ChunkDesc* descs;
    int32_t nchunks;
    CodecParams p;
    const uint8_t* raw;
    const uint8_t* scratch;
    const StreamRec* recs;
    uint8_t* comp;             // chunks are written at comp + desc.comp_off
    ChunkLayout* layout;       // per chunk
    int32_t uniform_nblocks;   // > 0: every chunk has this many blocks
    ChunkLayout* layout_host;  // optional second copy of `layout` in pinned host memory (read by the host after the sync)
    int32_t skip_assembled;    // 1 (the stand-alone kernels behind an assembling encode launch): chunks with ChunkDesc::assemble are done already
};

CIMG_DEV int rec_payload(const StreamRec& r) { return r.kind == REC_RUN ? (r.value > 0 ? 1 : 0) : r.csize; }

struct LayoutChunk {
    const AssembleArgs& a;
    int chunk;
    // inside the encode launch (encode_kernel.h): what this wave writes -- bstarts, header, the layout word -- is read by waves on
    // other XCDs before the launch ends, so it is written THROUGH to memory (agent-scope stores) instead of being written back by
    // an L2 flush afterwards; possible when the chunk starts on a 4-byte boundary (the caller checks)
    bool through = false;
    CIMG_DEV LayoutChunk(const AssembleArgs& a_, int chunk_) : a(a_), chunk(chunk_) {}

    CIMG_DEV void write_header(const ChunkDesc& d, uint8_t* c, int flags, int cbytes, int blosc2_flags)
    {
        LV<uint32_t> byte;
        FOR_LANES(l) {
            uint32_t v = 0;
            if (l == 0) v = 5;                                        // BLOSC2_VERSION_FORMAT_STABLE
            else if (l == 1) v = 1;                                   // codec format version
            else if (l == OFF_FLAGS) v = (uint32_t)flags;
            else if (l == OFF_TYPESIZE) v = (uint32_t)(a.p.typesize > 255 ? 1 : a.p.typesize);
            else if (l >= OFF_NBYTES && l < OFF_NBYTES + 4) v = ((uint32_t)d.nbytes >> (8 * (l - OFF_NBYTES))) & 0xFF;
            else if (l >= OFF_BLOCKSIZE && l < OFF_BLOCKSIZE + 4) v = ((uint32_t)d.blocksize >> (8 * (l - OFF_BLOCKSIZE))) & 0xFF;
            else if (l >= OFF_CBYTES && l < OFF_CBYTES + 4) v = ((uint32_t)cbytes >> (8 * (l - OFF_CBYTES))) & 0xFF;
            else if (l == OFF_FILTERS + 4) v = (uint32_t)a.p.trunc & 0xFF;          // trunc-prec: named, and its meta (the pixels came truncated)
            else if (l == OFF_FILTERS_META + 4) v = ((uint32_t)a.p.trunc >> 8) & 0xFF;
            else if (l == OFF_FILTERS + 5) v = (uint32_t)a.p.filter;
            else if (l == OFF_COMPCODE) v = (uint32_t)a.p.compcode;
            else if (l == OFF_BLOSC2_FLAGS) v = (uint32_t)blosc2_flags;
            byte[l] = v;
        }
        if (through) {
            // eight dwords, lanes 0 .. 7 (the bytes of dword k sit in lanes 4 k .. 4 k + 3)
            LV<int> src;
            LV<uint32_t> b0, b1, b2, b3;
            FOR_LANES(l) { src[l] = (4 * l) & 63; }
            lane_gather(byte, src, b0);
            FOR_LANES(l) { src[l] = (4 * l + 1) & 63; }
            lane_gather(byte, src, b1);
            FOR_LANES(l) { src[l] = (4 * l + 2) & 63; }
            lane_gather(byte, src, b2);
            FOR_LANES(l) { src[l] = (4 * l + 3) & 63; }
            lane_gather(byte, src, b3);
            FOR_LANES_W(l) { if (l < HEADER_LEN / 4) atomic_store_agent(reinterpret_cast<uint32_t*>(c) + l, b0[l] | (b1[l] << 8) | (b2[l] << 16) | (b3[l] << 24)); }
            return;
        }
        FOR_LANES(l) { if (l < HEADER_LEN) c[l] = (uint8_t)byte[l]; }
    }

    CIMG_DEV void run()
    {
        const ChunkDesc d = uniform_desc(a.descs + chunk);
        if (a.skip_assembled && d.assemble) return;                       // the encode launch did this chunk itself
        uint8_t* c = a.comp + d.comp_off;
        ChunkLayout lay;
        lay.cbytes = 0; lay.mode = 3;
        const int memcpy_bytes = d.nbytes + HEADER_LEN;
        bool fits = !d.memcpyed;
        int nt = HEADER_LEN + 4 * d.nblocks;
        if (fits && nt > d.destsize) fits = false;
        if (fits) {
            const int ts = a.p.typesize;
            const int nfull = d.leftover ? d.nblocks - 1 : d.nblocks;
            const int per_full = d.split ? ts : 1;
            const int total = nfull * per_full + (d.leftover ? 1 : 0);
            // records of GROUP tiles (64 streams each) are requested before the first tile is looked at: one wave per
            // chunk has nothing else to hide the load latency with
            constexpr int GROUP = 4;
            for (int g0 = 0; g0 < total && fits; g0 += 64 * GROUP) {
                LV<StreamRec> recs[GROUP];
                CIMG_UNROLL
                for (int k = 0; k < GROUP; k++) {
                    FOR_LANES(l) {
                        const int i = imin(g0 + 64 * k + l, total - 1);
                        int jb, s;
                        if (i < nfull * per_full) { jb = i / per_full; s = i - jb * per_full; } else { jb = nfull; s = 0; }
                        const StreamRec* rp = a.recs + (int64_t)(d.blk0 + jb) * a.p.streams_per_block + s;
                        if (through) {
                            // other waves' records, written through by them: read past this XCD's L2 (no invalidate needed)
                            const uint32_t* w = reinterpret_cast<const uint32_t*>(rp);
                            recs[k][l].kind = (int32_t)atomic_load_agent(w + 0); recs[k][l].value = (int32_t)atomic_load_agent(w + 1);
                            recs[k][l].csize = (int32_t)atomic_load_agent(w + 2); recs[k][l].need = (int32_t)atomic_load_agent(w + 3);
                        } else {
                            recs[k][l] = *rp;
                        }
                    }
                }
                CIMG_UNROLL
                for (int k = 0; k < GROUP; k++) {
                    const int i0 = g0 + 64 * k;
                    if (i0 >= total || !fits) break;
                    LV<int> sz, pre;
                    LV<bool> bad, first;
                    LV<int> blk;
                    FOR_LANES(l) {
                        const int i = i0 + l;
                        sz[l] = 0; bad[l] = false; first[l] = false; blk[l] = 0;
                        if (i < total) {
                            int jb, s;
                            if (i < nfull * per_full) { jb = i / per_full; s = i - jb * per_full; } else { jb = nfull; s = 0; }
                            sz[l] = 4 + rec_payload(recs[k][l]);
                            first[l] = s == 0;
                            blk[l] = jb;
                        }
                    }
                    int tile_total;
                    wave_exscan(sz, pre, tile_total);
                    FOR_LANES(l) {
                        const int i = i0 + l;
                        if (i < total) {
                            const int jb = blk[l];
                            const StreamRec r = recs[k][l];
                            const int bsize = (jb == d.nblocks - 1 && d.leftover) ? d.leftover : d.blocksize;
                            const int neblock = bsize / ((d.split && !(jb == d.nblocks - 1 && d.leftover)) ? ts : 1);
                            const int N = nt + pre[l] + 4;               // offset right after this stream's csize word
                            bool f = false;
                            if (r.kind == REC_RUN) {
                                f = N > d.destsize || (r.value > 0 && N + 1 > d.destsize);
                            } else {
                                int maxout = neblock;
                                if (N + maxout > d.destsize) { maxout = d.destsize - N; if (maxout <= 0) f = true; }
                                if (!f) {
                                    if (r.kind == REC_LZ4) { if (r.need > maxout) f = true; }
                                    else if (N + neblock > d.destsize) f = true;
                                }
                            }
                            bad[l] = f;
                            if (first[l]) { if (through) atomic_store_agent(reinterpret_cast<uint32_t*>(c + HEADER_LEN) + blk[l], (uint32_t)(nt + pre[l])); else st32(c + HEADER_LEN + 4 * blk[l], nt + pre[l]); }
                        }
                    }
                    if (ballot(bad)) fits = false;
                    nt += tile_total;
                }
            }
            if (fits) {
                if (nt == HEADER_LEN + 4 * d.nblocks + 4 * total) {
                    lay.cbytes = HEADER_LEN; lay.mode = 2;
                    write_header(d, c, d.flags, HEADER_LEN, SPECIAL_ZERO << 4);
                } else {
                    lay.cbytes = nt; lay.mode = 0;
                    write_header(d, c, d.flags, nt, 0);
                }
            }
        }
        if (!fits) {
            if (memcpy_bytes <= d.destsize) {
                lay.cbytes = memcpy_bytes; lay.mode = 1;
                write_header(d, c, d.flags | FLAG_MEMCPYED, memcpy_bytes, 0);
            } else {
                lay.cbytes = 0; lay.mode = 3;
                if (d.destsize >= HEADER_LEN) write_header(d, c, d.flags, 0, 0);
            }
        }
        FOR_LANES_W(l) {
            if (l == 0) {
                if (through) {
                    atomic_store_agent(reinterpret_cast<uint32_t*>(&a.layout[chunk].cbytes), (uint32_t)lay.cbytes);
                    atomic_store_agent(reinterpret_cast<uint32_t*>(&a.layout[chunk].mode), (uint32_t)lay.mode);
                } else {
                    a.layout[chunk] = lay;
                }
                if (a.layout_host) a.layout_host[chunk] = lay;
            }
        }
    }
};

// Can a stored stream of a split block be taken from the block's source bytes (REC_RAW_SRC)?  Byte plane of a 2- or 4-byte type
// under the byte shuffle, or a slice of an unfiltered block.
CIMG_HD bool plane_from_source_ok(int typesize, int filter)
{
    return (filter == FILTER_SHUFFLE && (typesize == 2 || typesize == 4)) || (filter == FILTER_NONE && typesize > 1);
}

// Stream s of a split block, as the encoder's phase A selects it (encode_kernel.h: load_plane), written at dst (any alignment) by one
// wave: registers only, no LDS.  `src` is the block's first byte in the launch's input, which nobody writes during the launch.
CIMG_DEV void wave_plane_from_source(const uint8_t* src, int bsize, int ts, int s, int neblock, bool shuf, uint8_t* dst)
{
    if (!shuf) { wave_copy_g2g<16>(src + (int64_t)s * neblock, dst, neblock, 0, 1); return; }
    const int units = bsize >> 4;                    // 16 source bytes = 16 / ts plane bytes
    constexpr int DEPTH = 16;                        // loads in flight per lane (load_plane)
    if (ts == 2) {
        const uint32_t sel = s ? 0x07050301u : 0x06040200u;
        int u0 = 0;
        for (; u0 + 64 * DEPTH <= units; u0 += 64 * DEPTH) {
            LV<u128> x[DEPTH];
            CIMG_UNROLL
            for (int k = 0; k < DEPTH; k++) { FOR_LANES(l) { x[k][l] = ld128u(src + 16 * (u0 + 64 * k + l)); } }
            CIMG_UNROLL
            for (int k = 0; k < DEPTH; k++) {
                FOR_LANES(l) {
                    const uint64_t q = (uint64_t)byte_perm(x[k][l].y, x[k][l].x, sel) | ((uint64_t)byte_perm(x[k][l].w, x[k][l].z, sel) << 32);
                    memcpy(dst + 8 * (u0 + 64 * k + l), &q, 8);
                }
            }
        }
        for (; u0 < units; u0 += 64) {
            FOR_LANES(l) {
                const int u = u0 + l;
                if (u < units) {
                    const u128 x = ld128u(src + 16 * u);
                    const uint64_t q = (uint64_t)byte_perm(x.y, x.x, sel) | ((uint64_t)byte_perm(x.w, x.z, sel) << 32);
                    memcpy(dst + 8 * u, &q, 8);
                }
            }
        }
    } else {                                         // ts == 4 (plane_from_source_ok)
        const uint32_t s1 = (s & 2) ? 0x07030602u : 0x05010400u;      // bytes {0,1}/{2,3} of two elements
        const uint32_t s2 = (s & 1) ? 0x07060302u : 0x05040100u;      // then byte s of four elements
        int u0 = 0;
        for (; u0 + 64 * DEPTH <= units; u0 += 64 * DEPTH) {
            LV<u128> x[DEPTH];
            CIMG_UNROLL
            for (int k = 0; k < DEPTH; k++) { FOR_LANES(l) { x[k][l] = ld128u(src + 16 * (u0 + 64 * k + l)); } }
            CIMG_UNROLL
            for (int k = 0; k < DEPTH; k++) {
                FOR_LANES(l) {
                    const uint32_t t = byte_perm(x[k][l].y, x[k][l].x, s1), q = byte_perm(x[k][l].w, x[k][l].z, s1);
                    st32(dst + 4 * (u0 + 64 * k + l), (int32_t)byte_perm(q, t, s2));
                }
            }
        }
        for (; u0 < units; u0 += 64) {
            FOR_LANES(l) {
                const int u = u0 + l;
                if (u < units) {
                    const u128 x = ld128u(src + 16 * u);
                    const uint32_t t = byte_perm(x.y, x.x, s1), q = byte_perm(x.w, x.z, s1);
                    st32(dst + 4 * u, (int32_t)byte_perm(q, t, s2));
                }
            }
        }
    }
    // elements of the block past the last whole 16-byte unit
    for (int e0 = (units << 4) / ts; e0 < neblock; e0 += 64) {
        FOR_LANES(l) { if (e0 + l < neblock) dst[e0 + l] = src[(int64_t)(e0 + l) * ts + s]; }
    }
}

struct EmitBlock {
    const AssembleArgs& a;
    int b;
    // inside the encode launch, where idle waves help to place stored planes (encode_kernel.h: encode_emit_own): block b's REC_RAW_SRC
    // streams are in place in this launch when placed[b] == gen.  Placing such a stream is idempotent -- the same bytes from the
    // launch's read-only input to the same address, whoever does it -- so the mark is read and written with plain agent-scope loads
    // and stores and never claimed: the worst a stale mark causes is a plane written twice.  ("In place": placed, or taken by a
    // helper that is placing it -- all an owner needs to know is that it need not.)
    // With plane items the stored planes of one block have different owners: an owner also marks its own plane, in a word per
    // stream (placed_streams[b * streams_per_block + s]), and sets the block's mark when it sees every other stored plane of the
    // block marked so.  (Two owners that finish together may both see the other's word unset: the block then stays open, and a
    // helper places it again.)
    uint32_t* placed = nullptr;
    uint32_t* placed_streams = nullptr;
    uint32_t gen = 0;
    bool src_skipped = false, src_placed = false;   // what copy() did with the block's stored planes (diagnostics: tools/diag_assemble.py)
    CIMG_DEV EmitBlock(const AssembleArgs& a_, int b_) : a(a_), b(b_) {}

    // the stand-alone kernel: `wave` of `nwaves` cooperating waves copy the whole block
    CIMG_DEV void run(int wave, int nwaves = 4) { copy(wave, nwaves, 0, MAX_STREAMS); }
    // inside the encode launch: ONE wave copies the streams [s_begin, s_end) it encoded itself.  What OTHER waves wrote -- the
    // closer's layout word and bstarts[j], the records of the block's other streams -- is read with agent-scope loads straight from
    // memory (the writers wrote it through / wrote it back); the payload is this wave's own and comes out of its own L2.  No
    // acquire fence: an L2 invalidate per wave and chunk, a thousand waves at once, cost the launch more than the copies.
    // only_src: the caller is a helper, not the owner -- it places the block's REC_RAW_SRC streams and nothing else.
    CIMG_DEV void run_streams(int s_begin, int s_end, bool only_src = false) { copy(0, 1, s_begin, s_end, true, only_src); }
    // (A REC_RAW_SRC stream has nothing in the scratch slot: its bytes are selected from the launch's input, which nobody writes.)
    CIMG_DEV void copy(int wave, int nwaves, int s_begin, int s_end, bool coherent = false, bool only_src = false)
    {
        const int chunk = find_chunk(a.descs, a.nchunks, b, a.uniform_nblocks);
        const ChunkDesc d = uniform_desc(a.descs + chunk);
        if (a.skip_assembled && d.assemble) return;                   // the encode launch did this chunk itself
        const int j = b - d.blk0;
        uint8_t* c = a.comp + d.comp_off;
        const bool leftover_blk = (j == d.nblocks - 1 && d.leftover);
        const int bsize = leftover_blk ? d.leftover : d.blocksize;
        const int ns = (d.split && !leftover_blk) ? a.p.typesize : 1;
        const StreamRec* rp = a.recs + (int64_t)b * a.p.streams_per_block;
        // What other waves wrote: the layout word, bstarts[j], {kind, value, csize} of the block's streams.  Coherent form: ONE
        // round trip of agent-scope loads, lane 0 the mode, lane 1 bstarts[j], lanes 2 + 3 s .. 4 + 3 s the record of stream s
        // (MAX_STREAMS = 16 streams: 50 lanes), lane 50 the block's mark, lanes 51 + s the mark of stream s < 13.  (bstarts[] is 4-byte aligned whenever the chunk is; a caller-chosen odd chunk
        // address takes a fence instead.)
        const bool aligned = ((uintptr_t)(c + HEADER_LEN) & 3) == 0;
        LV<int32_t> meta;
        if (coherent) {
            if (!aligned) fence_acquire();
            FOR_LANES(l) {
                const int k = l - 2, sidx = k >= 0 ? k / 3 : 0, f = k >= 0 ? k - 3 * sidx : 0;
                const uint32_t* p = l == 0 ? reinterpret_cast<const uint32_t*>(&a.layout[chunk].mode)
                                  : (l == 50 && placed) ? placed + b
                                  : (l > 50 && placed_streams && l - 51 < ns) ? placed_streams + (int64_t)b * a.p.streams_per_block + (l - 51)
                                  : l == 1 ? reinterpret_cast<const uint32_t*>(c + HEADER_LEN + (aligned ? 4 * j : 0))
                                           : reinterpret_cast<const uint32_t*>(rp + (sidx < ns ? sidx : 0)) + f;
                meta[l] = (l == 1 && !aligned) ? ld32s(c + HEADER_LEN + 4 * j) : (int32_t)atomic_load_agent(p);
            }
        } else {
            FOR_LANES(l) {
                const int k = l - 2, sidx = k >= 0 ? k / 3 : 0, f = k >= 0 ? k - 3 * sidx : 0;
                const StreamRec& r = rp[sidx < ns ? sidx : 0];
                meta[l] = l == 0 ? a.layout[chunk].mode : l == 1 ? ld32s(c + HEADER_LEN + 4 * j) : (f == 0 ? r.kind : f == 1 ? r.value : r.csize);
            }
        }
        const int mode = readlane(meta, 0);
        if (only_src && mode != 0) return;                            // (a helper keeps out of memcpyed, special and failed chunks)
        if (mode == 1) {
            // memcpyed chunk: the raw pixels of the block; a caller that owns streams [s_begin, s_end) of ns copies that share of them
            const int lo = s_begin <= 0 ? 0 : (int)((int64_t)bsize * s_begin / ns) & ~15;
            const int hi = s_end >= ns ? bsize : (int)((int64_t)bsize * s_end / ns) & ~15;
            const int64_t at = (int64_t)j * d.blocksize + lo;
            if (hi > lo) { if (nwaves == 1) wave_copy_g2g<16>(a.raw + d.raw_off + at, c + HEADER_LEN + at, hi - lo, 0, 1); else wave_copy_g2g(a.raw + d.raw_off + at, c + HEADER_LEN + at, hi - lo, wave, nwaves); }
            return;
        }
        if (mode != 0) return;
        // the mark (in-launch placing only): set, the block's REC_RAW_SRC streams are in place or being placed by a helper -- their
        // owner skips them, csize word and plane; a helper finds nothing left to do.  Whoever places ALL of them sets it afterwards
        // (a plane item's owner only when the block's other planes are not REC_RAW_SRC: those have owners of their own).
        const bool marked = coherent && placed && (uint32_t)readlane(meta, 50) == gen;
        if (only_src && marked) return;
        // A helper marks the block BEFORE it places it: from here on it places every stored plane of the block without fail, and the
        // sooner the others see the mark, the fewer take the same block.  (An owner that skips on this mark reads nothing of the
        // block; the launch does not end before the helper has placed it.)
        if (only_src && coherent && placed) { FOR_LANES_W(l) { if (l == 0) atomic_store_agent(placed + b, gen); } }
        const int neblock = bsize / ns;
        const uint8_t* slot = a.scratch + (int64_t)b * a.p.slot_bytes;
        int pos = readlane(meta, 1);
        for (int s = 0; s < ns && s < s_end && s < MAX_STREAMS; s++) {
            StreamRec r;
            r.kind = readlane(meta, 2 + 3 * s); r.value = readlane(meta, 3 + 3 * s); r.csize = readlane(meta, 4 + 3 * s); r.need = 0;
            const bool mine = s >= s_begin && (r.kind == REC_RAW_SRC ? !marked : !only_src);
            if (r.kind == REC_RAW_SRC && marked && s >= s_begin) { src_skipped = true; CIMG_EMU_COUNT(g_emu_src_owner_skipped); }
            if (wave == 0 && mine) {
                const int word = r.kind == REC_RUN ? -r.value : r.csize;
                FOR_LANES(l) {
                    if (l < 4) c[pos + l] = (uint8_t)(((uint32_t)word >> (8 * l)) & 0xFF);
                    if (l == 4 && r.kind == REC_RUN && r.value > 0) c[pos + 4] = 0x01;
                }
            }
            pos += 4;
            if (r.kind == REC_RAW_SRC) {
                // (the stand-alone kernel never meets one: the kind exists only in chunks assembled inside the encode launch, by one wave)
                if (mine) {
                    CIMG_EMU_COUNT(g_emu_src_placed);
                    src_placed = true;
                    if (only_src) CIMG_EMU_COUNT(g_emu_src_by_helper); else CIMG_EMU_COUNT(g_emu_src_by_owner);
                    wave_plane_from_source(a.raw + d.raw_off + (int64_t)j * d.blocksize, bsize, a.p.typesize, s, neblock, a.p.filter == FILTER_SHUFFLE, c + pos);
                }
            }
            else if (r.kind != REC_RUN && mine) { if (nwaves == 1) wave_copy_g2g<16>(slot + (int64_t)s * neblock, c + pos, r.csize, 0, 1); else wave_copy_g2g(slot + (int64_t)s * neblock, c + pos, r.csize, wave, nwaves); }
            pos += rec_payload(r);
        }
        if (coherent && placed && !marked && !only_src) {
            // every stored plane of the block in place?  An owner counts its own and those whose owners marked them.  (More streams than the 13 whose marks were read: the block is left to a helper.)
            bool all = true;
            const bool part = s_begin > 0 || s_end < ns;
            for (int s = 0; s < ns && s < MAX_STREAMS; s++) {
                if (readlane(meta, 2 + 3 * s) != REC_RAW_SRC) continue;
                const bool own = s >= s_begin && s < s_end;
                if (own && part && placed_streams) { FOR_LANES_W(l) { if (l == 0) atomic_store_agent(placed_streams + (int64_t)b * a.p.streams_per_block + s, gen); } }
                if (!own && !(placed_streams && s < 13 && (uint32_t)readlane(meta, 51 + s) == gen)) all = false;
            }
            if (all) { FOR_LANES_W(l) { if (l == 0) atomic_store_agent(placed + b, gen); } }
        }
    }
};

}  // namespace cimg
