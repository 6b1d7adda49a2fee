// window_plan.h -- the planner of cimg_decode_window (window_kernel.h) and the order in which a window call runs.  Pure C++,
// shared by the engine (engine.hip) and the emulator tests (tests/emu/window_emu.cpp, tests/emu/mock_window.cpp and the _strided files that include them), like
// wide_plan.h.
//
// A window is a strided 2-D view over the element space of one PLANE: chunks chunk_first .. chunk_first + chunk_count - 1 of the
// batch, read back to back.  Its row r covers elements [origin + r * row_pitch, + width) of the plane and goes to the output at
// out_off + r * out_pitch.  The planner validates every window before anything runs, then lists the blocks that meet some window
// row -- each once per window -- as work items.  Chunks whose blocks the window kernel cannot stage (zstd, blocks beyond LDS)
// are decoded whole through the batch path first and cut from there (copy-mode items).  A strided window (StridedWindowSpec, for
// cimg_decode_window_strided) takes every col_pitch-th element of its rows; its planner lists only the blocks that hold a byte of
// a sampled element, and run_windows and plan_windows_host serve both kinds of window.  A grouped call (run_windows_grouped, for
// cimg_decode_window_grouped) plans and runs the same way and regroups each launch's items by block: group_items.  A typed call
// (run_windows_typed, for cimg_decode_window_typed) is a grouped call whose windows also say how each element is converted and placed.
//
// The host-buffer call (cimg_decompress_windows_host) is planned here too, for the engine and the emulator alike: open_window_call
// (the opening of both read calls), read_named_headers, stage_chunk and pack_rows (shared with update_plan.h) and plan_windows_host,
// which decides everything between "the arguments are good" and "reserve the staging buffers".
#pragma once
#include "wide_plan.h"
#include "window_kernel.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace cimg {

// = cimg_window (include/cimg_hip.h)
struct WindowSpec {
    int32_t chunk_first, chunk_count;
    int64_t origin;
    int64_t row_pitch;
    int32_t width, height;
    int64_t out_off, out_pitch;
};

// = cimg_window_strided (include/cimg_hip.h): element c of row r is plane element origin + r * row_pitch + c * col_pitch
struct StridedWindowSpec {
    int32_t chunk_first, chunk_count;
    int64_t origin;
    int64_t row_pitch;
    int64_t col_pitch;
    int32_t width, height;
    int64_t out_off, out_pitch;
};

template <class Item>
struct WindowPlanT {
    std::vector<ChunkDesc> descs;       // every chunk of the batch (raw_off 0; untouched chunks are never read)
    std::vector<int64_t> plane_start;   // plane byte offset of each chunk in its window's plane (the last window that names it)
    std::vector<uint8_t> touched;       // 1: some window row meets the chunk
    std::vector<uint8_t> whole;         // 1: decoded whole (copy-mode items)
    std::vector<Item> items;            // decode items (b >= 0) and copy items (b < 0, src_off filled in by the caller)
    int32_t lds_bytes = 0;              // LDS of the window launch (largest staging among the chunks it decodes block by block)
    int64_t blocks = 0;                 // decode items
};
using WindowPlan = WindowPlanT<WindowItem>;
using StridedWindowPlan = WindowPlanT<StridedWindowItem>;
template <class Spec> struct PlanOf { using type = WindowPlan; };
template <> struct PlanOf<StridedWindowSpec> { using type = StridedWindowPlan; };

// the start of a plan: nothing listed, one descriptor per chunk of the batch
template <class Item>
inline void plan_descs(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const uint8_t* whole_hint, WindowPlanT<Item>* plan)
{
    plan->descs.assign((size_t)nchunks, ChunkDesc{});
    plan->plane_start.assign((size_t)nchunks, 0);
    plan->touched.assign((size_t)nchunks, 0);
    plan->whole.assign((size_t)nchunks, 0);
    plan->items.clear();
    plan->lds_bytes = 0;
    plan->blocks = 0;
    int32_t blk = 0;
    for (int i = 0; i < nchunks; i++) {
        ChunkDesc& d = plan->descs[(size_t)i];
        d.nbytes = nbytes[i];
        d.blocksize = blocksize[i] > 0 ? blocksize[i] : 1;
        d.nblocks = d.nbytes > 0 ? d.nbytes / d.blocksize : 0;
        d.leftover = d.nbytes > 0 ? d.nbytes % d.blocksize : 0;
        if (d.leftover) d.nblocks++;
        d.blk0 = blk;
        blk += d.nblocks;
        plan->whole[(size_t)i] = (whole_hint && whole_hint[i]) || decode_is_wide(d.blocksize);
    }
}

// the end of a plan: the launch's LDS and the count of decode items
template <class Item>
inline void plan_totals(WindowPlanT<Item>* plan)
{
    for (size_t i = 0; i < plan->descs.size(); i++)
        if (plan->touched[i] && !plan->whole[i]) plan->lds_bytes = imax(plan->lds_bytes, decode_lds_bound(plan->descs[i].blocksize));
    for (const Item& t : plan->items) if (t.b >= 0) plan->blocks++;
}

// the plane a window names: its typesize and its size in elements, or the refusal
inline int plane_of_window(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int chunk_first,
                           int chunk_count, int* ts_out, int64_t* elems)
{
    if (chunk_first < 0 || chunk_count < 1 || chunk_first > nchunks - chunk_count) return ERR_INVALID_PARAM;
    const int ts = typesize[chunk_first];
    if (ts <= 0) return ERR_INVALID_PARAM;
    int64_t total = 0;
    for (int i = chunk_first; i < chunk_first + chunk_count; i++) {
        if (nbytes[i] < 0 || blocksize[i] <= 0 || (nbytes[i] > 0 && blocksize[i] > nbytes[i])) return ERR_INVALID_HEADER;
        if (typesize[i] != ts) return ERR_INVALID_PARAM;
        if (i + 1 < chunk_first + chunk_count && nbytes[i] % ts) return ERR_INVALID_PARAM;
        total += nbytes[i];
    }
    *ts_out = ts;
    *elems = total / ts;
    return 0;
}

// nbytes / blocksize / typesize: per chunk, from the chunk headers.  whole_hint[i] = 1: chunk i must be decoded whole (its codec says
// so; wide blocks are found here).  Chunks outside every window's range are not looked at.
inline int plan_windows(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                        const WindowSpec* w, const uint8_t* whole_hint, WindowPlan* plan)
{
    if (nchunks < 0 || nwindows < 0 || (nwindows > 0 && !w)) return ERR_INVALID_PARAM;
    plan_descs(nchunks, nbytes, blocksize, whole_hint, plan);
    // validation first: nothing is listed unless every window is good
    for (int k = 0; k < nwindows; k++) {
        const WindowSpec& s = w[k];
        if (s.chunk_first < 0 || s.chunk_count < 1 || s.chunk_first > nchunks - s.chunk_count) return ERR_INVALID_PARAM;
        if (s.width < 0 || s.height < 0) return ERR_INVALID_PARAM;
        int ts = 0;
        int64_t elems = 0;
        const int prc = plane_of_window(nchunks, nbytes, blocksize, typesize, s.chunk_first, s.chunk_count, &ts, &elems);
        if (prc < 0) return prc;
        if (s.width == 0 || s.height == 0) continue;
        if (s.height > 1 && s.row_pitch < s.width) return ERR_INVALID_PARAM;
        if (s.out_pitch < (int64_t)s.width * ts || s.out_off < 0) return ERR_INVALID_PARAM;
        if (s.origin < 0 || s.origin > elems || s.width > elems) return ERR_INVALID_PARAM;
        if (s.height > 1 && (s.row_pitch > elems || (int64_t)(s.height - 1) > elems / (s.row_pitch ? s.row_pitch : 1))) return ERR_INVALID_PARAM;
        const int64_t last = s.origin + (int64_t)(s.height - 1) * (s.height > 1 ? s.row_pitch : 0) + s.width;
        if (last > elems) return ERR_INVALID_PARAM;
    }
    // items: rows run forward through the plane, so a block met again by the next row is the window's last item
    for (int k = 0; k < nwindows; k++) {
        const WindowSpec& s = w[k];
        if (s.width == 0 || s.height == 0) continue;
        const int ts = typesize[s.chunk_first];
        const int cf = s.chunk_first, cn = s.chunk_count;
        std::vector<int64_t> start((size_t)cn + 1, 0);
        for (int i = 0; i < cn; i++) start[(size_t)i + 1] = start[(size_t)i] + nbytes[cf + i];
        for (int i = 0; i < cn; i++) plan->plane_start[(size_t)(cf + i)] = start[(size_t)i];
        const size_t first_item = plan->items.size();
        const int64_t rpitch = (int64_t)ts * (s.height > 1 ? s.row_pitch : 0), wbytes = (int64_t)ts * s.width, row0 = (int64_t)ts * s.origin;
        int ci = 0;
        for (int r = 0; r < s.height; r++) {
            const int64_t rs = row0 + (int64_t)r * rpitch, re = rs + wbytes;
            while (ci + 1 < cn && start[(size_t)ci + 1] <= rs) ci++;
            for (int c = ci; c < cn && start[(size_t)c] < re; c++) {
                const int chunk = cf + c;
                const ChunkDesc& d = plan->descs[(size_t)chunk];
                const int64_t cs = start[(size_t)c], ce = start[(size_t)c + 1];
                if (ce <= rs || d.nbytes == 0) continue;
                plan->touched[(size_t)chunk] = 1;
                const int64_t lo = (rs > cs ? rs : cs) - cs, hi = (re < ce ? re : ce) - cs;   // [lo, hi) inside the chunk
                const bool whole = plan->whole[(size_t)chunk] != 0;
                const int jf = whole ? -1 : (int)(lo / d.blocksize), jl = whole ? -1 : (int)((hi - 1) / d.blocksize);
                for (int j = jf; j <= jl; j++) {
                    const int b = whole ? -1 : d.blk0 + j;
                    if (plan->items.size() > first_item) {
                        WindowItem& last = plan->items.back();
                        if (last.chunk == chunk && last.b == b) { last.r1 = r + 1; continue; }
                    }
                    WindowItem t{};
                    t.chunk = chunk; t.b = b; t.r0 = r; t.r1 = r + 1;
                    t.p0 = whole ? cs : cs + (int64_t)j * d.blocksize;
                    t.len = whole ? d.nbytes : 0;
                    t.row0 = row0; t.rpitch = rpitch; t.wbytes = wbytes;
                    t.out_off = s.out_off; t.out_pitch = s.out_pitch;
                    plan->items.push_back(t);
                }
            }
        }
    }
    plan_totals(plan);
    return 0;
}

// The strided form.  Validation adds: col_pitch >= 1; with span = (width - 1) * col_pitch + 1 the elements a row reaches over,
// row_pitch >= span when height > 1 (rows run forward and do not interleave) and origin + (height - 1) * row_pitch + span inside the
// plane -- every product is bounded by the plane before it is formed.  A block is listed only if it holds a byte of a sampled
// element: each row walks sample to sample, and from a listed block straight to the first sample that reaches past its end, so
// the work is min(blocks, samples) per row and the blocks (and chunks) between far-apart samples are never named.
// (the checks but the one on out_pitch, and the listing, are templates: typed windows -- further down -- share them)
// 0: good, 1: nothing to list (width or height 0), < 0: refused
template <class Spec>
inline int check_strided_window(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, const Spec& s, int* ts_out)
{
    if (s.chunk_first < 0 || s.chunk_count < 1 || s.chunk_first > nchunks - s.chunk_count) return ERR_INVALID_PARAM;
    if (s.width < 0 || s.height < 0 || s.col_pitch < 1) return ERR_INVALID_PARAM;
    int ts = 0;
    int64_t elems = 0;
    const int prc = plane_of_window(nchunks, nbytes, blocksize, typesize, s.chunk_first, s.chunk_count, &ts, &elems);
    if (prc < 0) return prc;
    *ts_out = ts;
    if (s.width == 0 || s.height == 0) return 1;
    if (s.out_off < 0) return ERR_INVALID_PARAM;
    if (s.origin < 0 || s.origin >= elems || s.width > elems) return ERR_INVALID_PARAM;
    if (s.width > 1 && s.col_pitch > (elems - 1) / (s.width - 1)) return ERR_INVALID_PARAM;       // span > elems
    const int64_t span = (int64_t)(s.width - 1) * (s.width > 1 ? s.col_pitch : 0) + 1;
    if (span > elems - s.origin) return ERR_INVALID_PARAM;
    if (s.height > 1) {
        if (s.row_pitch < span || s.row_pitch > elems || (int64_t)(s.height - 1) > elems / s.row_pitch) return ERR_INVALID_PARAM;
        if ((int64_t)(s.height - 1) * s.row_pitch > elems - s.origin - span) return ERR_INVALID_PARAM;
    }
    return 0;
}

// the items of validated windows; fill(item, window) completes a fresh item
template <class Spec, class Item, class Fill>
inline void list_strided_items(const int32_t* nbytes, const int32_t* typesize, int nwindows, const Spec* w, WindowPlanT<Item>* plan, Fill fill)
{
    for (int k = 0; k < nwindows; k++) {
        const Spec& s = w[k];
        if (s.width == 0 || s.height == 0) continue;
        const int ts = typesize[s.chunk_first];
        const int cf = s.chunk_first, cn = s.chunk_count;
        std::vector<int64_t> start((size_t)cn + 1, 0);
        for (int i = 0; i < cn; i++) start[(size_t)i + 1] = start[(size_t)i] + nbytes[cf + i];
        for (int i = 0; i < cn; i++) plan->plane_start[(size_t)(cf + i)] = start[(size_t)i];
        const size_t first_item = plan->items.size();
        const int64_t rpitch = (int64_t)ts * (s.height > 1 ? s.row_pitch : 0), row0 = (int64_t)ts * s.origin;
        const int64_t cpitch = (int64_t)ts * (s.width > 1 ? s.col_pitch : 1);
        int ci = 0;
        for (int r = 0; r < s.height; r++) {
            const int64_t rs = row0 + (int64_t)r * rpitch;
            int64_t c = 0;
            while (c < s.width) {
                const int64_t pos = rs + c * cpitch;                                 // the sample's bytes: [pos, pos + ts), inside one chunk
                while (ci + 1 < cn && start[(size_t)ci + 1] <= pos) ci++;
                const int chunk = cf + ci;
                const ChunkDesc& d = plan->descs[(size_t)chunk];
                const int64_t cs = start[(size_t)ci], ce = start[(size_t)ci + 1];
                plan->touched[(size_t)chunk] = 1;
                const bool whole = plan->whole[(size_t)chunk] != 0;
                const int jf = whole ? -1 : (int)((pos - cs) / d.blocksize), jl = whole ? -1 : (int)((pos + ts - 1 - cs) / d.blocksize);
                for (int j = jf; j <= jl; j++) {
                    const int b = whole ? -1 : d.blk0 + j;
                    if (plan->items.size() > first_item) {
                        Item& last = plan->items.back();
                        if (last.chunk == chunk && last.b == b) { last.r1 = r + 1; continue; }
                    }
                    Item t{};
                    t.chunk = chunk; t.b = b; t.r0 = r; t.r1 = r + 1;
                    t.p0 = whole ? cs : cs + (int64_t)j * d.blocksize;
                    t.len = whole ? d.nbytes : 0;
                    t.row0 = row0; t.rpitch = rpitch; t.wbytes = (int64_t)ts * s.width;
                    t.out_off = s.out_off; t.out_pitch = s.out_pitch;
                    t.cpitch = cpitch; t.ts = ts;
                    fill(t, s);
                    plan->items.push_back(t);
                }
                if (c + 1 >= s.width) break;                                         // (the row's last sample: nothing to skip to)
                // the first sample with a byte at or past the end of what was just listed
                int64_t edge = whole ? ce : cs + (int64_t)(jl + 1) * d.blocksize;
                if (edge > ce) edge = ce;
                const int64_t next = (edge - ts - rs) / cpitch + 1;                  // (edge >= pos + ts: the numerator is >= 0)
                c = next > c + 1 ? next : c + 1;
            }
        }
    }
}

inline int plan_windows(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                        const StridedWindowSpec* w, const uint8_t* whole_hint, StridedWindowPlan* plan)
{
    if (nchunks < 0 || nwindows < 0 || (nwindows > 0 && !w)) return ERR_INVALID_PARAM;
    plan_descs(nchunks, nbytes, blocksize, whole_hint, plan);
    for (int k = 0; k < nwindows; k++) {
        int ts = 0;
        const int rc = check_strided_window(nchunks, nbytes, blocksize, typesize, w[k], &ts);
        if (rc < 0) return rc;
        if (rc == 0 && w[k].out_pitch < (int64_t)w[k].width * ts) return ERR_INVALID_PARAM;
    }
    list_strided_items(nbytes, typesize, nwindows, w, plan, [](StridedWindowItem&, const StridedWindowSpec&) {});
    plan_totals(plan);
    return 0;
}

struct WindowStats {
    int64_t blocks_decoded = 0, chunks_whole = 0, comp_bytes_uploaded = 0;
};

// One window call, in the order the engine and the emulators run it.  Env provides
//   int decode_whole(const std::vector<int>& chunks, const std::vector<int64_t>& dst_off, int64_t total, int32_t* st)
//       -- the batch path over the listed chunks into its scratch (st: one status per listed chunk); < 0 only when the
//          device itself failed;
//   int run_items(const WindowPlan& plan, const std::vector<WindowItem>& items, int32_t* status)
//       -- one window launch over `items`, waited for; a chunk's status word is set when one of its blocks fails
//          (for strided windows: the same over StridedWindowPlan and StridedWindowItem).
// A zstd chunk is recognised by its header: the host call knows it up front (whole_hint), the device call when its blocks come
// back pending from the window launch -- those chunks then go the whole-chunk way in a second round.
template <class Env, class Spec>
int run_windows(Env& env, int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                const Spec* w, std::vector<uint8_t> hint, int32_t* status, WindowStats* stats)
{
    typename PlanOf<Spec>::type plan;
    using Item = typename decltype(plan.items)::value_type;
    int rc = plan_windows(nchunks, nbytes, blocksize, typesize, nwindows, w, hint.empty() ? nullptr : hint.data(), &plan);
    if (rc < 0) return rc;
    for (int i = 0; i < nchunks; i++) status[i] = 0;
    *stats = WindowStats{};
    std::vector<uint8_t> done_whole((size_t)nchunks, 0);
    for (int round = 0; round < 2; round++) {
        std::vector<int> list;
        std::vector<int64_t> off;
        std::vector<int64_t> at((size_t)nchunks, -1);
        int64_t total = 0;
        for (int i = 0; i < nchunks; i++)
            if (plan.touched[(size_t)i] && plan.whole[(size_t)i] && !done_whole[(size_t)i]) {
                list.push_back(i); off.push_back(total); at[(size_t)i] = total;
                total += ((int64_t)nbytes[i] + 255) & ~(int64_t)255;
            }
        if (!list.empty()) {
            std::vector<int32_t> st(list.size(), 0);
            if ((rc = env.decode_whole(list, off, total, st.data())) < 0) return rc;
            for (size_t k = 0; k < list.size(); k++) { status[list[k]] = st[k]; done_whole[(size_t)list[k]] = 1; }
            stats->chunks_whole += (int64_t)list.size();
        }
        std::vector<Item> items;
        for (const Item& t : plan.items) {
            if (t.b < 0) {
                if (at[(size_t)t.chunk] < 0 || status[t.chunk] != 0) continue;          // (a chunk that failed whole: nothing to cut)
                Item c = t;
                c.src_off = at[(size_t)t.chunk];
                items.push_back(c);
            } else if (round == 0) {
                items.push_back(t);
            }
        }
        if (!items.empty() && (rc = env.run_items(plan, items, status)) < 0) return rc;
        std::vector<uint8_t> pending((size_t)nchunks, 0);
        bool any = false;
        for (int i = 0; i < nchunks; i++)
            if (status[i] == STATUS_ZSTD_PENDING || status[i] == STATUS_ZSTD_PENDING_SPLIT) { pending[(size_t)i] = 1; status[i] = 0; any = true; }
        if (round == 0)
            for (const Item& t : plan.items) if (t.b >= 0 && !pending[(size_t)t.chunk]) stats->blocks_decoded++;
        if (!any || round == 1) break;
        // second round: the chunks found to be zstd, decoded whole and cut
        if (hint.empty()) hint.assign((size_t)nchunks, 0);
        for (int i = 0; i < nchunks; i++) if (pending[(size_t)i]) hint[(size_t)i] = 1;
        if ((rc = plan_windows(nchunks, nbytes, blocksize, typesize, nwindows, w, hint.data(), &plan)) < 0) return rc;
    }
    for (int i = 0; i < nchunks; i++) if (status[i] != 0) return status[i];
    return 0;
}

// ---- grouped windows: every block staged once, for all the windows that meet it ---------------------------------------------
// (cimg_decode_window_grouped, window_kernel.h).  plan_windows and run_windows stay as they are -- validation, item listing, the
// whole route and the second round for chunks found to be zstd -- and the grouping sits between the plan and the launch: the
// items of a launch are stable-sorted by batch-wide block and cut into units, one per distinct block, whose items keep window
// order (each with its own p0: windows of two planes may share a chunk).  Copy-mode items follow, each a unit of its own.
// The sort is given as a permutation -- order[k]: the item that goes to place k of the launch's table -- so that the 96-byte items
// are moved once, by whoever fills the table; the units name places.  The blocks of a call usually lie close together: a counting
// sort over their range where that range is small against the items, a sort of (block, index) keys otherwise.
template <class Item>
inline void group_items(const std::vector<Item>& items, std::vector<int32_t>* order, std::vector<WindowUnit>* units)
{
    const size_t n = items.size();
    order->resize(n);
    units->clear();
    int64_t lo = INT64_MAX, hi = -1;
    size_t ndec = 0;
    for (const Item& t : items)
        if (t.b >= 0) { lo = t.b < lo ? t.b : lo; hi = t.b > hi ? t.b : hi; ndec++; }
    size_t at = 0;
    if (ndec) {
        const uint64_t range = (uint64_t)(hi - lo) + 1;
        if (range <= 8 * (uint64_t)ndec + 4096) {
            std::vector<int32_t> start((size_t)range + 1, 0);
            for (const Item& t : items) if (t.b >= 0) start[(size_t)(t.b - lo) + 1]++;
            int32_t pos = 0;
            for (size_t j = 0; j < (size_t)range; j++) {
                const int32_t c = start[j + 1];
                start[j] = pos;
                if (c) units->push_back(WindowUnit{pos, c});
                pos += c;
            }
            for (size_t k = 0; k < n; k++) if (items[k].b >= 0) (*order)[(size_t)start[(size_t)(items[k].b - lo)]++] = (int32_t)k;
            at = ndec;
        } else {
            std::vector<uint64_t> keys;
            keys.reserve(ndec);
            for (size_t k = 0; k < n; k++) if (items[k].b >= 0) keys.push_back(((uint64_t)(uint32_t)items[k].b << 32) | (uint64_t)k);
            std::sort(keys.begin(), keys.end());                      // (the index in the low half keeps window order inside a block)
            for (const uint64_t key : keys) {
                (*order)[at] = (int32_t)(key & 0xffffffffu);
                if (!units->empty() && items[(size_t)(*order)[(size_t)units->back().item0]].b == (int32_t)(key >> 32)) units->back().nitems++;
                else units->push_back(WindowUnit{(int32_t)at, 1});
                at++;
            }
        }
    }
    for (size_t k = 0; k < n; k++)
        if (items[k].b < 0) { (*order)[at] = (int32_t)k; units->push_back(WindowUnit{(int32_t)at, 1}); at++; }
}

// An upper bound of the items plan_windows lists, without listing them: a sample has bytes in at most `typesize` blocks.  The
// tables of a grouped launch index items and units with int32 (WindowUnit).
template <class Spec>
inline bool grouped_counts_fit(int nchunks, const int32_t* typesize, int nwindows, const Spec* w)
{
    int64_t bound = 0;
    for (int k = 0; k < nwindows; k++) {
        if (w[k].width <= 0 || w[k].height <= 0) continue;
        const int ts = w[k].chunk_first >= 0 && w[k].chunk_first < nchunks && typesize[w[k].chunk_first] > 0 ? typesize[w[k].chunk_first] : 1;
        const int64_t samples = (int64_t)w[k].width * w[k].height;             // (< 2^62)
        if (samples > INT32_MAX) return false;
        bound += samples * ts;                                                 // (< 2^39 a window; the sum is checked as it grows)
        if (bound > INT32_MAX) return false;
    }
    return true;
}

// run_windows' Env for a grouped call, over an Env that provides decode_whole and
//   int run_units(const StridedWindowPlan& plan, const std::vector<StridedWindowItem>& items, const std::vector<int32_t>& order,
//                 const std::vector<WindowUnit>& units, int32_t* status)
//       -- one grouped launch, waited for, over the table items[order[0]], items[order[1]], ... whose places the units name.
// blocks: the decode units whose chunk was not found to be zstd, that is, the distinct blocks staged block by block.
template <class Env>
struct GroupedEnv {
    Env& env;
    int64_t blocks = 0;

    int decode_whole(const std::vector<int>& list, const std::vector<int64_t>& dst_off, int64_t total, int32_t* st)
    {
        return env.decode_whole(list, dst_off, total, st);
    }
    int run_items(const StridedWindowPlan& plan, const std::vector<StridedWindowItem>& items, int32_t* status)
    {
        if (items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;
        std::vector<int32_t> order;
        std::vector<WindowUnit> units;
        group_items(items, &order, &units);
        const int rc = env.run_units(plan, items, order, units, status);
        if (rc < 0) return rc;
        for (const WindowUnit& u : units) {
            const StridedWindowItem& t = items[(size_t)order[(size_t)u.item0]];
            if (t.b >= 0 && status[t.chunk] != STATUS_ZSTD_PENDING && status[t.chunk] != STATUS_ZSTD_PENDING_SPLIT) blocks++;
        }
        return 0;
    }
};

// run_windows with every launch grouped.  Output, status and return value are those of run_windows over the same windows;
// stats->blocks_decoded counts distinct blocks.  A call whose items might not fit the tables' int32 fields is planned once more up
// front and refused before anything runs.
template <class Env>
int run_windows_grouped(Env& env, int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                        const StridedWindowSpec* w, std::vector<uint8_t> hint, int32_t* status, WindowStats* stats)
{
    if (nwindows > 0 && w && !grouped_counts_fit(nchunks, typesize, nwindows, w)) {
        StridedWindowPlan plan;
        const int rc = plan_windows(nchunks, nbytes, blocksize, typesize, nwindows, w, hint.empty() ? nullptr : hint.data(), &plan);
        if (rc < 0) return rc;
        if (plan.items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;
    }
    GroupedEnv<Env> g{env};
    const int rc = run_windows(g, nchunks, nbytes, blocksize, typesize, nwindows, w, std::move(hint), status, stats);
    stats->blocks_decoded = g.blocks;
    return rc;
}

// ---- typed windows: convert, scale and place each element in the launch -------------------------------------------------------
// (cimg_decode_window_typed, window_kernel.h).  A typed window is a strided window with a description of the memory side: element c
// of row r goes to out_off + r * out_pitch + c * elem_pitch as out_type, after y = fl32(fl32((float)v * scale) + offset); a window
// whose out_type is its src_type with scale 1 and offset 0 copies elements unchanged.  The window checks are those of the strided
// windows but for out_pitch (a row need not be dense); added: known types, src_type of the plane's typesize, only float32 / float16
// out of a conversion, elem_pitch >= the output size, rows that do not run into each other, natural alignment of every output
// element, and blocks made of whole elements all through the window's plane (a converted element cannot come from two blocks).
// = cimg_window_typed (include/cimg_hip.h)
struct TypedWindowSpec {
    int32_t chunk_first, chunk_count;
    int64_t origin;
    int64_t row_pitch;
    int64_t col_pitch;
    int32_t width, height;
    int64_t out_off, out_pitch;
    int64_t elem_pitch;
    int32_t src_type, out_type;
    float scale, offset;
};
using TypedWindowPlan = WindowPlanT<TypedWindowItem>;
template <> struct PlanOf<TypedWindowSpec> { using type = TypedWindowPlan; };

inline bool typed_identity(const TypedWindowSpec& s) { return s.out_type == s.src_type && s.scale == 1.0f && s.offset == 0.0f; }

// the checks of typed windows (shared by the reads, below, and the typed write call: update_plan.h)
inline int check_typed_windows(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                               const TypedWindowSpec* w)
{
    for (int k = 0; k < nwindows; k++) {
        const TypedWindowSpec& s = w[k];
        int ts = 0;
        const int rc = check_strided_window(nchunks, nbytes, blocksize, typesize, s, &ts);
        if (rc < 0) return rc;
        const int osz = type_size(s.out_type);
        if (!osz || type_size(s.src_type) != ts) return ERR_INVALID_PARAM;
        if (!typed_identity(s) && s.out_type != T_F32 && s.out_type != T_F16) return ERR_INVALID_PARAM;
        for (int i = s.chunk_first; i < s.chunk_first + s.chunk_count; i++) if (blocksize[i] % ts) return ERR_INVALID_PARAM;
        if (s.elem_pitch < osz || s.elem_pitch % osz) return ERR_INVALID_PARAM;
        if (rc) continue;
        if (s.out_off % osz) return ERR_INVALID_PARAM;
        if (s.width > 1 && s.elem_pitch > (INT64_MAX - osz) / (s.width - 1)) return ERR_INVALID_PARAM;
        if (s.height > 1 && (s.out_pitch < (int64_t)(s.width - 1) * s.elem_pitch + osz || s.out_pitch % osz)) return ERR_INVALID_PARAM;
    }
    return 0;
}

inline int plan_windows(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                        const TypedWindowSpec* w, const uint8_t* whole_hint, TypedWindowPlan* plan)
{
    if (nchunks < 0 || nwindows < 0 || (nwindows > 0 && !w)) return ERR_INVALID_PARAM;
    plan_descs(nchunks, nbytes, blocksize, whole_hint, plan);
    const int crc = check_typed_windows(nchunks, nbytes, blocksize, typesize, nwindows, w);
    if (crc < 0) return crc;
    list_strided_items(nbytes, typesize, nwindows, w, plan, [](TypedWindowItem& t, const TypedWindowSpec& s) {
        t.epitch = s.elem_pitch; t.src_type = s.src_type; t.out_type = s.out_type; t.scale = s.scale; t.offset = s.offset;
    });
    plan_totals(plan);
    return 0;
}

// The order of a typed launch's decode units: by the output address of the first element each writes.  The windows of the C planes
// of a pixel-major read fill the channel slots of the same cache lines from C workgroups; this puts those workgroups side by side
// in the grid (stable: the channels stay in order).  Copy-mode units stay behind the others.
inline void order_units_by_output(const std::vector<TypedWindowItem>& items, const std::vector<int32_t>& order, std::vector<WindowUnit>* units)
{
    size_t ndec = 0;
    while (ndec < units->size() && items[(size_t)order[(size_t)(*units)[ndec].item0]].b >= 0) ndec++;
    std::vector<std::pair<int64_t, int32_t>> keys(ndec);
    for (size_t k = 0; k < ndec; k++) {
        const TypedWindowItem& t = items[(size_t)order[(size_t)(*units)[k].item0]];
        const int64_t rel = t.row0 + (int64_t)t.r0 * t.rpitch - t.p0;
        const int64_t c_lo = rel >= 0 ? 0 : (-rel + t.cpitch - 1) / t.cpitch;
        keys[k] = {t.out_off + (int64_t)t.r0 * t.out_pitch + c_lo * t.epitch, (int32_t)k};
    }
    std::sort(keys.begin(), keys.end());
    std::vector<WindowUnit> sorted(ndec);
    for (size_t k = 0; k < ndec; k++) sorted[k] = (*units)[(size_t)keys[k].second];
    std::copy(sorted.begin(), sorted.end(), units->begin());
}

// run_windows' Env for a typed call (GroupedEnv's counterpart), over an Env that provides decode_whole and
//   int run_typed_units(const TypedWindowPlan& plan, const std::vector<TypedWindowItem>& items, const std::vector<int32_t>& order,
//                       const std::vector<WindowUnit>& units, int32_t* status)
template <class Env>
struct TypedEnv {
    Env& env;
    int64_t blocks = 0;

    int decode_whole(const std::vector<int>& list, const std::vector<int64_t>& dst_off, int64_t total, int32_t* st)
    {
        return env.decode_whole(list, dst_off, total, st);
    }
    int run_items(const TypedWindowPlan& plan, const std::vector<TypedWindowItem>& items, int32_t* status)
    {
        if (items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;
        std::vector<int32_t> order;
        std::vector<WindowUnit> units;
        group_items(items, &order, &units);
        order_units_by_output(items, order, &units);
        const int rc = env.run_typed_units(plan, items, order, units, status);
        if (rc < 0) return rc;
        for (const WindowUnit& u : units) {
            const TypedWindowItem& t = items[(size_t)order[(size_t)u.item0]];
            if (t.b >= 0 && status[t.chunk] != STATUS_ZSTD_PENDING && status[t.chunk] != STATUS_ZSTD_PENDING_SPLIT) blocks++;
        }
        return 0;
    }
};

// run_windows_grouped for typed windows: same status, return value and stats (distinct blocks)
template <class Env>
int run_windows_typed(Env& env, int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                      const TypedWindowSpec* w, std::vector<uint8_t> hint, int32_t* status, WindowStats* stats)
{
    if (nwindows > 0 && w && !grouped_counts_fit(nchunks, typesize, nwindows, w)) {
        TypedWindowPlan plan;
        const int rc = plan_windows(nchunks, nbytes, blocksize, typesize, nwindows, w, hint.empty() ? nullptr : hint.data(), &plan);
        if (rc < 0) return rc;
        if (plan.items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;
    }
    TypedEnv<Env> g{env};
    const int rc = run_windows(g, nchunks, nbytes, blocksize, typesize, nwindows, w, std::move(hint), status, stats);
    stats->blocks_decoded = g.blocks;
    return rc;
}

// ---- the host-buffer calls: what is decided before anything is staged -----------------------------------------------------------

// The opening of a read call: < 0 refused, CALL_DONE nothing to do (the call returns 0), 0 go on.
enum : int { CALL_DONE = 1 };
inline int open_window_call(int nchunks, int nwindows, int32_t* status)
{
    if (nchunks < 0 || nwindows < 0) return ERR_INVALID_PARAM;
    if (status) for (int i = 0; i < nchunks; i++) status[i] = 0;
    if (nwindows == 0) return CALL_DONE;
    return nchunks == 0 ? ERR_INVALID_PARAM : 0;
}

// What both host calls plan.  Per-chunk arrays cover the whole batch; a chunk no window names keeps the defaults and is never
// dereferenced, a chunk no window row meets is not staged (up 0).
struct HostCallPlan {
    std::vector<uint8_t> named, flags, version, special;        // named: some window's [chunk_first, +chunk_count) holds the chunk; special: the header's special field
    std::vector<int32_t> nbytes, blocksize, cbytes, typesize;   // from the named chunks' headers
    int bad_window = -1;                // ERR_INVALID_PARAM: this window's chunks leave the batch
    int short_chunk = -1;               // ERR_READ_BUFFER: this named chunk's buffer cannot hold a header
    int bad_chunk = -1;                 // a touched chunk's header was refused (its status word says why)
    // the touched chunks in the staging buffer, in 64-byte slots: `up` bytes of chunk i at d_comp_off[i]
    std::vector<int64_t> d_comp_off;
    std::vector<int32_t> up;
    int64_t comp_total = 0, comp_used = 0, comp_bytes_uploaded = 0;     // (_used: the last byte a slot holds; _total rounds it up)
    // the windows with their rows packed one after the other, each window at a multiple of 256
    std::vector<WindowSpec> dw;
    std::vector<int64_t> wbytes;
    int64_t rows_total = 0, rows_used = 0;
};

// The headers of the chunks the windows name (the geometry of their planes); the others are not looked at.
template <class Spec>
inline int read_named_headers(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                              const Spec* w, HostCallPlan* hp)
{
    const size_t n = (size_t)nchunks;
    hp->named.assign(n, 0); hp->flags.assign(n, 0); hp->version.assign(n, 0); hp->special.assign(n, 0);
    hp->nbytes.assign(n, 0); hp->blocksize.assign(n, 1); hp->cbytes.assign(n, 0); hp->typesize.assign(n, 0);
    hp->d_comp_off.assign(n, 0); hp->up.assign(n, 0);
    for (int k = 0; k < nwindows; k++) {
        if (w[k].chunk_first < 0 || w[k].chunk_count < 1 || w[k].chunk_first > nchunks - w[k].chunk_count) { hp->bad_window = k; return ERR_INVALID_PARAM; }
        for (int i = w[k].chunk_first; i < w[k].chunk_first + w[k].chunk_count; i++) hp->named[(size_t)i] = 1;
    }
    for (int i = 0; i < nchunks; i++) {
        if (!hp->named[(size_t)i]) continue;
        if (comp_size && comp_size[i] < HEADER_LEN) { hp->short_chunk = i; return ERR_READ_BUFFER; }
        const uint8_t* c = comp + comp_off[i];
        memcpy(&hp->nbytes[(size_t)i], c + OFF_NBYTES, 4); memcpy(&hp->blocksize[(size_t)i], c + OFF_BLOCKSIZE, 4); memcpy(&hp->cbytes[(size_t)i], c + OFF_CBYTES, 4);
        hp->typesize[(size_t)i] = c[OFF_TYPESIZE];
        hp->flags[(size_t)i] = c[OFF_FLAGS];
        hp->version[(size_t)i] = c[0];
        hp->special[(size_t)i] = (c[OFF_BLOSC2_FLAGS] >> 4) & 7;
    }
    return 0;
}

// the next slot of the staging buffer: `bytes` of chunk i
inline void stage_chunk(HostCallPlan* hp, int i, int32_t bytes)
{
    hp->d_comp_off[(size_t)i] = hp->comp_total;
    hp->up[(size_t)i] = bytes;
    hp->comp_used = hp->comp_total + bytes;
    hp->comp_total += ((int64_t)bytes + 63) & ~63ll;
    hp->comp_bytes_uploaded += bytes;
}

// the windows as the device sees them: rows packed (out_pitch = width * typesize); the caller's out_off / out_pitch stay in w
template <class Spec>
inline void pack_rows(int nwindows, const Spec* w, const int32_t* typesize, HostCallPlan* hp, std::vector<Spec>* dw)
{
    dw->assign(w, w + nwindows);
    hp->wbytes.assign((size_t)nwindows, 0);
    for (int k = 0; k < nwindows; k++) {
        if (w[k].width <= 0 || w[k].height <= 0) continue;
        const int64_t row = (int64_t)w[k].width * typesize[w[k].chunk_first];
        (*dw)[(size_t)k].out_off = hp->rows_total;
        (*dw)[(size_t)k].out_pitch = row;
        hp->wbytes[(size_t)k] = row * w[k].height;
        hp->rows_used = hp->rows_total + hp->wbytes[(size_t)k];
        hp->rows_total += (hp->wbytes[(size_t)k] + 255) & ~255ll;
    }
}

inline void pack_rows(int nwindows, const WindowSpec* w, const int32_t* typesize, HostCallPlan* hp) { pack_rows(nwindows, w, typesize, hp, &hp->dw); }

struct WindowHostPlan : HostCallPlan {
    std::vector<uint8_t> hint;          // 1: a zstd chunk, decoded whole
};

// cimg_decompress_windows_host: the chunks some window row meets get their full header checks (a refusal is that chunk's status
// word and the call's code), then only they are staged.  ERR_INVALID_PARAM with bad_window < 0: plan_windows refused a window.
// (dw: the packed windows -- hp->dw, or the strided call's list)
template <class Spec>
inline int plan_windows_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                             const Spec* w, int32_t* status, WindowHostPlan* hp, std::vector<Spec>* dw)
{
    int rc = read_named_headers(nchunks, comp, comp_off, comp_size, nwindows, w, hp);
    if (rc < 0) return rc;
    hp->hint.assign((size_t)nchunks, 0);
    // (the special field is decided before the memcpyed flag and the codec format, here as in the kernels: special_plan.h)
    for (int i = 0; i < nchunks; i++) hp->hint[(size_t)i] = (hp->flags[(size_t)i] >> 5) == 4 && !(hp->flags[(size_t)i] & FLAG_MEMCPYED) && hp->special[(size_t)i] == 0;
    typename PlanOf<Spec>::type plan;
    if ((rc = plan_windows(nchunks, hp->nbytes.data(), hp->blocksize.data(), hp->typesize.data(), nwindows, w, hp->hint.data(), &plan)) < 0) return rc;
    for (int i = 0; i < nchunks; i++) {
        if (!plan.touched[(size_t)i]) continue;
        const int32_t cb = hp->cbytes[(size_t)i];
        int code = 0;
        if (hp->version[(size_t)i] > 5) code = ERR_VERSION_SUPPORT;
        else if (cb < HEADER_LEN) code = ERR_INVALID_HEADER;
        else if (comp_size && cb > comp_size[i]) code = ERR_READ_BUFFER;
        if (code) { status[i] = code; hp->bad_chunk = i; return code; }
        stage_chunk(hp, i, cb);
    }
    pack_rows(nwindows, w, hp->typesize.data(), hp, dw);
    return 0;
}
inline int plan_windows_host(int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size, int nwindows,
                             const WindowSpec* w, int32_t* status, WindowHostPlan* hp)
{
    return plan_windows_host(nchunks, comp, comp_off, comp_size, nwindows, w, status, hp, &hp->dw);
}

}  // namespace cimg
