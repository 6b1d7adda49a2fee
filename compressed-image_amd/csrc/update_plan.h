// update_plan.h -- window writes: validation, routing and the order in which an update call runs.  Pure C++, shared by the engine
// (engine.hip) and the emulator tests (tests/emu/window_write_emu.cpp, tests/emu/mock_window_write.cpp), like window_plan.h.
//
// Windows are cimg_window / WindowSpec -- or, for the strided calls, cimg_window_strided / StridedWindowSpec, for the typed call
// cimg_window_typed / TypedWindowSpec, for the masked and constant calls cimg_window_masked / MaskedWindowSpec: run_update and
// plan_update_host are templates over the window type, as run_windows and plan_windows_host are -- with out_off / out_pitch locating the SOURCE rows.  Every touched chunk's new bytes are what a
// from-scratch compress of its decoded pixels with the windows written in gives.  Two routes:
//   splice  regular lz4 / lz4hc / blosclz chunks whose blocks the window kernel can stage and the batch encoder can take: the touched
//           blocks are staged and patched (cimg_update_patch), re-encoded as one-block pseudo-chunks (the batch encode launch, no
//           assembly behind it), and spliced with the old streams of the untouched blocks (cimg_update_layout + cimg_update_emit).
//   whole   everything else (zstd, wide blocks, memcpyed or special-zero chunks, a chunk whose new form clipped at an old coded stream
//           or fell back to memcpyed): decoded whole through the batch path, patched in place, compressed through the batch path.
//
// The host-buffer call (cimg_update_windows_host) is planned here for the engine and the emulator alike: open_update_call (the opening
// of both write calls) and plan_update_host, over window_plan.h's read_named_headers, stage_chunk and pack_rows.
#pragma once
#include "plan.h"
#include "window_plan.h"
#include "update_kernel.h"
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>

namespace cimg {

struct UpdateStats {
    int64_t blocks_decoded = 0, blocks_encoded = 0, chunks_whole = 0, bytes_uploaded = 0;
};

enum : int { ROUTE_NONE = 0, ROUTE_SPLICE = 1, ROUTE_WHOLE = 2, ROUTE_FAILED = 3 };

// true: the rows of items[first .. first + count) cover all `len` bytes of their unit (each item's p0 is the unit's first byte in
// that item's plane)
inline bool items_cover(const std::vector<WindowItem>& items, size_t first, size_t count, int64_t len)
{
    int64_t written = 0;
    for (size_t k = first; k < first + count; k++) written += (int64_t)(items[k].r1 - items[k].r0) * items[k].wbytes;
    if (written < len) return false;
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (size_t k = first; k < first + count; k++) {
        const WindowItem& t = items[k];
        for (int r = t.r0; r < t.r1; r++) {
            const int64_t rs = t.row0 + (int64_t)r * t.rpitch - t.p0;
            const int64_t s = std::max<int64_t>(rs, 0), e = std::min(rs + t.wbytes, len);
            if (s < e) iv.push_back({s, e});
        }
    }
    std::sort(iv.begin(), iv.end());
    int64_t reach = 0;
    for (const auto& x : iv) {
        if (x.first > reach) return false;
        reach = std::max(reach, x.second);
    }
    return reach >= len;
}

// Env provides (each step waited for before it returns; < 0 only when the device itself failed):
//   int headers(list, out)                                 -- the first 32 bytes of every listed chunk, back to back (ONE round trip)
//   int decode_whole(list, dst_off, total, st)             -- the batch path into the env's whole buffer (st per listed chunk)
//   int patch(descs, lds_bytes, units, stage_items, items, to_whole, patch_bytes, status)
//                                                          -- cimg_update_patch into the patch buffer (to_whole 0, patch_bytes long)
//                                                             or into the whole buffer (1); a chunk's status word is set on failure
//   int encode(const EncodePlan&)                          -- the batch encode launch over the patch buffer, records + slots left
//   int splice(cp, chunks, blocks, layout)                 -- cimg_update_layout + cimg_update_emit, layout back on the host
//   int compress(p, list, raw_off, nbytes, destsize, new_off, cbytes)
//                                                          -- the batch compress of chunks lying in the whole buffer (with trunc-prec
//                                                             in p: the pass over those chunks, then the compress)
//   int patch_strided(descs, lds_bytes, units, stage_items, items, to_whole, patch_bytes, status)
//                                                          -- the same for a call over StridedWindowSpec: cimg_update_patch_strided over
//                                                             StridedPatchUnit and StridedWindowItem (only such calls need it)
//   int patch_typed(descs, lds_bytes, units, stage_items, items, to_whole, patch_bytes, status)
//                                                          -- the same for a call over TypedWindowSpec: cimg_update_patch_typed over
//                                                             StridedPatchUnit and TypedWindowItem (only such calls need it)
//   int patch_masked(descs, lds_bytes, units, stage_items, items, to_whole, patch_bytes, status)
//                                                          -- the same for a call over MaskedWindowSpec: cimg_update_patch_masked over
//                                                             StridedPatchUnit and MaskedWindowItem, the env's mask beside its source
//                                                             (only such calls need it)
//   int trunc(typesize, mask64, off, len)    [optional]    -- trunc-prec in place over pieces of the patch buffer, in front of encode().
//                                                             An env without it cannot truncate: parameters that name the filter are
//                                                             ERR_INVALID_PARAM there, as they were before the filter was built.
template <class Env, class = void> struct env_has_trunc : std::false_type {};
template <class Env>
struct env_has_trunc<Env, std::void_t<decltype(std::declval<Env&>().trunc(0, uint64_t(0), std::declval<const std::vector<int64_t>&>(),
                                                                          std::declval<const std::vector<int32_t>&>()))>> : std::true_type {};

// ---- strided windows (StridedWindowSpec: cimg_update_windows_strided_*) -----------------------------------------------------------
// Coverage: a unit needs no staging only if its DENSE items (cpitch == typesize: col_pitch 1, or one element a row) cover it --
// items_cover over those; strided items never prove coverage.
template <class Item, class = std::enable_if_t<std::is_base_of_v<StridedWindowItem, Item>>>
inline bool items_cover(const std::vector<Item>& items, size_t first, size_t count, int64_t len)
{
    int64_t written = 0;                                             // (most units are not covered: no table for them)
    for (size_t k = first; k < first + count; k++) if (items[k].cpitch == items[k].ts) written += (int64_t)(items[k].r1 - items[k].r0) * items[k].wbytes;
    if (written < len) return false;
    std::vector<WindowItem> dense;
    for (size_t k = first; k < first + count; k++) if (items[k].cpitch == items[k].ts) dense.push_back(items[k]);
    return items_cover(dense, 0, dense.size(), len);
}

// Schedule: true when no two items of the unit write a common byte, so that the kernel may hand them to its four waves with no
// barrier between them.  Conservative: every row of every item gives one byte interval inside the unit, from the first to the last
// sampled byte it holds there (the bytes between samples count as written); the intervals are sorted and ANY intersection makes
// the unit ordered.  (Rows of one item never intersect: row_pitch >= span.)  Above UPDATE_DISJOINT_MAX_ROWS intervals a unit the
// proof gives up and says "ordered": 4096 keeps the sort of a unit in the tens of microseconds, and a unit with more rows than
// that has work enough for 256 threads an item.
enum : int { UPDATE_DISJOINT_MAX_ROWS = 4096 };
inline bool items_disjoint(const std::vector<WindowItem>&, size_t, size_t, int64_t, std::vector<std::pair<int64_t, int64_t>>*) { return false; }
// (ivp: the caller's table, so that the units of a call share one allocation)
template <class Item, class = std::enable_if_t<std::is_base_of_v<StridedWindowItem, Item>>>
inline bool items_disjoint(const std::vector<Item>& items, size_t first, size_t count, int64_t len,
                           std::vector<std::pair<int64_t, int64_t>>* ivp)
{
    if (count < 2) return false;                                 // (one item: the schedule does not matter)
    int64_t rows = 0;
    for (size_t k = first; k < first + count; k++) rows += items[k].r1 - items[k].r0;
    if (rows > UPDATE_DISJOINT_MAX_ROWS) return false;
    std::vector<std::pair<int64_t, int64_t>>& iv = *ivp;
    iv.clear();
    for (size_t k = first; k < first + count; k++) {
        const Item& t = items[k];
        const int64_t width = t.wbytes / t.ts;
        for (int r = t.r0; r < t.r1; r++) {
            const int64_t rel = t.row0 + (int64_t)r * t.rpitch - t.p0;
            const int64_t lo = -rel - (t.ts - 1), hi = len - 1 - rel;
            if (hi < 0) continue;
            if (width == 1) {                                    // (a pixel: no division)
                if (lo <= 0) iv.push_back({std::max<int64_t>(rel, 0), std::min(rel + t.ts, len)});
                continue;
            }
            const int64_t c_lo = lo <= 0 ? 0 : (lo + t.cpitch - 1) / t.cpitch;
            const int64_t c_hi = std::min(hi / t.cpitch, width - 1);
            if (c_lo > c_hi) continue;
            iv.push_back({std::max<int64_t>(rel + c_lo * t.cpitch, 0), std::min(rel + c_hi * t.cpitch + t.ts, len)});
        }
    }
    std::sort(iv.begin(), iv.end());
    for (size_t k = 1; k < iv.size(); k++) if (iv[k].first < iv[k - 1].second) return false;
    return true;
}

// the patch launch of a call: cimg_update_patch for plain windows, cimg_update_patch_strided (units with their schedule) for strided
template <class Env>
int patch_units(Env& env, const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<PatchUnit>& units, const std::vector<uint8_t>&,
                const std::vector<WindowItem>& stage, const std::vector<WindowItem>& items, int to_whole, int64_t patch_bytes, int32_t* status)
{
    return env.patch(descs, lds_bytes, units, stage, items, to_whole, patch_bytes, status);
}
template <class Env>
int patch_units(Env& env, const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<PatchUnit>& units, const std::vector<uint8_t>& disjoint,
                const std::vector<WindowItem>& stage, const std::vector<StridedWindowItem>& items, int to_whole, int64_t patch_bytes,
                int32_t* status)
{
    std::vector<StridedPatchUnit> su(units.size());
    for (size_t k = 0; k < units.size(); k++) su[k] = StridedPatchUnit{units[k], disjoint[k], 0};
    return env.patch_strided(descs, lds_bytes, su, stage, items, to_whole, patch_bytes, status);
}
template <class Env>
int patch_units(Env& env, const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<PatchUnit>& units, const std::vector<uint8_t>& disjoint,
                const std::vector<WindowItem>& stage, const std::vector<TypedWindowItem>& items, int to_whole, int64_t patch_bytes,
                int32_t* status)
{
    std::vector<StridedPatchUnit> su(units.size());
    for (size_t k = 0; k < units.size(); k++) su[k] = StridedPatchUnit{units[k], disjoint[k], 0};
    return env.patch_typed(descs, lds_bytes, su, stage, items, to_whole, patch_bytes, status);
}

// ---- typed windows (TypedWindowSpec: cimg_update_windows_typed_device) -------------------------------------------------------------
// A typed WRITE reads its windows the other way round: out_off / out_pitch / elem_pitch / out_type describe the SOURCE in memory,
// src_type the plane.  run_update serves it as it serves the strided call (same items through list_strided_items, same units, same
// coverage and disjointness proofs -- both look at the plane side only); this is what is checked on top, BEFORE the call touches
// status or new_cbytes: every check of the typed reads (check_typed_windows), a finite non-zero scale and a finite offset, a float64
// plane only as the identity, and d_src aligned like every other part of a source address.
inline int check_typed_update(int nchunks, const int32_t* nbytes, const int32_t* blocksize, int typesize, int nwindows, const TypedWindowSpec* w,
                              const void* d_src)
{
    if (nchunks < 0 || nwindows < 0 || typesize <= 0) return ERR_INVALID_PARAM;
    const auto finite = [](float f) { return (f32_bits(f) & 0x7F800000u) != 0x7F800000u; };
    for (int k = 0; k < nwindows; k++) {
        const TypedWindowSpec& s = w[k];
        if (!finite(s.scale) || !finite(s.offset) || s.scale == 0.0f) return ERR_INVALID_PARAM;
        const int msz = type_size(s.out_type);
        if (!msz || !type_size(s.src_type)) return ERR_INVALID_PARAM;
        if (!typed_identity(s) && s.src_type == T_F64) return ERR_INVALID_PARAM;
        if ((uintptr_t)d_src % (uintptr_t)msz) return ERR_INVALID_PARAM;
    }
    const std::vector<int32_t> tsv((size_t)nchunks, typesize > 255 ? 1 : typesize);
    return check_typed_windows(nchunks, nbytes, blocksize, tsv.data(), nwindows, w);
}

// ---- masked and constant windows (MaskedWindowSpec: cimg_update_windows_masked_*) ---------------------------------------------------
// A strided window with flags: WM_CONST (every written element is `value`; out_off / out_pitch are ignored and no source is read)
// and WM_MASK (element c of row r is written only where mask[mask_off + r * mask_pitch + c] != 0).  run_update serves the call as
// it serves the strided one, the items through list_strided_items.  Coverage: only dense UNMASKED items prove that a unit needs no
// staging, constant or not; a masked item never does, whatever its mask holds -- the mask is never read on the host, so a unit
// whose mask bytes are all 0 is still staged, re-encoded and comes out byte for byte the old block.  Disjointness: items_disjoint
// looks at the plane side only and stays sound, since a mask only removes writes.
// = cimg_window_masked (include/cimg_hip.h)
struct MaskedWindowSpec {
    int32_t chunk_first, chunk_count;
    int64_t origin;
    int64_t row_pitch;
    int64_t col_pitch;
    int32_t width, height;
    int64_t out_off, out_pitch;
    int64_t mask_off, mask_pitch;
    int32_t flags;
    int32_t pad_;
    uint8_t value[8];
};
using MaskedWindowPlan = WindowPlanT<MaskedWindowItem>;
template <> struct PlanOf<MaskedWindowSpec> { using type = MaskedWindowPlan; };

// what a masked call checks on top of the strided call's checks, BEFORE it touches status or new_cbytes
inline int check_masked_update(int typesize, int nwindows, const MaskedWindowSpec* w, const void* src, const void* mask)
{
    for (int k = 0; k < nwindows; k++) {
        const MaskedWindowSpec& s = w[k];
        if (s.flags & ~(WM_CONST | WM_MASK)) return ERR_INVALID_PARAM;
        if ((s.flags & WM_CONST) && typesize > 8) return ERR_INVALID_PARAM;
        if (!(s.flags & WM_CONST) && !src) return ERR_INVALID_PARAM;
        if (s.flags & WM_MASK) {
            if (!mask || s.mask_off < 0 || s.mask_pitch < 0) return ERR_INVALID_PARAM;
            if (s.height > 1 && s.mask_pitch < s.width) return ERR_INVALID_PARAM;
            // (the last mask byte's offset fits an int64)
            if (s.height > 1 && s.width >= 0 && s.mask_pitch > (INT64_MAX - s.mask_off - s.width) / (s.height - 1)) return ERR_INVALID_PARAM;
        }
    }
    return 0;
}

inline int plan_windows(int nchunks, const int32_t* nbytes, const int32_t* blocksize, const int32_t* typesize, int nwindows,
                        const MaskedWindowSpec* w, const uint8_t* whole_hint, MaskedWindowPlan* plan)
{
    if (nchunks < 0 || nwindows < 0 || (nwindows > 0 && !w)) return ERR_INVALID_PARAM;
    plan_descs(nchunks, nbytes, blocksize, whole_hint, plan);
    for (int k = 0; k < nwindows; k++) {
        int ts = 0;
        MaskedWindowSpec s = w[k];
        if (s.flags & WM_CONST) s.out_off = 0;                       // (a constant window's source fields are ignored, not checked)
        const int rc = check_strided_window(nchunks, nbytes, blocksize, typesize, s, &ts);
        if (rc < 0) return rc;
        if (rc == 0 && !(s.flags & WM_CONST) && s.out_pitch < (int64_t)s.width * ts) return ERR_INVALID_PARAM;
    }
    list_strided_items(nbytes, typesize, nwindows, w, plan, [](MaskedWindowItem& t, const MaskedWindowSpec& s) {
        t.flags = s.flags; t.mask_off = s.mask_off; t.mask_pitch = s.mask_pitch;
        t.value = 0;
        for (int i = 0; i < 8; i++) t.value |= (uint64_t)s.value[i] << (8 * i);
    });
    plan_totals(plan);
    return 0;
}

inline bool items_cover(const std::vector<MaskedWindowItem>& items, size_t first, size_t count, int64_t len)
{
    const auto proves = [](const MaskedWindowItem& t) { return t.cpitch == t.ts && !(t.flags & WM_MASK); };
    int64_t written = 0;
    for (size_t k = first; k < first + count; k++) if (proves(items[k])) written += (int64_t)(items[k].r1 - items[k].r0) * items[k].wbytes;
    if (written < len) return false;
    std::vector<WindowItem> dense;
    for (size_t k = first; k < first + count; k++) if (proves(items[k])) dense.push_back(items[k]);
    return items_cover(dense, 0, dense.size(), len);
}

template <class Env>
int patch_units(Env& env, const std::vector<ChunkDesc>& descs, int lds_bytes, const std::vector<PatchUnit>& units, const std::vector<uint8_t>& disjoint,
                const std::vector<WindowItem>& stage, const std::vector<MaskedWindowItem>& items, int to_whole, int64_t patch_bytes,
                int32_t* status)
{
    std::vector<StridedPatchUnit> su(units.size());
    for (size_t k = 0; k < units.size(); k++) su[k] = StridedPatchUnit{units[k], disjoint[k], 0};
    return env.patch_masked(descs, lds_bytes, su, stage, items, to_whole, patch_bytes, status);
}

template <class Env, class Spec>
int run_update(Env& env, const HostCParams& p, int nchunks, const int64_t* comp_off, const int32_t* comp_size, const int32_t* nbytes,
               const int32_t* blocksize, const int32_t* destsize, int nwindows, const Spec* w, const int64_t* new_off,
               int32_t* new_cbytes, int32_t* status, UpdateStats* stats)
{
    using Plan = typename PlanOf<Spec>::type;
    using Item = typename decltype(Plan::items)::value_type;
    *stats = UpdateStats{};
    if (nchunks < 0 || nwindows < 0) return ERR_INVALID_PARAM;
    for (int i = 0; i < nchunks; i++) { status[i] = 0; new_cbytes[i] = 0; }
    if (nwindows == 0) return 0;
    if (nchunks == 0 || p.typesize <= 0) return ERR_INVALID_PARAM;
    int filter = 0;
    // trunc-prec in slot 4 (trunc_plan.h): header and p must agree on it like on everything else; patched pixels are truncated before
    // they are encoded, so a new chunk equals the from-scratch compress of (old pixels with the windows written in), truncated
    uint64_t mask64 = 0;
    const int trunc = trunc_from_cparams(p.typesize, p.filters, p.filters_meta, &mask64);
    if (trunc < 0 || (trunc && !env_has_trunc<Env>::value)) return ERR_INVALID_PARAM;
    {
        HostCParams q;
        int32_t tb = 0;
        if (strip_trunc(p, trunc != 0, &q, &tb) < 0 || single_filter(q, &filter) < 0) return ERR_INVALID_PARAM;
    }
    const int ts = p.typesize > 255 ? 1 : p.typesize;
    for (int i = 0; i < nchunks; i++) if (destsize[i] < HEADER_LEN) return ERR_INVALID_PARAM;
    const std::vector<int32_t> tsv((size_t)nchunks, ts);
    Plan plan;
    if (plan_windows(nchunks, nbytes, blocksize, tsv.data(), nwindows, w, nullptr, &plan) < 0) return ERR_INVALID_PARAM;
    // (the tables index items and units with int32.  The limit is theoretical: 2^31 items of ~100 bytes are listed before it is
    // looked at, so a call that large runs out of memory first; it is here so that no count is ever narrowed silently)
    if (plan.items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;

    // the touched chunks' headers: damage is the chunk's status, disagreement with p the call's error
    std::vector<uint8_t> route((size_t)nchunks, ROUTE_NONE);
    std::vector<ChunkDesc> nd((size_t)nchunks);
    std::vector<int32_t> old_cbytes((size_t)nchunks, 0);
    std::vector<int> tl;
    for (int i = 0; i < nchunks; i++) if (plan.touched[(size_t)i]) tl.push_back(i);
    std::vector<uint8_t> hdrs(tl.size() * HEADER_LEN);
    if (!tl.empty()) {
        const int rc = env.headers(tl, hdrs.data());
        if (rc < 0) return rc;
    }
    for (size_t t = 0; t < tl.size(); t++) {
        const int i = tl[t];
        const uint8_t* h = hdrs.data() + t * HEADER_LEN;
        int32_t hnb, hbs, hcb;
        memcpy(&hnb, h + OFF_NBYTES, 4); memcpy(&hbs, h + OFF_BLOCKSIZE, 4); memcpy(&hcb, h + OFF_CBYTES, 4);
        int code = 0;
        if (h[0] > 5) code = ERR_VERSION_SUPPORT;
        else if (hcb < HEADER_LEN) code = ERR_INVALID_HEADER;
        else if (comp_size && hcb > comp_size[i]) code = ERR_READ_BUFFER;
        if (code) { status[i] = code; route[(size_t)i] = ROUTE_FAILED; continue; }
        ChunkDesc& d = nd[(size_t)i];
        if (plan_chunk(p, nbytes[i], destsize[i], &d) < 0) return ERR_INVALID_PARAM;
        const int flags = h[OFF_FLAGS];
        bool agree = hnb == nbytes[i] && hbs == blocksize[i] && hbs == d.blocksize && h[OFF_TYPESIZE] == ts &&
                     ((flags ^ d.flags) & ~FLAG_MEMCPYED) == 0 && h[OFF_COMPCODE] == p.compcode && h[OFF_FILTERS + 5] == filter;
        for (int k = 0; k < 4; k++) agree = agree && h[OFF_FILTERS + k] == 0;
        agree = agree && h[OFF_FILTERS + 4] == (trunc ? FILTER_TRUNC_PREC : 0) && (!trunc || h[OFF_FILTERS_META + 4] == p.filters_meta[4]);
        if (!agree) return ERR_INVALID_PARAM;
        old_cbytes[(size_t)i] = hcb;
        const int fmt = flags >> 5, special = (h[OFF_BLOSC2_FLAGS] >> 4) & 7;
        bool splice = !(flags & FLAG_MEMCPYED) && special == 0 && (fmt == 0 || fmt == 1) && !d.memcpyed && !decode_is_wide(hbs);
        if (splice) {
            EncodePlan ep;
            const int64_t zero = 0;
            splice = plan_encode_batch(p, 1, &zero, &nbytes[i], &zero, &destsize[i], &ep, trunc != 0) == 0;
        }
        route[(size_t)i] = splice ? ROUTE_SPLICE : ROUTE_WHOLE;
    }

    // ---- splice route ----
    std::vector<uint8_t> hint((size_t)nchunks, 0);
    for (int i = 0; i < nchunks; i++) hint[(size_t)i] = route[(size_t)i] != ROUTE_SPLICE;
    // (the plan above is this one already unless some touched chunk leaves the splice route.  The hint would change plan.whole[] for
    // chunks no window meets only, and those have no items; lds_bytes, descs and items depend on touched chunks alone.  This holds
    // only because NOTHING READS plan.whole[] PAST THIS POINT: code that starts to must re-plan here whenever the hint is not all zero
    // over the chunks it looks at, or the plain calls change without a sign.)
    bool replan = false;
    for (const int i : tl) replan = replan || route[(size_t)i] != ROUTE_SPLICE;
    if (replan && plan_windows(nchunks, nbytes, blocksize, tsv.data(), nwindows, w, hint.data(), &plan) < 0) return ERR_INVALID_PARAM;
    for (int i = 0; i < nchunks; i++) {
        plan.descs[(size_t)i].comp_off = plan.touched[(size_t)i] ? comp_off[i] : 0;
        plan.descs[(size_t)i].destsize = comp_size ? comp_size[i] : 0x7fffffff;
    }
    // the spliced chunks' items by block, call order kept inside a block: (block, index) keys are sorted and the items moved once
    std::vector<Item> blk_items;
    {
        std::vector<uint64_t> keys;
        keys.reserve(plan.items.size());
        for (size_t k = 0; k < plan.items.size(); k++) {
            const Item& t = plan.items[k];
            if (t.b >= 0 && route[(size_t)t.chunk] == ROUTE_SPLICE) keys.push_back(((uint64_t)(uint32_t)t.b << 32) | (uint64_t)k);
        }
        std::sort(keys.begin(), keys.end());
        blk_items.reserve(keys.size());
        for (const uint64_t key : keys) blk_items.push_back(plan.items[(size_t)(key & 0xffffffffu)]);
    }
    std::vector<std::pair<int64_t, int64_t>> iv;     // items_disjoint's table, one for the call
    std::vector<PatchUnit> units;
    std::vector<uint8_t> disjoint;                   // per unit: no two of its items write a common byte (strided calls)
    std::vector<WindowItem> stage;
    std::vector<int32_t> unit_b;
    int64_t patch_bytes = 0;
    for (size_t k = 0; k < blk_items.size();) {
        size_t e = k;
        while (e < blk_items.size() && blk_items[e].b == blk_items[k].b) e++;
        const Item& t = blk_items[k];
        const ChunkDesc& d = plan.descs[(size_t)t.chunk];
        const int j = t.b - d.blk0;
        const int64_t blen = (j == d.nblocks - 1 && d.leftover) ? d.leftover : d.blocksize;
        PatchUnit u{};
        u.chunk = t.chunk;
        u.stage = items_cover(blk_items, k, e - k, blen) ? 0 : 1;
        u.item0 = (int32_t)k; u.nitems = (int32_t)(e - k);
        u.len = blen; u.dst_off = patch_bytes;
        patch_bytes += (blen + 63) & ~(int64_t)63;
        WindowItem s{};
        s.chunk = t.chunk; s.b = u.stage ? t.b : -1;
        units.push_back(u); stage.push_back(s); unit_b.push_back(t.b);
        disjoint.push_back(items_disjoint(blk_items, k, e - k, blen, &iv) ? 1 : 0);
        k = e;
    }
    if (!units.empty()) {
        int rc = patch_units(env, plan.descs, plan.lds_bytes, units, disjoint, stage, blk_items, 0, patch_bytes, status);
        if (rc < 0) return rc;
        for (int i = 0; i < nchunks; i++) if (route[(size_t)i] == ROUTE_SPLICE && status[i] != 0) route[(size_t)i] = ROUTE_FAILED;
        // one-block pseudo-chunks with the parent's geometry (a short last block stays unsplit), no assembly
        std::vector<int> sl;
        std::vector<int64_t> zoff;
        std::vector<int32_t> snb, sds;
        for (int i = 0; i < nchunks; i++)
            if (route[(size_t)i] == ROUTE_SPLICE) { sl.push_back(i); snb.push_back(nbytes[i]); sds.push_back(destsize[i]); zoff.push_back(0); }
        EncodePlan ep;
        std::vector<int32_t> enc_of(units.size(), -1);
        if (!sl.empty()) {
            if (plan_encode_batch(p, (int)sl.size(), zoff.data(), snb.data(), zoff.data(), sds.data(), &ep, trunc != 0) < 0) return ERR_INVALID_PARAM;
            std::vector<ChunkDesc> pd;
            ep.lds_split = ep.lds_unsplit = 0;
            for (size_t k = 0; k < units.size(); k++) {
                const PatchUnit& u = units[k];
                if (route[(size_t)u.chunk] != ROUTE_SPLICE) continue;
                const ChunkDesc& par = nd[(size_t)u.chunk];
                ChunkDesc q{};
                q.raw_off = u.dst_off; q.comp_off = 0; q.nbytes = (int32_t)u.len; q.destsize = (int32_t)u.len + HEADER_LEN + 4 * MAX_STREAMS + 64;
                q.blocksize = par.blocksize; q.nblocks = 1; q.leftover = u.len != par.blocksize ? (int32_t)u.len : 0;
                q.blk0 = (int32_t)pd.size(); q.flags = par.flags; q.split = par.split; q.memcpyed = 0;
                q.nstreams = (q.split && !q.leftover) ? ep.cp.typesize : 1;
                q.assemble = 0;
                const bool multi = q.split && ep.cp.typesize > 1;
                if (q.leftover) ep.lds_unsplit = imax(ep.lds_unsplit, encode_lds_bytes(q.leftover, p.compcode));
                else if (multi) ep.lds_split = imax(ep.lds_split, encode_lds_bytes(q.blocksize / ep.cp.typesize, p.compcode));
                else ep.lds_unsplit = imax(ep.lds_unsplit, encode_lds_bytes(q.blocksize, p.compcode));
                enc_of[k] = (int32_t)pd.size();
                pd.push_back(q);
            }
            ep.descs = pd;
            ep.total_blocks = (int32_t)pd.size();
            ep.uniform_nblocks = 1;
            if constexpr (env_has_trunc<Env>::value) {
                if (trunc && !pd.empty()) {                  // the patched slots, in place (a block starts on an element boundary of its chunk)
                    std::vector<int64_t> toff;
                    std::vector<int32_t> tlen;
                    for (const ChunkDesc& q : pd) { toff.push_back(q.raw_off); tlen.push_back(q.nbytes); }
                    if ((rc = env.trunc(ts, mask64, toff, tlen)) < 0) return rc;
                }
            }
            if (!pd.empty() && (rc = env.encode(ep)) < 0) return rc;
            stats->blocks_encoded = (int64_t)pd.size();
            for (size_t k = 0; k < units.size(); k++) if (enc_of[k] >= 0 && units[k].stage) stats->blocks_decoded++;
            // the splice tables
            std::vector<SpliceChunk> sc;
            std::vector<SpliceBlock> sb;
            for (int i : sl) {
                const ChunkDesc& d = nd[(size_t)i];
                SpliceChunk c{};
                c.old_off = comp_off[i]; c.new_off = new_off[i]; c.old_cbytes = old_cbytes[(size_t)i]; c.destsize = destsize[i];
                c.nbytes = d.nbytes; c.blocksize = d.blocksize; c.nblocks = d.nblocks; c.leftover = d.leftover;
                c.split = d.split; c.flags = d.flags; c.blk0 = (int32_t)sb.size(); c.nstreams = d.nstreams;
                for (int j = 0; j < d.nblocks; j++) sb.push_back(SpliceBlock{(int32_t)sc.size(), j, -1, 0, 0, 0});
                sc.push_back(c);
            }
            std::vector<int32_t> sc_of((size_t)nchunks, -1);
            for (size_t k = 0; k < sl.size(); k++) sc_of[(size_t)sl[k]] = (int32_t)k;
            for (size_t k = 0; k < units.size(); k++) {
                if (enc_of[k] < 0) continue;
                const int i = units[k].chunk;
                const int j = unit_b[k] - plan.descs[(size_t)i].blk0;
                sb[(size_t)(sc[(size_t)sc_of[(size_t)i]].blk0 + j)].unit = enc_of[k];
            }
            std::vector<ChunkLayout> lay(sc.size());
            if ((rc = env.splice(ep.cp, sc, sb, lay)) < 0) return rc;
            for (size_t k = 0; k < sl.size(); k++) {
                const int i = sl[k];
                const ChunkLayout& L = lay[k];
                if (L.mode == SPLICE_REGULAR || L.mode == SPLICE_ZERO) new_cbytes[i] = L.cbytes;
                else if (L.mode == SPLICE_WHOLE) route[(size_t)i] = ROUTE_WHOLE;
                else { status[i] = L.cbytes < 0 ? L.cbytes : ERR_DATA; route[(size_t)i] = ROUTE_FAILED; }
            }
        }
    }

    // ---- whole route (and the splice route's hand-backs) ----
    std::vector<int> wl;
    std::vector<int64_t> woff;
    int64_t wtotal = 0;
    for (int i = 0; i < nchunks; i++)
        if (route[(size_t)i] == ROUTE_WHOLE) { wl.push_back(i); woff.push_back(wtotal); wtotal += ((int64_t)nbytes[i] + 255) & ~(int64_t)255; }
    if (!wl.empty()) {
        std::vector<int32_t> st(wl.size(), 0);
        int rc = env.decode_whole(wl, woff, wtotal, st.data());
        if (rc < 0) return rc;
        stats->chunks_whole = (int64_t)wl.size();
        for (int i = 0; i < nchunks; i++) hint[(size_t)i] = route[(size_t)i] == ROUTE_WHOLE;
        if (plan_windows(nchunks, nbytes, blocksize, tsv.data(), nwindows, w, hint.data(), &plan) < 0) return ERR_INVALID_PARAM;
        std::vector<int64_t> at((size_t)nchunks, -1);
        std::vector<int> ok;
        std::vector<int64_t> okoff;
        for (size_t k = 0; k < wl.size(); k++) {
            if (st[k] != 0) { status[wl[k]] = st[k]; route[(size_t)wl[k]] = ROUTE_FAILED; continue; }
            at[(size_t)wl[k]] = woff[k];
            ok.push_back(wl[k]); okoff.push_back(woff[k]);
        }
        std::vector<Item> items;
        std::vector<PatchUnit> wunits;
        std::vector<uint8_t> wdisjoint;
        std::vector<WindowItem> wstage;
        for (int i : ok) {
            PatchUnit u{};
            u.chunk = i; u.stage = 0; u.item0 = (int32_t)items.size();
            u.len = nbytes[i]; u.dst_off = at[(size_t)i];
            for (const Item& t : plan.items) if (t.b < 0 && t.chunk == i) items.push_back(t);
            u.nitems = (int32_t)items.size() - u.item0;
            wdisjoint.push_back(items_disjoint(items, (size_t)u.item0, (size_t)u.nitems, u.len, &iv) ? 1 : 0);
            WindowItem s{};
            s.chunk = i; s.b = -1;
            wunits.push_back(u); wstage.push_back(s);
        }
        if (!ok.empty()) {
            if ((rc = patch_units(env, plan.descs, 0, wunits, wdisjoint, wstage, items, 1, wtotal, status)) < 0) return rc;
            std::vector<int32_t> nb, ds, cb(ok.size(), 0);
            std::vector<int64_t> no;
            for (int i : ok) { nb.push_back(nbytes[i]); ds.push_back(destsize[i]); no.push_back(new_off[i]); }
            if ((rc = env.compress(p, ok, okoff, nb, ds, no, cb.data())) < 0) return rc;
            for (size_t k = 0; k < ok.size(); k++) new_cbytes[ok[k]] = cb[k];
        }
    }
    for (int i = 0; i < nchunks; i++) if (status[i] != 0) return status[i];
    return 0;
}

// ---- the host-buffer call: what is decided before anything is staged -------------------------------------------------------------

// The opening of a write call (new_chunks: the host call's): < 0 refused, CALL_DONE nothing to do, 0 go on.  Chunks are asked for
// later: by the host call once its pointers are known to be good, by run_update for the device call.
inline int open_update_call(int nchunks, int nwindows, int32_t* status, int32_t* new_cbytes, void** new_chunks)
{
    if (nchunks < 0 || nwindows < 0) return ERR_INVALID_PARAM;
    if (status) for (int i = 0; i < nchunks; i++) status[i] = 0;
    if (new_cbytes) for (int i = 0; i < nchunks; i++) new_cbytes[i] = 0;
    if (new_chunks) for (int i = 0; i < nchunks; i++) new_chunks[i] = nullptr;
    return nwindows == 0 ? CALL_DONE : 0;
}

struct UpdateHostPlan : HostCallPlan {
    std::vector<int32_t> held;          // the bytes the caller holds of each chunk: comp_size, or what the header says
    std::vector<int64_t> new_off;       // the touched chunks' new forms, in 64-byte slots of destsize each
    int64_t new_total = 0, new_used = 0, bytes_uploaded = 0;
    // masked calls: the mask rows of the masked windows packed one after the other (mask_pitch = width), each at a multiple of 64
    std::vector<int64_t> mbytes;
    int64_t mask_total = 0, mask_used = 0;
};

// the windows of a masked call as the device sees them: the rows of the windows that have a source packed as pack_rows packs them,
// the mask rows of the masked ones packed likewise in a buffer of their own; a constant window sends no rows, an unmasked one no mask
inline void pack_rows(int nwindows, const MaskedWindowSpec* w, const int32_t* typesize, UpdateHostPlan* hp, std::vector<MaskedWindowSpec>* dw)
{
    dw->assign(w, w + nwindows);
    hp->wbytes.assign((size_t)nwindows, 0);
    hp->mbytes.assign((size_t)nwindows, 0);
    for (int k = 0; k < nwindows; k++) {
        if (w[k].width <= 0 || w[k].height <= 0) continue;
        MaskedWindowSpec& d = (*dw)[(size_t)k];
        if (!(w[k].flags & WM_CONST)) {
            const int64_t row = (int64_t)w[k].width * typesize[w[k].chunk_first];
            d.out_off = hp->rows_total;
            d.out_pitch = row;
            hp->wbytes[(size_t)k] = row * w[k].height;
            hp->rows_used = hp->rows_total + hp->wbytes[(size_t)k];
            hp->rows_total += (hp->wbytes[(size_t)k] + 255) & ~255ll;
        }
        if (w[k].flags & WM_MASK) {
            d.mask_off = hp->mask_total;
            d.mask_pitch = w[k].width;
            hp->mbytes[(size_t)k] = (int64_t)w[k].width * w[k].height;
            hp->mask_used = hp->mask_total + hp->mbytes[(size_t)k];
            hp->mask_total += (hp->mbytes[(size_t)k] + 63) & ~63ll;
        }
    }
}

// cimg_update_windows_host: only the touched chunks go up, and a header that claims more than the buffer holds is the chunk's
// own error, found by run_update (hence `up`: what is there to copy, a header at least).  ERR_INVALID_PARAM with bad_window < 0:
// the typesize or a window was refused.
// (dw: the packed windows -- hp->dw, or the strided call's list)
template <class Spec>
inline int plan_update_host(int typesize, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                            const int32_t* destsize, int nwindows, const Spec* w, int32_t* status, UpdateHostPlan* hp, std::vector<Spec>* dw)
{
    const int rc = read_named_headers(nchunks, comp, comp_off, comp_size, nwindows, w, hp);
    if (hp->short_chunk >= 0) status[hp->short_chunk] = rc;
    if (rc < 0) return rc;
    if (typesize <= 0) return ERR_INVALID_PARAM;
    const std::vector<int32_t> tsv((size_t)nchunks, typesize > 255 ? 1 : typesize);
    typename PlanOf<Spec>::type plan;
    if (plan_windows(nchunks, hp->nbytes.data(), hp->blocksize.data(), tsv.data(), nwindows, w, nullptr, &plan) < 0) return ERR_INVALID_PARAM;
    if (plan.items.size() > (size_t)INT32_MAX) return ERR_INVALID_PARAM;
    hp->held.assign((size_t)nchunks, 0);
    hp->new_off.assign((size_t)nchunks, 0);
    for (int i = 0; i < nchunks; i++) {
        const int32_t cb = hp->cbytes[(size_t)i];
        hp->held[(size_t)i] = comp_size ? comp_size[i] : cb;
        if (!plan.touched[(size_t)i]) continue;
        stage_chunk(hp, i, std::max((int32_t)HEADER_LEN, std::min(cb, hp->held[(size_t)i])));
        hp->new_off[(size_t)i] = hp->new_total;
        hp->new_used = hp->new_total + std::max(destsize[i], 0);
        hp->new_total += ((int64_t)std::max(destsize[i], 0) + 63) & ~63ll;
    }
    pack_rows(nwindows, w, tsv.data(), hp, dw);
    hp->bytes_uploaded = hp->comp_bytes_uploaded;
    for (const int64_t b : hp->wbytes) hp->bytes_uploaded += b;
    for (const int64_t b : hp->mbytes) hp->bytes_uploaded += b;      // (masked calls only: the table is empty otherwise)
    return 0;
}
inline int plan_update_host(int typesize, int nchunks, const uint8_t* comp, const int64_t* comp_off, const int32_t* comp_size,
                            const int32_t* destsize, int nwindows, const WindowSpec* w, int32_t* status, UpdateHostPlan* hp)
{
    return plan_update_host(typesize, nchunks, comp, comp_off, comp_size, destsize, nwindows, w, status, hp, &hp->dw);
}

}  // namespace cimg
