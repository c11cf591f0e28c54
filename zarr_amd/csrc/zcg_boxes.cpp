// zcg_boxes.cpp — the store-level calls for many boxes and for a list of
// coordinates (ZarrNdarrayReader::read_ndarray, src/ndarray.rs:153-268, and
// write_ndarray, ndarray.rs:276-385, once per box in the reference): plan, then
// one driver.
//
// Plan (before any file is opened).  plan_head checks what `meta` alone decides
// and fills the region descriptor all items share; plan_boxes and plan_points
// add the in-grid check of every visited chunk and take the items in
// consecutive groups whose unique chunks fit a budget of decoded device slots
// (a chunk two groups share is decoded in each), each group with its union
// table range.  A strided box's chunks (the _s calls) are the touched ones
// (zcg_region_s_chunks), not the hull's whole grid range; points are sorted by
// chunk first, so a group is a run of sorted points.  plan_ortho sorts every
// list of an orthogonal selection by itself; its groups are sub-products of
// runs of the sorted lists, so no chunk is shared between two groups.
//
// Driver.  run_groups is the per-group loop, once for both directions and both
// kinds of item.  It owns the stream, the group's slots and chunk files, which
// chunks are read first, the chunk table, the absent list and its fill, the one
// synchronisation per group (also the one place where an error after an
// enqueued copy waits before the host vectors go out of scope), the per-chunk
// failure report and, on the write side, the one encode-and-write of every
// chunk of the group.
//   read:  every chunk of the group is read and decoded once; an absent one is
//          a NULL table entry.  A group without chunks still launches: items
//          outside every chunk get fill.
//   write: a group without chunks is skipped; only chunks with read_first set
//          are read (boxes: those whose first visiting box leaves part of them
//          uncovered; points: all, unless a chunk is one element), absent ones
//          start as fill value; nothing is written if a step before failed.
//
// Payloads.  What is scattered or assembled is the payload's business: its part
// of the group's device block, its staging and bounce copies, its launches, its
// status check and its host copy-back.
//   BoxPayload:    [records nb][status nb][scratch of the _v kernels].  One
//                  shape for all boxes keeps the one-shape kernels
//                  (zcg_read_regions / zcg_write_regions), a shape per box the
//                  _v kernels, a step per box and dimension the _s kernels.  A
//                  read is one launch; a write is one launch per wave of
//                  zcg_regions[_v|_s]_waves, so a later box wins.  Host callers
//                  get one copy per group, straight to or from their memory
//                  when the boxes are consecutive, else through a bounce buffer.
//   PointsPayload: [coordinates np * nd][original indices np][first-outside
//                  word].  One launch (zcg_region_p.hip); a device caller's
//                  values stay in the caller's order through the index array,
//                  host values are permuted on the host.
//   OrthoPayload:  [indices, per dimension][their positions][scratch of the
//                  kernels][outside words].  One launch (zcg_region_o.hip) for
//                  the group's runs of the sorted lists; the values stay in the
//                  caller's order through the positions, a host caller's in
//                  one device array for the whole call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "zcg_common.h"

namespace zcg {
void ctx_set_error(zcg_ctx* ctx, const std::string& e);
int ctx_device(zcg_ctx* ctx);
}  // namespace zcg

namespace {

using namespace zcg;

constexpr uint64_t BOXES_DEFAULT_BUDGET = 4ull << 30;
constexpr uint64_t BOXES_MAX_TABLE = 1ull << 24;

// lib.rs:340-342, kept verbatim with its over-count when a % b == b - 1
uint64_t u64_ceil_div(uint64_t a, uint64_t b) { return (a + 1) / b + (a % b != 0 ? 1 : 0); }

struct DevMem {
    void* p = nullptr;
    ~DevMem() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)); }
};
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

struct Group {
    uint32_t b0, b1;
    std::vector<uint64_t> keys;  // unique visited chunks, as linear indices over the array's grid, ascending
    std::vector<uint8_t> read_first;  // write: per key, 1 = the chunk's file is read before the scatter
};

std::string pos_text(const uint64_t* pos, uint32_t nd) {
    std::string s = "[";
    for (uint32_t d = 0; d < nd; d++) s += (d ? ", " : "") + std::to_string(pos[d]);
    return s + "]";
}

int fail_hip(zcg_ctx* ctx, hipError_t e, const std::string& what) {
    ctx_set_error(ctx, what + ": " + hipGetErrorString(e));
    return ZCG_ERR_RUNTIME;
}

// What the box calls plan before any file is read or written: the region
// descriptor every box shares, and the boxes in consecutive groups with each
// group's unique chunks and union table range.
struct Plan {
    zcg_region r;
    uint32_t nd = 0, es = 0;
    uint64_t D = 0;                     // bytes of a decoded chunk
    bool varied = false;                // a shape per box (the _v calls); r.bbox_shape is then their bound
    const uint64_t* shapes = nullptr;   // box b's shape: shapes + b * sstep
    const int64_t* strides = nullptr;   // varied, device views: box b's strides, strides + b * nd; NULL: dense
    const uint64_t* steps = nullptr;    // the _s calls (varied): box b's steps, steps + b * nd; shapes are sample counts
    size_t sstep = 0;
    std::vector<uint64_t> at;           // byte offset of box b among the boxes back to back, dense (n_boxes + 1)
    uint64_t extent[ZCG_MAX_DIMS];      // the array's chunk grid
    uint64_t gstr[ZCG_MAX_DIMS];        // linear chunk keys over the array's grid
    uint64_t budget = 0;                // bytes of decoded slots a group may hold
    bool nothing = false;               // no box, no point: the call is done
    std::vector<Group> groups;
    std::vector<uint64_t> glo, gn, gentries;  // per group: table range (ZCG_MAX_DIMS each), entries

    const uint64_t* shape_of(uint32_t b) const { return shapes + (size_t)b * sstep; }
    uint64_t box_bytes(uint32_t b) const { return at[b + 1] - at[b]; }
    // varied shapes: box b's view strides per array dim, the caller's or dense in the chunk memory order
    void strides_of(uint32_t b, int64_t* out) const {
        if (strides) {
            for (uint32_t d = 0; d < nd; d++) out[d] = strides[(size_t)b * nd + d];
            return;
        }
        int64_t acc = 1;
        for (uint32_t k = 0; k < nd; k++) {
            const uint32_t d = r.chunk_order == 1 ? k : nd - 1 - k;
            out[d] = acc;
            acc *= (int64_t)std::max<uint64_t>(shape_of(b)[d], 1);
        }
    }
    void key_pos(uint64_t key, uint64_t* pos) const {
        for (uint32_t d = 0; d < nd; d++) { pos[d] = key / gstr[d]; key -= pos[d] * gstr[d]; }
    }
};

// What the box calls refuse from `meta` alone, and what the strided calls
// refuse from one box's sample counts and steps alone.  `say` receives the
// message; plan_boxes and the context-free check of the strided write entries
// (strided_write_args) both go through these, so the rules exist once.
template <class Say>
int meta_args_status(const std::string& what, const zcg_array_meta* meta, Say say) {
    if (meta->ndim != meta->chunk_ndim) {
        say(what + ": shape and chunk_shape differ in their number of dimensions");
        return ZCG_ERR_INVALID_DATA;
    }
    if (meta->ndim < 1 || meta->ndim > ZCG_MAX_DIMS) return ZCG_ERR_INVALID_INPUT;
    if (meta->dtype_kind == ZCG_DT_RAW) {
        say(what + ": raw (rN) element types have no ndarray form");
        return ZCG_ERR_INVALID_INPUT;
    }
    return ZCG_OK;
}

template <class Say>
int sbox_args_status(const std::string& what, uint32_t b, uint32_t nd, const uint64_t* counts, const uint64_t* stp,
                     const uint64_t* chunk_shape, Say say) {
    for (uint32_t d = 0; d < nd; d++) {
        const uint64_t c = counts[d];
        if (stp[d] == 0) {
            say(what + ": box " + std::to_string(b) + " has a step of 0");
            return ZCG_ERR_INVALID_INPUT;
        }
        if (c > 1 && (stp[d] >= (1ull << 32) || c > (1ull << 32) || (c - 1) * stp[d] + chunk_shape[d] >= (1ull << 32))) {
            say(what + ": box " + std::to_string(b) +
                ": hull extent + chunk extent along a dimension must stay below 2^32");
            return ZCG_ERR_UNSUPPORTED;
        }
    }
    return ZCG_OK;
}

// What plan_boxes and plan_points share, up to "nothing to do" (P.nothing) and
// on to the region descriptor and the array's chunk grid.  It comes in two
// parts, because plan_boxes refuses boxes above 2^62 bytes between them and a
// call that is wrong in two ways keeps its status.  `where` and `bufs`: the
// items' positions and memory, NULL only without items; `items` names them in
// the refusal of 2^32 and more (Group::b0 / b1 are 32-bit).
int plan_head(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root, const char* path,
              const void* where, const void* bufs, uint64_t n, const char* items, bool fill_missing, Plan& P) {
    if (!ctx || !meta || !root || !path) return ZCG_ERR_INVALID_INPUT;
    if (n && (!where || !bufs)) return ZCG_ERR_INVALID_INPUT;
    const int mrc = meta_args_status(what, meta, [&](const std::string& e) { ctx_set_error(ctx, e); });
    if (mrc != ZCG_OK) return mrc;
    const uint32_t nd = meta->ndim;
    const uint32_t es = meta->array.dtype.elem_size;
    if (es != 1 && es != 2 && es != 4 && es != 8) return ZCG_ERR_INVALID_INPUT;
    P.nd = nd;
    P.es = es;
    P.D = meta->array.chunk_num_elements * (uint64_t)es;
    if (n == 0) {
        P.nothing = true;
        return ZCG_OK;
    }
    if (n >= (1ull << 32)) {
        ctx_set_error(ctx, what + ": more than 2^32 " + items + " in one call");
        return ZCG_ERR_UNSUPPORTED;
    }
    zcg_region& r = P.r;
    memset(&r, 0, sizeof r);
    r.ndim = nd;
    r.elem_size = es;
    r.chunk_order = meta->chunk_order;
    r.fill_missing = fill_missing ? 1u : 0u;
    r.fill_value = meta->has_fill_value ? meta->fill_value : 0;
    for (uint32_t d = 0; d < nd; d++) {
        if (meta->chunk_shape[d] == 0) return ZCG_ERR_INVALID_INPUT;
        r.array_shape[d] = meta->shape[d];
        r.chunk_shape[d] = meta->chunk_shape[d];
        P.extent[d] = u64_ceil_div(meta->shape[d], meta->chunk_shape[d]);
    }
    return ZCG_OK;
}

// plan_head's second part: linear chunk keys over the grid, and the budget
int plan_head_grid(zcg_ctx* ctx, const std::string& what, uint64_t slot_budget_bytes, Plan& P) {
    uint64_t g = 1;
    for (int d = (int)P.nd - 1; d >= 0; d--) {
        P.gstr[d] = g;
        if (P.extent[d] && g > (~0ull) / P.extent[d]) {
            ctx_set_error(ctx, what + ": the array's chunk grid exceeds 2^64 chunks");
            return ZCG_ERR_UNSUPPORTED;
        }
        g *= P.extent[d];
    }
    P.budget = slot_budget_bytes ? slot_budget_bytes : BOXES_DEFAULT_BUDGET;
    return ZCG_OK;
}

// Argument checks, the in-bounds check of every visited chunk (the reference
// panics at storage.rs:217) and the grouping under the slot budget.  `what`
// prefixes the messages.  host == true: boxes are host buffers, each dense in
// the chunk memory order; else device views with the caller's strides.
// varied == false: every box has the shape box_shape (ndim) and, as a device
// view, the strides `strides` (ndim); true: box_shape and strides hold
// n_boxes * ndim entries, box-major, and NULL strides mean dense views.
// cover == true (write): Group::read_first is filled in.  box_steps (varied):
// n_boxes * ndim steps, box_shape then holds sample counts and a box's
// chunks are the touched ones; NULL: dense boxes.
int plan_boxes(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root, const char* path,
               const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* strides, bool varied,
               uint32_t fill_missing,
               const uint64_t* offsets, const void* const* bufs, uint32_t n_boxes, uint64_t slot_budget_bytes,
               bool host, bool cover, Plan& P) {
    if ((!box_shape && !(varied && n_boxes == 0)) || (!host && !strides && !varied)) return ZCG_ERR_INVALID_INPUT;
    auto say = [&](const std::string& e) { ctx_set_error(ctx, e); };
    const int hrc = plan_head(ctx, what, meta, root, path, offsets, bufs, n_boxes, "boxes", host || fill_missing, P);
    if (hrc != ZCG_OK || P.nothing) return hrc;
    const uint32_t nd = P.nd, es = P.es;
    zcg_region& r = P.r;
    const uint64_t *gstr = P.gstr, *extent = P.extent;
    P.varied = varied;
    P.shapes = box_shape;
    P.sstep = varied ? nd : 0;
    P.strides = varied && !host ? strides : nullptr;
    P.steps = box_steps;
    // the boxes back to back, and the bound of their extents
    P.at.assign((size_t)n_boxes + 1, 0);
    for (uint32_t b = 0; b < n_boxes; b++) {
        uint64_t elems = 1;
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t s = P.shape_of(b)[d];
            r.bbox_shape[d] = std::max(r.bbox_shape[d], s);
            elems = s && elems > (1ull << 62) / s ? 1ull << 62 : elems * s;
        }
        if (elems >= (1ull << 62) / es || P.at[b] + elems * es < P.at[b]) {
            ctx_set_error(ctx, what + ": the boxes hold more than 2^62 bytes");
            return ZCG_ERR_UNSUPPORTED;
        }
        P.at[b + 1] = P.at[b] + elems * es;
    }
    {   // dense host layout in the chunk memory order
        int64_t acc = 1;
        for (uint32_t k = 0; k < nd; k++) {
            const uint32_t d = meta->chunk_order == 1 ? k : nd - 1 - k;
            r.out_strides[d] = varied ? 0 : host ? acc : strides[d];
            acc *= (int64_t)std::max<uint64_t>(r.bbox_shape[d], 1);
        }
    }
    const int grc = plan_head_grid(ctx, what, slot_budget_bytes, P);
    if (grc != ZCG_OK) return grc;
    const uint64_t D = P.D, budget = P.budget;

    // every box's visited chunks: in bounds, grouped under the slot budget.
    // seen: chunk key -> does the group's first box to visit it leave part of
    // its nominal bounds uncovered (write: the chunk is read first)
    std::vector<Group>& groups = P.groups;
    {
        std::unordered_map<uint64_t, uint8_t> seen;
        std::vector<uint64_t> fresh;
        Group cur{0, 0, {}, {}};
        auto close = [&](uint32_t b1) {
            cur.b1 = b1;
            cur.keys.reserve(seen.size());
            for (const auto& kv : seen) cur.keys.push_back(kv.first);
            std::sort(cur.keys.begin(), cur.keys.end());
            if (cover) {
                cur.read_first.reserve(seen.size());
                for (uint64_t k : cur.keys) cur.read_first.push_back(seen[k]);
            }
            groups.push_back(std::move(cur));
        };
        std::vector<uint8_t> touched;
        std::vector<uint64_t> cell[ZCG_MAX_DIMS];  // strided: the touched grid indices per dimension
        for (uint32_t b = 0; b < n_boxes; b++) {
            uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS], pos[ZCG_MAX_DIMS];
            zcg_region rb = r;  // this box alone
            for (uint32_t d = 0; d < nd; d++) {
                rb.bbox_offset[d] = offsets[(size_t)b * nd + d];
                rb.bbox_shape[d] = P.shape_of(b)[d];
            }
            // cnt chunks to read, out of a grid range of `range` chunks; chunk i is
            // at lo[d] + i_d, or for a strided box at cell[d][i_d], i_d < m[d]
            uint64_t cnt, range, m[ZCG_MAX_DIMS];
            if (box_steps) {
                const uint64_t* stp = box_steps + (size_t)b * nd;
                const int brc = sbox_args_status(what, b, nd, rb.bbox_shape, stp, rb.chunk_shape, say);
                if (brc != ZCG_OK) return brc;
                cnt = zcg_region_s_chunks(&rb, rb.bbox_offset, rb.bbox_shape, stp, lo, n, nullptr);
                range = cnt ? 1 : 0;
                for (uint32_t d = 0; cnt && d < nd; d++)
                    range = n[d] > BOXES_MAX_TABLE || range * n[d] > BOXES_MAX_TABLE ? BOXES_MAX_TABLE + 1 : range * n[d];
                if (cnt && range <= BOXES_MAX_TABLE) {
                    uint64_t sum = 0;
                    for (uint32_t d = 0; d < nd; d++) sum += n[d];
                    touched.assign(sum, 0);
                    zcg_region_s_chunks(&rb, rb.bbox_offset, rb.bbox_shape, stp, lo, n, touched.data());
                    const uint8_t* tp = touched.data();
                    for (uint32_t d = 0; d < nd; d++) {
                        cell[d].clear();
                        for (uint64_t j = 0; j < n[d]; j++)
                            if (tp[j]) cell[d].push_back(lo[d] + j);
                        tp += n[d];
                        m[d] = cell[d].size();
                    }
                }
            } else {
                cnt = range = zcg_region_grid(&rb, lo, n);
                for (uint32_t d = 0; d < nd; d++) m[d] = n[d];
            }
            if (range > BOXES_MAX_TABLE) {
                ctx_set_error(ctx, what + ": a chunk table above 2^24 entries is not supported");
                return ZCG_ERR_UNSUPPORTED;
            }
            auto at = [&](uint32_t d, uint64_t i) { return box_steps ? cell[d][i] : lo[d] + i; };
            for (uint32_t d = 0; cnt && d < nd; d++)
                if (at(d, m[d] - 1) >= extent[d]) {
                    for (uint32_t k = 0; k < nd; k++) pos[k] = at(k, m[k] - 1);
                    ctx_set_error(ctx, what + ": box " + std::to_string(b) + " visits chunk " + pos_text(pos, nd) +
                                           " outside the array's chunk grid");
                    return ZCG_ERR_INVALID_INPUT;
                }
            auto visit = [&]() {
                fresh.clear();
                for (uint64_t i = 0; i < cnt; i++) {
                    uint64_t rem = i, key = 0;
                    bool part = false;
                    for (int d = (int)nd - 1; d >= 0; d--) {
                        const uint64_t c = at((uint32_t)d, rem % m[d]);
                        key += c * gstr[d];
                        rem /= m[d];
                        if (cover) {  // write_bb == nom_chunk_bb (ndarray.rs:327), per dimension
                            const uint64_t cs = rb.chunk_shape[d], o = rb.bbox_offset[d], o1 = o + rb.bbox_shape[d];
                            // strided: every index of the chunk's nominal bounds must be a sample.  A
                            // touched chunk of extent 1 is its one sample; a wider one needs step 1
                            // (a lone sample has none) and the run of samples across it
                            const uint64_t stp = box_steps && rb.bbox_shape[d] > 1 ? box_steps[(size_t)b * nd + d] : 1;
                            const bool unit = box_steps && cs == 1;
                            part |= !unit && (stp != 1 || c * cs < o || c * cs + cs > (o1 < o ? ~0ull : o1));
                        }
                    }
                    if (seen.emplace(key, part ? 1 : 0).second) fresh.push_back(key);
                }
            };
            visit();
            if (b > cur.b0 && (uint64_t)seen.size() > budget / std::max<uint64_t>(D, 1)) {
                // this box does not fit beside the others: it starts the next group
                for (uint64_t k : fresh) seen.erase(k);
                close(b);
                cur = Group{b, b, {}, {}};
                seen.clear();
                visit();
            }
        }
        close(n_boxes);
    }
    P.glo.resize(groups.size() * ZCG_MAX_DIMS);
    P.gn.resize(groups.size() * ZCG_MAX_DIMS);
    P.gentries.resize(groups.size());
    for (size_t g = 0; g < groups.size(); g++) {
        const Group& G = groups[g];
        P.gentries[g] =
            box_steps ? zcg_regions_s_grid(&r, offsets + (size_t)G.b0 * nd, box_shape + (size_t)G.b0 * nd,
                                           box_steps + (size_t)G.b0 * nd, G.b1 - G.b0, &P.glo[g * ZCG_MAX_DIMS],
                                           &P.gn[g * ZCG_MAX_DIMS]) :
            varied ? zcg_regions_v_grid(&r, offsets + (size_t)G.b0 * nd, box_shape + (size_t)G.b0 * nd, G.b1 - G.b0,
                                        &P.glo[g * ZCG_MAX_DIMS], &P.gn[g * ZCG_MAX_DIMS])
                   : zcg_regions_grid(&r, offsets + (size_t)G.b0 * nd, G.b1 - G.b0, &P.glo[g * ZCG_MAX_DIMS],
                                      &P.gn[g * ZCG_MAX_DIMS]);
        if (P.gentries[g] > BOXES_MAX_TABLE) {
            ctx_set_error(ctx, what + ": the boxes' union chunk table (" + std::to_string(P.gentries[g]) +
                                   " entries) exceeds 2^24; split the boxes over several calls");
            return ZCG_ERR_UNSUPPORTED;
        }
    }
    return ZCG_OK;
}

// The chunk files and device slots of a group: slot i (D bytes, packed) and
// file i belong to chunk G.keys[i], table index tidx[i].
struct GroupSlots {
    DevMem slots;
    std::vector<std::string> paths;
    std::vector<const char*> cpaths;
    std::vector<void*> ptrs;
    std::vector<uint64_t> tidx;
};

int group_slots(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root,
                const char* path, const Plan& P, size_t g, GroupSlots& S) {
    const Group& G = P.groups[g];
    const uint32_t nd = P.nd, m = (uint32_t)G.keys.size();
    const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
    const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
    const hipError_t e = S.slots.alloc((size_t)m * P.D);
    if (e != hipSuccess) return fail_hip(ctx, e, (what + " slots").c_str());
    S.paths.resize(m);
    S.cpaths.resize(m);
    S.ptrs.resize(m);
    S.tidx.resize(m);
    std::string key;
    for (uint32_t i = 0; i < m; i++) {
        uint64_t pos[ZCG_MAX_DIMS], ti = 0, tstr = 1;
        P.key_pos(G.keys[i], pos);
        for (int d = (int)nd - 1; d >= 0; d--) { ti += (pos[d] - lo[d]) * tstr; tstr *= n[d]; }
        S.tidx[i] = ti;
        key.resize(zcg_chunk_key(path, meta->separator, pos, nd, nullptr, 0) + 1);
        zcg_chunk_key(path, meta->separator, pos, nd, &key[0], key.size());
        uint64_t plen = 0;
        int rc = zcg_store_path(root, key.c_str(), nullptr, 0, &plen);
        if (rc == ZCG_OK) {
            S.paths[i].resize(plen + 1);
            rc = zcg_store_path(root, key.c_str(), &S.paths[i][0], plen + 1, nullptr);
        }
        if (rc != ZCG_OK) {
            ctx_set_error(ctx, what + ": chunk " + pos_text(pos, nd) + ": key outside the hierarchy");
            return rc;
        }
        S.cpaths[i] = S.paths[i].c_str();
        S.ptrs[i] = (uint8_t*)S.slots.p + (size_t)i * P.D;
    }
    return ZCG_OK;
}

int chunk_failed(zcg_ctx* ctx, const std::string& what, const Plan& P, uint64_t key, int32_t status) {
    uint64_t pos[ZCG_MAX_DIMS];
    P.key_pos(key, pos);
    ctx_set_error(ctx, what + ": chunk " + pos_text(pos, P.nd) + ": status " + std::to_string(status));
    return status;
}

// The records of boxes b0 .. b0 + nb as the region kernels take them: zcg_box
// for one shape, zcg_vbox (shape and strides per box) for varied shapes.  Box
// b's view is bufs[b], or, host == true, its place in the dense staging buffer.
size_t record_bytes(const Plan& P) {
    return P.steps ? sizeof(zcg_sbox) : P.varied ? sizeof(zcg_vbox) : sizeof(zcg_box);
}

std::vector<uint8_t> box_records(const Plan& P, const uint64_t* offsets, const void* const* bufs, void* staging,
                                 uint32_t b0, uint32_t nb, bool host) {
    std::vector<uint8_t> recs((size_t)nb * record_bytes(P), 0);
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t b = b0 + i;
        void* view = host ? (void*)((uint8_t*)staging + (P.at[b] - P.at[b0])) : (void*)bufs[b];
        if (P.steps) {
            zcg_sbox& x = ((zcg_sbox*)recs.data())[i];
            for (uint32_t d = 0; d < P.nd; d++) {
                x.offset[d] = offsets[(size_t)b * P.nd + d];
                x.shape[d] = P.shape_of(b)[d];
                x.step[d] = P.steps[(size_t)b * P.nd + d];
            }
            P.strides_of(b, x.strides);
            x.base = view;
        } else if (P.varied) {
            zcg_vbox& x = ((zcg_vbox*)recs.data())[i];
            for (uint32_t d = 0; d < P.nd; d++) {
                x.offset[d] = offsets[(size_t)b * P.nd + d];
                x.shape[d] = P.shape_of(b)[d];
            }
            P.strides_of(b, x.strides);
            x.base = view;
        } else {
            zcg_box& x = ((zcg_box*)recs.data())[i];
            for (uint32_t d = 0; d < P.nd; d++) x.offset[d] = offsets[(size_t)b * P.nd + d];
            x.out = view;
        }
    }
    return recs;
}

// One region call for records first .. first + count of a group (dir 0:
// assemble, 1: scatter): the one-shape kernels, or the _v kernels for varied
// shapes (d_scratch: zcg_regions_v_scratch_bytes(count) bytes).
int regions_launch(zcg_ctx* ctx, const Plan& P, const uint64_t* lo, const uint64_t* n, void* d_table, void* d_recs,
                   uint32_t first, uint32_t count, void* d_scratch, int32_t* d_status, hipStream_t s, uint32_t dir) {
    if (P.steps) {
        const zcg_sbox* bx = (const zcg_sbox*)d_recs + first;
        return dir ? zcg_write_regions_s(ctx, &P.r, lo, n, (void* const*)d_table, bx, count, d_scratch,
                                         d_status + first, (void*)s)
                   : zcg_read_regions_s(ctx, &P.r, lo, n, (const void* const*)d_table, bx, count, d_scratch,
                                        d_status + first, (void*)s);
    }
    if (P.varied) {
        const zcg_vbox* bx = (const zcg_vbox*)d_recs + first;
        return dir ? zcg_write_regions_v(ctx, &P.r, lo, n, (void* const*)d_table, bx, count, d_scratch,
                                         d_status + first, (void*)s)
                   : zcg_read_regions_v(ctx, &P.r, lo, n, (const void* const*)d_table, bx, count, d_scratch,
                                        d_status + first, (void*)s);
    }
    const zcg_box* bx = (const zcg_box*)d_recs + first;
    return dir ? zcg_write_regions(ctx, &P.r, lo, n, (void* const*)d_table, bx, count, d_status + first, (void*)s)
               : zcg_read_regions(ctx, &P.r, lo, n, (const void* const*)d_table, bx, count, d_status + first,
                                  (void*)s);
}

// The per-group loop of every store-level call (the header comment has the
// contract).  Payload X, per group G and in this order:
//   X.device_bytes(G)                 bytes of its part of the group's device block
//   X.upload(G, d_part, stream)       its records and a host caller's values, enqueued
//   X.launch(ctx, G, lo, n, d_table, stream)
//                                     its kernels, then its status and a host caller's
//                                     results on their way back, enqueued
//   X.finish(ctx, G)                  after the synchronisation: its status check and
//                                     host copy-back
// Host memory that X hands to an enqueued copy must live as long as X does.
template <class Payload>
int run_groups(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root, const char* path,
               const Plan& P, bool write, uint32_t io_threads, Payload& X) {
    const uint32_t threads = io_threads ? io_threads : 1;
    const uint64_t fillv = meta->has_fill_value ? meta->fill_value : 0;
    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, what + " stream");

    for (size_t g = 0; g < P.groups.size(); g++) {
        const Group& G = P.groups[g];
        const uint32_t m = (uint32_t)G.keys.size();
        if (write && m == 0) continue;  // no item of the group visits a chunk: nothing to write
        const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = P.gentries[g];
        GroupSlots S;
        DevMem block;

        // 1. the chunks that are read first: all of them (read), or those a write leaves partly as
        // they were.  Read: an absent chunk is a NULL entry (read_chunk -> Ok(None)); write: every
        // chunk has a slot, and an absent one starts as fill value (ndarray.rs:351-364)
        std::vector<void*> table(std::max<uint64_t>(entries, 1), nullptr), absent;
        if (m) {
            int rc = group_slots(ctx, what, meta, root, path, P, g, S);
            if (rc != ZCG_OK) return rc;
            std::vector<uint32_t> idx;
            std::vector<const char*> rpaths;
            std::vector<void*> rptrs;
            for (uint32_t i = 0; i < m; i++) {
                table[S.tidx[i]] = S.ptrs[i];
                if (write && !G.read_first[i]) continue;
                idx.push_back(i);
                rpaths.push_back(S.cpaths[i]);
                rptrs.push_back(S.ptrs[i]);
            }
            std::vector<int32_t> status(idx.size(), ZCG_OK);
            if (!idx.empty()) {
                rc = zcg_store_read_chunks_device(ctx, &meta->array, (uint32_t)idx.size(), rpaths.data(), rptrs.data(),
                                                  status.data(), threads);
                if (rc != ZCG_OK) return rc;
            }
            for (size_t k = 0; k < idx.size(); k++) {
                if (status[k] == ZCG_ABSENT) {
                    if (write) absent.push_back(rptrs[k]);
                    else table[S.tidx[idx[k]]] = nullptr;
                } else if (status[k] != ZCG_OK) {
                    return chunk_failed(ctx, what, P, G.keys[idx[k]], status[k]);
                }
            }
        }

        // 2. device: [table entries][absent slots][the payload's part]
        const size_t o_abs = up256(entries * sizeof(void*));
        const size_t o_pay = up256(o_abs + absent.size() * sizeof(void*));
        if ((e = block.alloc(o_pay + X.device_bytes(G))) != hipSuccess) return fail_hip(ctx, e, what + " table");
        uint8_t* db = (uint8_t*)block.p;
        if (entries) e = hipMemcpyAsync(db, table.data(), entries * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess && !absent.empty())
            e = hipMemcpyAsync(db + o_abs, absent.data(), absent.size() * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess) e = X.upload(G, db + o_pay, st.s);
        if (e == hipSuccess && write)
            e = launch_slot_fill((void* const*)(db + o_abs), (uint32_t)absent.size(), P.D, P.es, fillv, st.s);

        // 3. the payload's launches, and the group's one synchronisation: whatever went wrong after
        // a copy was enqueued, the host vectors of this scope and of X outlive the copy
        int rc = e != hipSuccess ? fail_hip(ctx, e, what + " H2D") : X.launch(ctx, G, lo, n, db, st.s);
        e = hipStreamSynchronize(st.s);
        if (rc == ZCG_OK && e != hipSuccess) rc = fail_hip(ctx, e, what + (write ? " scatter" : " assembly"));
        if (rc == ZCG_OK) rc = X.finish(ctx, G);
        if (rc != ZCG_OK) return rc;
        if (!write) continue;

        // 4. write: encode and write every chunk of the group, once
        std::vector<int32_t> wst(m, ZCG_OK);
        rc = zcg_store_write_chunks_device(ctx, &meta->array, m, S.cpaths.data(), (const void* const*)S.ptrs.data(),
                                           wst.data(), threads);
        if (rc != ZCG_OK) return rc;
        for (uint32_t i = 0; i < m; i++)
            if (wst[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], wst[i]);
    }
    return ZCG_OK;
}

// The boxes of a group (the header comment has the device layout).  bufs[b]:
// box b's host buffer, dense in the chunk memory order (host), or the base of
// its device view; a read writes through it.
struct BoxPayload {
    const Plan& P;
    const std::string& what;
    const uint64_t* offsets;
    void* const* bufs;
    bool host, write;
    DevMem staging;  // host: the group's boxes back to back
    std::vector<uint8_t> recs, bounce;
    bool copy_back = false;  // a read went through `bounce`: finish() hands the boxes out
    std::vector<int32_t> bst;
    std::vector<uint32_t> wave_of;
    uint8_t* d = nullptr;  // the group's records; status and scratch follow
    size_t o_st = 0, o_scr = 0;

    uint64_t group_bytes(const Group& G) const { return P.at[G.b1] - P.at[G.b0]; }
    uint8_t* bounce_at(const Group& G, uint32_t b) { return bounce.data() + (P.at[b] - P.at[G.b0]); }
    // are the group's host buffers consecutive in memory?  Then one copy serves them as they are
    bool consecutive(const Group& G) const {
        for (uint32_t b = G.b0 + 1; b < G.b1; b++)
            if ((uint8_t*)bufs[b] != (uint8_t*)bufs[G.b0] + (P.at[b] - P.at[G.b0])) return false;
        return true;
    }

    size_t device_bytes(const Group& G) {
        const uint32_t nb = G.b1 - G.b0;
        o_st = up256((size_t)nb * record_bytes(P));
        o_scr = up256(o_st + (size_t)nb * sizeof(int32_t));
        return o_scr + (P.varied ? zcg_regions_v_scratch_bytes(nb) : 0);
    }

    hipError_t upload(const Group& G, uint8_t* d_part, hipStream_t s) {
        d = d_part;
        hipError_t e = host ? staging.alloc(group_bytes(G)) : hipSuccess;
        if (e != hipSuccess) return e;
        recs = box_records(P, offsets, bufs, staging.p, G.b0, G.b1 - G.b0, host);
        e = hipMemcpyAsync(d, recs.data(), recs.size(), hipMemcpyHostToDevice, s);
        if (e != hipSuccess || !host || !write || !group_bytes(G)) return e;
        const uint8_t* src = (const uint8_t*)bufs[G.b0];
        if (!consecutive(G)) {
            bounce.resize(group_bytes(G));
            for (uint32_t b = G.b0; b < G.b1; b++)
                if (P.box_bytes(b)) memcpy(bounce_at(G, b), bufs[b], P.box_bytes(b));
            src = bounce.data();
        }
        return hipMemcpyAsync(staging.p, src, group_bytes(G), hipMemcpyHostToDevice, s);
    }

    int launch(zcg_ctx* ctx, const Group& G, const uint64_t* lo, const uint64_t* n, void* d_table, hipStream_t s) {
        const uint32_t nb = G.b1 - G.b0, nd = P.nd;
        int32_t* d_st = (int32_t*)(d + o_st);
        if (!write) {
            const int rc = regions_launch(ctx, P, lo, n, d_table, d, 0, nb, d + o_scr, d_st, s, 0);
            if (rc != ZCG_OK) return rc;
        } else {
            // wave by wave: a later box wins what it shares with an earlier one
            const uint64_t* off = offsets + (size_t)G.b0 * nd;
            wave_of.resize(nb);
            if (P.steps)
                zcg_regions_s_waves(&P.r, off, P.shapes + (size_t)G.b0 * nd, P.steps + (size_t)G.b0 * nd, nb,
                                    wave_of.data());
            else if (P.varied)
                zcg_regions_v_waves(&P.r, off, P.shapes + (size_t)G.b0 * nd, nb, wave_of.data());
            else
                zcg_regions_waves(&P.r, off, nb, wave_of.data());
            for (uint32_t b0 = 0; b0 < nb;) {
                uint32_t b1 = b0 + 1;
                while (b1 < nb && wave_of[b1] == wave_of[b0]) b1++;
                const int rc = regions_launch(ctx, P, lo, n, d_table, d, b0, b1 - b0, d + o_scr, d_st, s, 1);
                if (rc != ZCG_OK) return rc;
                b0 = b1;
            }
        }
        bst.assign(nb, ZCG_OK);
        hipError_t e = hipMemcpyAsync(bst.data(), d_st, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        copy_back = false;
        if (e == hipSuccess && host && !write && group_bytes(G)) {
            uint8_t* dst = (uint8_t*)bufs[G.b0];
            if (!consecutive(G)) {
                bounce.resize(group_bytes(G));
                dst = bounce.data();
                copy_back = true;
            }
            e = hipMemcpyAsync(dst, staging.p, group_bytes(G), hipMemcpyDeviceToHost, s);
        }
        return e == hipSuccess ? ZCG_OK : fail_hip(ctx, e, what + (write ? " scatter" : " assembly"));
    }

    int finish(zcg_ctx* ctx, const Group& G) {
        staging.release();
        for (uint32_t b = G.b0; b < G.b1; b++)
            if (bst[b - G.b0] != ZCG_OK) {
                ctx_set_error(ctx, what + ": box " + std::to_string(b) + ": status " + std::to_string(bst[b - G.b0]));
                return bst[b - G.b0];
            }
        if (copy_back)  // a read whose buffers are not consecutive
            for (uint32_t b = G.b0; b < G.b1; b++)
                if (P.box_bytes(b)) memcpy(bufs[b], bounce_at(G, b), P.box_bytes(b));
        return ZCG_OK;
    }
};

// write == false: read_ndarray for every box; host == true: bufs are host
// buffers, each box dense in the chunk memory order with fill, else device
// views with the caller's strides.  write == true: write_ndarray for the boxes
// in order (ndarray.rs:276-385).  varied, box_steps: plan_boxes'.
int run_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
              const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* strides, bool varied,
              uint32_t fill_missing, const uint64_t* offsets, void* const* bufs, uint32_t n_boxes,
              uint64_t slot_budget_bytes, uint32_t io_threads, bool host, bool write) {
    const std::string what = write ? "write_boxes" : "read_boxes";
    Plan P;
    // before any file is read or written
    const int prc = plan_boxes(ctx, what, meta, root, path, box_shape, box_steps, strides, varied, fill_missing,
                               offsets, bufs, n_boxes, slot_budget_bytes, host, write, P);
    if (prc != ZCG_OK) return prc;
    if (P.nothing || P.at[n_boxes] == 0) return ZCG_OK;
    BoxPayload X{P, what, offsets, bufs, host, write};
    return run_groups(ctx, what, meta, root, path, P, write, io_threads, X);
}

int read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
               const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* out_strides, bool varied,
               uint32_t fill_missing, const uint64_t* offsets, void* const* outs, uint32_t n_boxes,
               uint64_t slot_budget_bytes, uint32_t io_threads, bool host) {
    return run_boxes(ctx, meta, root, path, box_shape, box_steps, out_strides, varied, fill_missing, offsets, outs,
                     n_boxes, slot_budget_bytes, io_threads, host, false);
}

int write_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* in_strides, bool varied,
                const uint64_t* offsets, const void* const* ins, uint32_t n_boxes, uint64_t slot_budget_bytes,
                uint32_t io_threads, bool host) {
    return run_boxes(ctx, meta, root, path, box_shape, box_steps, in_strides, varied, 0, offsets, (void* const*)ins,
                     n_boxes, slot_budget_bytes, io_threads, host, true);
}

}  // namespace

extern "C" int zcg_store_write_boxes_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                            const char* path, const uint64_t* box_shape, const int64_t* in_strides,
                                            const uint64_t* offsets, const void* const* d_ins, uint32_t n_boxes,
                                            uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_boxes(ctx, meta, root, path, box_shape, nullptr, in_strides, false, offsets, d_ins, n_boxes,
                       slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_write_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                     const uint64_t* box_shape, const uint64_t* offsets, const void* const* ins,
                                     uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_boxes(ctx, meta, root, path, box_shape, nullptr, nullptr, false, offsets, ins, n_boxes, slot_budget_bytes,
                       io_threads, true);
}

extern "C" int zcg_store_read_boxes_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                           const char* path, const uint64_t* box_shape, const int64_t* out_strides,
                                           uint32_t fill_missing, const uint64_t* offsets, void* const* d_outs,
                                           uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shape, nullptr, out_strides, false, fill_missing, offsets, d_outs, n_boxes,
                      slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                    const uint64_t* box_shape, const uint64_t* offsets, void* const* outs,
                                    uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shape, nullptr, nullptr, false, 1, offsets, outs, n_boxes, slot_budget_bytes,
                      io_threads, true);
}

extern "C" int zcg_store_read_boxes_v_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                             const char* path, const uint64_t* box_shapes,
                                             const int64_t* out_strides, uint32_t fill_missing,
                                             const uint64_t* offsets, void* const* d_outs, uint32_t n_boxes,
                                             uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shapes, nullptr, out_strides, true, fill_missing, offsets, d_outs, n_boxes,
                      slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_read_boxes_v(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                      const uint64_t* box_shapes, const uint64_t* offsets, void* const* outs,
                                      uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shapes, nullptr, nullptr, true, 1, offsets, outs, n_boxes, slot_budget_bytes,
                      io_threads, true);
}

extern "C" int zcg_store_write_boxes_v_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                              const char* path, const uint64_t* box_shapes,
                                              const int64_t* in_strides, const uint64_t* offsets,
                                              const void* const* d_ins, uint32_t n_boxes,
                                              uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_boxes(ctx, meta, root, path, box_shapes, nullptr, in_strides, true, offsets, d_ins, n_boxes,
                       slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_write_boxes_v(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                       const uint64_t* box_shapes, const uint64_t* offsets, const void* const* ins,
                                       uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_boxes(ctx, meta, root, path, box_shapes, nullptr, nullptr, true, offsets, ins, n_boxes, slot_budget_bytes,
                       io_threads, true);
}

// Every step is 1 and no box is empty: the strided call is then the _v call,
// chunk for chunk and error for error, and takes its kernels (the dense walk
// of zcg_region_v.hip is the faster one at step 1: profiles/boxes_s_bench.json).
// An empty box keeps the strided plan, which unlike the _v plan never checks a
// chunk that holds no sample.
static bool all_dense(const zcg_array_meta* meta, const uint64_t* box_shapes, const uint64_t* box_steps,
                      uint32_t n_boxes) {
    if (!meta || !box_shapes || !box_steps || meta->ndim < 1 || meta->ndim > ZCG_MAX_DIMS) return false;
    for (size_t i = 0; i < (size_t)n_boxes * meta->ndim; i++)
        if (box_steps[i] != 1 || box_shapes[i] == 0) return false;
    return n_boxes != 0;
}

extern "C" int zcg_store_read_boxes_s_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                             const char* path, const uint64_t* box_shapes, const uint64_t* box_steps,
                                             const int64_t* out_strides, uint32_t fill_missing,
                                             const uint64_t* offsets, void* const* d_outs, uint32_t n_boxes,
                                             uint64_t slot_budget_bytes, uint32_t io_threads) {
    if (!box_steps && n_boxes) return ZCG_ERR_INVALID_INPUT;
    if (all_dense(meta, box_shapes, box_steps, n_boxes)) box_steps = nullptr;
    return read_boxes(ctx, meta, root, path, box_shapes, box_steps, out_strides, true, fill_missing, offsets, d_outs,
                      n_boxes, slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_read_boxes_s(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                      const uint64_t* box_shapes, const uint64_t* box_steps, const uint64_t* offsets,
                                      void* const* outs, uint32_t n_boxes, uint64_t slot_budget_bytes,
                                      uint32_t io_threads) {
    if (!box_steps && n_boxes) return ZCG_ERR_INVALID_INPUT;
    if (all_dense(meta, box_shapes, box_steps, n_boxes)) box_steps = nullptr;
    return read_boxes(ctx, meta, root, path, box_shapes, box_steps, nullptr, true, 1, offsets, outs, n_boxes,
                      slot_budget_bytes, io_threads, true);
}

// What the strided write calls refuse from their arguments alone, by
// plan_boxes' own checks but without needing a context: a caller (or a test)
// learns of them on a machine without a GPU.  ZCG_OK: go on.
static int strided_write_args(zcg_ctx* ctx, const zcg_array_meta* meta, const uint64_t* box_shapes,
                              const uint64_t* box_steps, uint32_t n_boxes) {
    const std::string what = "write_boxes";
    auto say = [&](const std::string& e) { if (ctx) ctx_set_error(ctx, e); };
    if (!meta || (n_boxes && (!box_shapes || !box_steps))) return ZCG_ERR_INVALID_INPUT;
    int rc = meta_args_status(what, meta, say);
    const uint32_t nd = meta->ndim;
    for (uint32_t b = 0; rc == ZCG_OK && b < n_boxes; b++)
        rc = sbox_args_status(what, b, nd, box_shapes + (size_t)b * nd, box_steps + (size_t)b * nd, meta->chunk_shape, say);
    return rc;
}

extern "C" int zcg_store_write_boxes_s_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                              const char* path, const uint64_t* box_shapes, const uint64_t* box_steps,
                                              const int64_t* in_strides, const uint64_t* offsets,
                                              const void* const* d_ins, uint32_t n_boxes,
                                              uint64_t slot_budget_bytes, uint32_t io_threads) {
    const int arc = strided_write_args(ctx, meta, box_shapes, box_steps, n_boxes);
    if (arc != ZCG_OK) return arc;
    if (all_dense(meta, box_shapes, box_steps, n_boxes)) box_steps = nullptr;
    return write_boxes(ctx, meta, root, path, box_shapes, box_steps, in_strides, true, offsets, d_ins, n_boxes,
                       slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_write_boxes_s(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                       const uint64_t* box_shapes, const uint64_t* box_steps, const uint64_t* offsets,
                                       const void* const* ins, uint32_t n_boxes, uint64_t slot_budget_bytes,
                                       uint32_t io_threads) {
    const int arc = strided_write_args(ctx, meta, box_shapes, box_steps, n_boxes);
    if (arc != ZCG_OK) return arc;
    if (all_dense(meta, box_shapes, box_steps, n_boxes)) box_steps = nullptr;
    return write_boxes(ctx, meta, root, path, box_shapes, box_steps, nullptr, true, offsets, ins, n_boxes,
                       slot_budget_bytes, io_threads, true);
}

// ---- a list of coordinates --------------------------------------------------
// zcg_store_read_points / zcg_store_write_points: read_ndarray / write_ndarray
// (ndarray.rs:153-385) for the 1-element boxes at the coordinates, without the
// boxes.  The points are sorted by chunk, then by their place in the chunk:
// the sort yields the unique chunks and the groups (consecutive runs of sorted
// points whose chunks fit the slot budget), and a wave's lanes fall into one
// chunk and neighbouring lines.  The kernel (zcg_region_p.hip) gets the sorted
// coordinates with each point's original index, so a device caller's values
// stay in the caller's order; host values are permuted on the host.
namespace zcg {
int points_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                const void* const* d_chunk_table, const uint64_t* d_coords, const uint64_t* d_order,
                uint64_t n_points, void* d_vals, uint64_t* d_first_outside, void* stream, uint32_t dir);
}

namespace {

struct SortedPoint {
    uint64_t key;  // linear chunk index over the array's grid; ~0: the point visits no chunk
    uint64_t at;   // element index inside the chunk, in the chunk memory order
    uint64_t i;    // index in the caller's list
};

// plan_boxes for points: the same argument checks and in-grid rule (a point is
// its 1-element box), then the sort and the groups.  Group::b0 .. b1 index
// `pts`.  keep (write): only points with keep[i] != 0 take part, and points
// that visit no chunk are dropped.
int plan_points(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root, const char* path,
                uint32_t fill_missing, const uint64_t* coords, const void* buf, uint64_t n_points,
                const uint8_t* keep, uint64_t slot_budget_bytes, Plan& P, std::vector<SortedPoint>& pts) {
    const int hrc = plan_head(ctx, what, meta, root, path, coords, buf, n_points, "points", fill_missing, P);
    if (hrc != ZCG_OK || P.nothing) return hrc;
    const uint32_t nd = P.nd;
    zcg_region& r = P.r;
    const int grc = plan_head_grid(ctx, what, slot_budget_bytes, P);
    if (grc != ZCG_OK) return grc;
    const uint64_t* extent = P.extent;
    uint64_t cstr[ZCG_MAX_DIMS], c = 1;  // element strides inside a chunk, in the chunk memory order
    for (uint32_t k = 0; k < nd; k++) {
        const uint32_t d = meta->chunk_order == 1 ? k : nd - 1 - k;
        r.bbox_shape[d] = 1;
        cstr[d] = c;
        c *= meta->chunk_shape[d];
    }
    const uint64_t max_chunks = std::max<uint64_t>(P.budget / std::max<uint64_t>(P.D, 1), 1);

    // every point's chunk: in bounds (the reference panics at storage.rs:217)
    pts.clear();
    pts.reserve(n_points);
    zcg_region rb = r;
    for (uint64_t i = 0; i < n_points; i++) {
        if (keep && !keep[i]) continue;
        uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS];
        for (uint32_t d = 0; d < nd; d++) rb.bbox_offset[d] = coords[i * nd + d];
        SortedPoint sp{~0ull, 0, i};
        if (zcg_region_grid(&rb, lo, n)) {
            sp.key = 0;
            for (uint32_t d = 0; d < nd; d++) {
                if (lo[d] + n[d] - 1 >= extent[d]) {
                    for (uint32_t k = 0; k < nd; k++) lo[k] += n[k] - 1;
                    ctx_set_error(ctx, what + ": point " + std::to_string(i) + " visits chunk " + pos_text(lo, nd) +
                                           " outside the array's chunk grid");
                    return ZCG_ERR_INVALID_INPUT;
                }
                sp.key += lo[d] * P.gstr[d];
                sp.at += (rb.bbox_offset[d] - lo[d] * r.chunk_shape[d]) * cstr[d];
            }
        } else if (keep) {
            continue;  // write: no chunk, no element
        }
        pts.push_back(sp);
    }
    std::sort(pts.begin(), pts.end(), [](const SortedPoint& a, const SortedPoint& b) {
        return a.key != b.key ? a.key < b.key : a.at != b.at ? a.at < b.at : a.i < b.i;
    });

    // groups: runs of sorted points whose unique chunks fit the budget; the points without a chunk end the last
    Group cur{0, 0, {}, {}};
    for (size_t s = 0; s < pts.size(); s++) {
        const uint64_t key = pts[s].key;
        if (key != ~0ull && (cur.keys.empty() || cur.keys.back() != key)) {
            if (cur.keys.size() >= max_chunks) {
                cur.b1 = (uint32_t)s;
                P.groups.push_back(std::move(cur));
                cur = Group{(uint32_t)s, (uint32_t)s, {}, {}};
            }
            cur.keys.push_back(key);
        }
    }
    cur.b1 = (uint32_t)pts.size();
    if (cur.b1 > cur.b0) P.groups.push_back(std::move(cur));
    // a group's table: the bounding grid range of its chunks
    const size_t ng = P.groups.size();
    P.glo.assign(ng * ZCG_MAX_DIMS, 0);
    P.gn.assign(ng * ZCG_MAX_DIMS, 0);
    P.gentries.assign(ng, 0);
    for (size_t g = 0; g < ng; g++) {
        Group& G = P.groups[g];
        // a one-element chunk is covered by its point; any other is read before the scatter
        G.read_first.assign(G.keys.size(), meta->array.chunk_num_elements != 1 ? 1 : 0);
        uint64_t hi[ZCG_MAX_DIMS] = {0}, pos[ZCG_MAX_DIMS];
        uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        for (size_t i = 0; i < G.keys.size(); i++) {
            P.key_pos(G.keys[i], pos);
            for (uint32_t d = 0; d < nd; d++) {
                lo[d] = i ? std::min(lo[d], pos[d]) : pos[d];
                hi[d] = i ? std::max(hi[d], pos[d] + 1) : pos[d] + 1;
            }
        }
        uint64_t entries = G.keys.empty() ? 0 : 1;
        for (uint32_t d = 0; d < nd; d++) {
            P.gn[g * ZCG_MAX_DIMS + d] = hi[d] - lo[d];
            entries = entries > BOXES_MAX_TABLE ? entries : entries * (hi[d] - lo[d]);
        }
        P.gentries[g] = entries;
        if (entries > BOXES_MAX_TABLE) {
            ctx_set_error(ctx, what + ": the points' chunk table (" + std::to_string(entries) +
                                   " entries) exceeds 2^24; split the points over several calls");
            return ZCG_ERR_UNSUPPORTED;
        }
    }
    return ZCG_OK;
}

// The sorted points of a group (the header comment has the device layout).
// vals: the caller's values in the caller's order, host or device; a read
// writes them.
struct PointsPayload {
    const Plan& P;
    const std::string& what;
    const std::vector<SortedPoint>& pts;
    const uint64_t* coords;
    void* vals;
    bool host, write;
    DevMem staging;  // host: the group's values in sorted order
    std::vector<uint64_t> recs;  // coordinates, then indices
    std::vector<uint8_t> bounce;
    uint64_t first_outside = ~0ull;
    uint8_t* d = nullptr;  // the group's coordinates; indices and the first-outside word follow
    size_t o_ord = 0, o_fo = 0;

    size_t device_bytes(const Group& G) {
        const size_t np = G.b1 - G.b0;
        o_ord = np * P.nd * sizeof(uint64_t);
        o_fo = o_ord + np * sizeof(uint64_t);
        return o_fo + sizeof(uint64_t);
    }

    hipError_t upload(const Group& G, uint8_t* d_part, hipStream_t s) {
        const uint32_t nd = P.nd, es = P.es;
        const size_t np = G.b1 - G.b0;
        d = d_part;
        hipError_t e = host ? staging.alloc(np * es) : hipSuccess;
        if (e != hipSuccess) return e;
        recs.resize(np * nd + np);
        for (size_t i = 0; i < np; i++) {
            const SortedPoint& sp = pts[G.b0 + i];
            memcpy(&recs[i * nd], coords + sp.i * nd, nd * sizeof(uint64_t));
            recs[np * nd + i] = sp.i;
        }
        e = hipMemcpyAsync(d, recs.data(), recs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        if (e != hipSuccess || !host || !write) return e;
        bounce.resize(np * es);
        for (size_t i = 0; i < np; i++)
            memcpy(bounce.data() + i * es, (const uint8_t*)vals + pts[G.b0 + i].i * es, es);
        return hipMemcpyAsync(staging.p, bounce.data(), np * es, hipMemcpyHostToDevice, s);
    }

    // one launch: no two points of a write share an element (zcg_points_last).  host: the group's
    // values in sorted order, permuted on the host; device: straight from or to the caller's order
    int launch(zcg_ctx* ctx, const Group& G, const uint64_t* lo, const uint64_t* n, void* d_table, hipStream_t s) {
        const size_t np = G.b1 - G.b0;
        const int rc = points_call(ctx, &P.r, lo, n, (const void* const*)d_table, (const uint64_t*)d,
                                   host ? nullptr : (const uint64_t*)(d + o_ord), np, host ? staging.p : vals,
                                   (uint64_t*)(d + o_fo), (void*)s, write ? 1 : 0);
        if (rc != ZCG_OK) return rc;
        first_outside = ~0ull;
        hipError_t e = hipMemcpyAsync(&first_outside, d + o_fo, sizeof first_outside, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && host && !write) {
            bounce.resize(np * P.es);
            e = hipMemcpyAsync(bounce.data(), staging.p, np * P.es, hipMemcpyDeviceToHost, s);
        }
        return e == hipSuccess ? ZCG_OK : fail_hip(ctx, e, what + (write ? " scatter" : " assembly"));
    }

    int finish(zcg_ctx* ctx, const Group& G) {
        staging.release();
        if (first_outside != ~0ull) {
            ctx_set_error(ctx, what + ": sorted point " + std::to_string(first_outside) +
                                   " fell outside its group's table");
            return ZCG_ERR_RUNTIME;
        }
        if (host && !write)
            for (size_t i = 0; i < (size_t)(G.b1 - G.b0); i++)
                memcpy((uint8_t*)vals + pts[G.b0 + i].i * P.es, bounce.data() + i * P.es, P.es);
        return ZCG_OK;
    }
};

// read_ndarray (write == false) or write_ndarray (true) for the 1-element boxes
// of point 0, 1, ... in order.  Of two points of a write with one coordinate
// the later one counts (zcg_points_last), so the kernel never sees two values
// for one element.
int run_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path, const uint64_t* coords,
               uint64_t n_points, uint32_t fill_missing, void* vals, uint64_t slot_budget_bytes, uint32_t io_threads,
               bool host, bool write) {
    const std::string what = write ? "write_points" : "read_points";
    Plan P;
    std::vector<SortedPoint> pts;
    std::vector<uint8_t> keep;
    if (write) {
        keep.assign(n_points, 1);
        if (coords && meta && meta->ndim >= 1 && meta->ndim <= ZCG_MAX_DIMS)
            zcg_points_last(coords, n_points, meta->ndim, keep.data());
    }
    // before any file is read or written
    const int prc = plan_points(ctx, what, meta, root, path, !write && (host || fill_missing), coords, vals, n_points,
                                write ? keep.data() : nullptr, slot_budget_bytes, P, pts);
    if (prc != ZCG_OK) return prc;
    if (P.nothing) return ZCG_OK;
    PointsPayload X{P, what, pts, coords, vals, host, write};
    return run_groups(ctx, what, meta, root, path, P, write, io_threads, X);
}

}  // namespace

extern "C" int zcg_store_read_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                            const char* path, const uint64_t* coords, uint64_t n_points,
                                            uint32_t fill_missing, void* d_out, uint64_t slot_budget_bytes,
                                            uint32_t io_threads) {
    return run_points(ctx, meta, root, path, coords, n_points, fill_missing, d_out, slot_budget_bytes, io_threads,
                      false, false);
}

extern "C" int zcg_store_read_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                     const uint64_t* coords, uint64_t n_points, void* out,
                                     uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_points(ctx, meta, root, path, coords, n_points, 1, out, slot_budget_bytes, io_threads, true, false);
}

extern "C" int zcg_store_write_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                             const char* path, const uint64_t* coords, uint64_t n_points,
                                             const void* d_in, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_points(ctx, meta, root, path, coords, n_points, 0, (void*)d_in, slot_budget_bytes, io_threads, false,
                      true);
}

extern "C" int zcg_store_write_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                      const uint64_t* coords, uint64_t n_points, const void* in,
                                      uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_points(ctx, meta, root, path, coords, n_points, 0, (void*)in, slot_budget_bytes, io_threads, true, true);
}

// ---- an index list per dimension --------------------------------------------
// zcg_store_read_ortho / zcg_store_write_ortho: the point calls on the
// Cartesian product of the lists, without the product.  Every list is sorted by
// chunk index, index and position (the sum of the lists, never the product);
// a CELL is the run of a sorted list that falls into one grid index, and the
// touched chunks are the product of the per-dimension cells.  A group is a
// sub-product of runs of cells, so a chunk belongs to one group and is decoded
// once in the whole call.  The kernels (zcg_region_o.hip) get a group's runs of
// the sorted lists with each entry's original position, and address the
// caller's values, dense in C order over the positions, through them.
namespace zcg {
int ortho_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
               const void* const* d_chunk_table, const zcg_osel* sel, const uint64_t* const* d_pos, void* d_scratch,
               uint64_t* d_outside, void* stream, uint32_t dir);
}

namespace {

struct AxisEntry {
    uint64_t q;  // grid index along the dimension; ~0: the index visits no chunk
    uint64_t c;  // array index
    uint64_t i;  // position in the caller's list
};
struct AxisCell {
    uint64_t q;       // AxisEntry::q of the run
    uint32_t e0, e1;  // the run in the sorted list
    bool whole;       // write: every index of the chunk's nominal extent along the dimension is in the run
};
struct OrthoAxis {
    std::vector<AxisEntry> ent;   // sorted by (q, c, i); the entries without a chunk last
    std::vector<AxisCell> cells;  // ascending q
};
struct OrthoRange {
    uint32_t c0[ZCG_MAX_DIMS], c1[ZCG_MAX_DIMS];  // per dimension: cells c0 .. c1
};

// plan_points for an index list per dimension.  Group::b0 indexes `ranges`.
// write: per list the last occurrence of an index stays, and indices that
// visit no chunk are dropped.
int plan_ortho(zcg_ctx* ctx, const std::string& what, const zcg_array_meta* meta, const char* root, const char* path,
               uint32_t fill_missing, const uint64_t* const* lists, const uint64_t* count, const void* buf, bool write,
               uint64_t slot_budget_bytes, Plan& P, OrthoAxis* axes, std::vector<OrthoRange>& ranges) {
    if (!count) return ZCG_ERR_INVALID_INPUT;
    uint64_t some = 1;
    for (uint32_t d = 0; meta && d < meta->ndim && d < ZCG_MAX_DIMS; d++)
        if (count[d] == 0) some = 0;
    const int hrc = plan_head(ctx, what, meta, root, path, lists, buf, some, "selections", fill_missing, P);
    if (hrc != ZCG_OK || P.nothing) return hrc;
    const uint32_t nd = P.nd;
    uint64_t total = 1;
    for (uint32_t d = 0; d < nd; d++) {
        if (!lists[d]) return ZCG_ERR_INVALID_INPUT;
        if (count[d] >= (1ull << 32)) {
            ctx_set_error(ctx, what + ": a list must hold fewer than 2^32 indices");
            return ZCG_ERR_UNSUPPORTED;
        }
        total = total >= (1ull << 60) / count[d] + 1 ? 1ull << 60 : total * count[d];
    }
    if (total >= (1ull << 60) / P.es) {
        ctx_set_error(ctx, what + ": the selection holds 2^60 bytes or more");
        return ZCG_ERR_UNSUPPORTED;
    }
    const int grc = plan_head_grid(ctx, what, slot_budget_bytes, P);
    if (grc != ZCG_OK) return grc;
    const zcg_region& r = P.r;

    // every list: in-grid check (the reference panics at storage.rs:217), sort, cells
    for (uint32_t d = 0; d < nd; d++) {
        std::vector<AxisEntry>& ent = axes[d].ent;
        const uint64_t cs = r.chunk_shape[d];
        ent.reserve(count[d]);
        for (uint64_t i = 0; i < count[d]; i++) {
            const uint64_t c = lists[d][i];
            const bool visits = c < r.array_shape[d] || c % cs;
            if (visits && c / cs >= P.extent[d]) {
                ctx_set_error(ctx, what + ": dimension " + std::to_string(d) + ", position " + std::to_string(i) +
                                       ": index " + std::to_string(c) + " visits chunk " + std::to_string(c / cs) +
                                       " outside the array's chunk grid");
                return ZCG_ERR_INVALID_INPUT;
            }
            if (visits || !write) ent.push_back(AxisEntry{visits ? c / cs : ~0ull, c, i});
        }
    }
    for (uint32_t d = 0; d < nd; d++) {
        std::vector<AxisEntry>& ent = axes[d].ent;
        std::sort(ent.begin(), ent.end(), [](const AxisEntry& a, const AxisEntry& b) {
            return a.q != b.q ? a.q < b.q : a.c != b.c ? a.c < b.c : a.i < b.i;
        });
        if (write) {  // of the entries with one index the last position stays
            size_t k = 0;
            for (size_t s = 0; s < ent.size(); s++)
                if (s + 1 == ent.size() || ent[s + 1].c != ent[s].c) ent[k++] = ent[s];
            ent.resize(k);
        }
        if (ent.empty()) {  // write: no index of the list visits a chunk
            P.nothing = true;
            return ZCG_OK;
        }
        std::vector<AxisCell>& cells = axes[d].cells;
        for (size_t s = 0; s < ent.size(); s++) {
            if (cells.empty() || cells.back().q != ent[s].q) cells.push_back(AxisCell{ent[s].q, (uint32_t)s, 0, false});
            cells.back().e1 = (uint32_t)s + 1;
        }
        // without duplicates, a run as long as the chunk extent holds every index of the chunk
        for (AxisCell& c : cells) c.whole = write && c.e1 - c.e0 == r.chunk_shape[d];
    }

    // groups: the longest suffix of dimensions whose cells fit the budget is taken whole, the dimension
    // before it in runs of cells that fit, the dimensions before that one cell at a time.  A read's last
    // cell of entries without a chunk counts as a cell like the others: a group may then hold one
    // chunk fewer than the budget allows, never more
    const uint64_t max_chunks = std::max<uint64_t>(P.budget / std::max<uint64_t>(P.D, 1), 1);
    uint64_t ncell[ZCG_MAX_DIMS], steps[ZCG_MAX_DIMS], suffix = 1, run = 1;
    for (uint32_t d = 0; d < nd; d++) ncell[d] = axes[d].cells.size();
    uint32_t j = nd;  // dimensions j .. nd-1 are whole
    while (j > 0 && ncell[j - 1] <= max_chunks / suffix) suffix *= ncell[--j];
    uint64_t ngroups = 1;
    for (uint32_t d = 0; d < nd; d++) {
        if (d + 1 == j) run = std::max<uint64_t>(max_chunks / suffix, 1);
        steps[d] = d >= j ? 1 : d + 1 == j ? (ncell[d] + run - 1) / run : ncell[d];
        ngroups = ngroups > (1ull << 32) / steps[d] ? 1ull << 32 : ngroups * steps[d];
    }
    if (ngroups >= (1ull << 32)) {
        ctx_set_error(ctx, what + ": more than 2^32 groups of chunks; raise slot_budget_bytes or split the selection");
        return ZCG_ERR_UNSUPPORTED;
    }
    ranges.resize(ngroups);
    P.groups.resize(ngroups);
    P.glo.assign(ngroups * ZCG_MAX_DIMS, 0);
    P.gn.assign(ngroups * ZCG_MAX_DIMS, 0);
    P.gentries.assign(ngroups, 0);
    for (uint64_t g = 0; g < ngroups; g++) {
        OrthoRange& R = ranges[g];
        Group& G = P.groups[g];
        G.b0 = (uint32_t)g;
        G.b1 = (uint32_t)g + 1;
        uint64_t rem = g, real0[ZCG_MAX_DIMS], real1[ZCG_MAX_DIMS], chunks = 1, entries = 1;
        for (int d = (int)nd - 1; d >= 0; d--) {
            const uint64_t s = rem % steps[d];
            rem /= steps[d];
            R.c0[d] = (uint32_t)((uint32_t)d >= j ? 0 : (uint32_t)d + 1 == j ? s * run : s);
            R.c1[d] = (uint32_t)((uint32_t)d >= j ? ncell[d] : (uint32_t)d + 1 == j ? std::min(ncell[d], s * run + run) : s + 1);
            // the cells with a chunk: all but a last one of entries that visit none
            real0[d] = R.c0[d];
            real1[d] = R.c1[d] - (axes[d].cells[R.c1[d] - 1].q == ~0ull ? 1 : 0);
            chunks *= real1[d] - real0[d];
        }
        // the group's table: the bounding grid range of its chunks.  A read's run of entries without
        // a chunk leaves the group without chunks and the table without entries, but the other
        // dimensions keep their range: their entries are inside it
        for (uint32_t d = 0; d < nd; d++) {
            const bool real = real1[d] > real0[d];
            const uint64_t lo = real ? axes[d].cells[real0[d]].q : 0;
            const uint64_t n = real ? axes[d].cells[real1[d] - 1].q - lo + 1 : 0;
            P.glo[g * ZCG_MAX_DIMS + d] = lo;
            P.gn[g * ZCG_MAX_DIMS + d] = n;
            entries = entries > BOXES_MAX_TABLE ? entries : entries * n;
        }
        P.gentries[g] = entries;
        if (entries > BOXES_MAX_TABLE) {
            ctx_set_error(ctx, what + ": a group's chunk table (" + std::to_string(entries) +
                                   " entries) exceeds 2^24; split the selection over several calls");
            return ZCG_ERR_UNSUPPORTED;
        }
        if (chunks == 0) continue;  // fill only
        G.keys.reserve(chunks);
        uint64_t at[ZCG_MAX_DIMS];
        for (uint32_t d = 0; d < nd; d++) at[d] = real0[d];
        for (uint64_t k = 0; k < chunks; k++) {  // dimension 0 slowest: ascending keys
            uint64_t key = 0;
            bool whole = true;
            for (uint32_t d = 0; d < nd; d++) {
                key += axes[d].cells[at[d]].q * P.gstr[d];
                whole &= axes[d].cells[at[d]].whole;
            }
            G.keys.push_back(key);
            if (write) G.read_first.push_back(whole ? 0 : 1);
            for (int d = (int)nd - 1; d >= 0; d--) {
                if (++at[d] < real1[d]) break;
                at[d] = real0[d];
            }
        }
    }
    return ZCG_OK;
}

// A group's runs of the sorted lists: [indices, per dimension][positions, per
// dimension][scratch of the kernels][the outside words].  d_vals: the values,
// dense in C order over the caller's positions.
struct OrthoPayload {
    const Plan& P;
    const std::string& what;
    const OrthoAxis* axes;
    const std::vector<OrthoRange>& ranges;
    const uint64_t* count;
    void* d_vals;
    bool write;
    std::vector<uint64_t> recs;
    uint64_t len[ZCG_MAX_DIMS] = {0}, first[ZCG_MAX_DIMS] = {0}, sum = 0;
    uint64_t outside[ZCG_MAX_DIMS];
    uint8_t* d = nullptr;
    size_t o_scr = 0, o_out = 0;

    size_t device_bytes(const Group& G) {
        const OrthoRange& R = ranges[G.b0];
        sum = 0;
        for (uint32_t k = 0; k < P.nd; k++) {
            first[k] = axes[k].cells[R.c0[k]].e0;
            len[k] = axes[k].cells[R.c1[k] - 1].e1 - first[k];
            sum += len[k];
        }
        o_scr = up256(2 * sum * sizeof(uint64_t));
        o_out = o_scr + zcg_ortho_scratch_bytes(P.nd, len);
        return o_out + ZCG_MAX_DIMS * sizeof(uint64_t);
    }

    hipError_t upload(const Group&, uint8_t* d_part, hipStream_t s) {
        d = d_part;
        recs.resize(2 * sum);
        size_t at = 0;
        for (uint32_t k = 0; k < P.nd; k++)
            for (uint64_t i = 0; i < len[k]; i++, at++) {
                recs[at] = axes[k].ent[first[k] + i].c;
                recs[sum + at] = axes[k].ent[first[k] + i].i;
            }
        return hipMemcpyAsync(d, recs.data(), recs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    }

    int launch(zcg_ctx* ctx, const Group&, const uint64_t* lo, const uint64_t* n, void* d_table, hipStream_t s) {
        zcg_osel sel;
        memset(&sel, 0, sizeof sel);
        const uint64_t* pos[ZCG_MAX_DIMS] = {nullptr};
        const uint64_t* dl = (const uint64_t*)d;
        int64_t acc = 1;
        for (int k = (int)P.nd - 1; k >= 0; k--) {
            sel.strides[k] = acc;
            acc *= (int64_t)count[k];
        }
        for (uint32_t k = 0; k < P.nd; k++) {
            sel.index[k] = dl;
            pos[k] = dl + sum;
            sel.count[k] = len[k];
            dl += len[k];
        }
        sel.base = d_vals;
        const int rc = ortho_call(ctx, &P.r, lo, n, (const void* const*)d_table, &sel, pos, d + o_scr,
                                  (uint64_t*)(d + o_out), (void*)s, write ? 1 : 0);
        if (rc != ZCG_OK) return rc;
        for (uint32_t k = 0; k < ZCG_MAX_DIMS; k++) outside[k] = ~0ull;
        const hipError_t e = hipMemcpyAsync(outside, d + o_out, P.nd * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
        return e == hipSuccess ? ZCG_OK : fail_hip(ctx, e, what + (write ? " scatter" : " assembly"));
    }

    int finish(zcg_ctx* ctx, const Group&) {
        for (uint32_t k = 0; k < P.nd; k++)
            if (outside[k] != ~0ull) {
                ctx_set_error(ctx, what + ": dimension " + std::to_string(k) + ", sorted entry " +
                                       std::to_string(outside[k]) + " fell outside its group's table");
                return ZCG_ERR_RUNTIME;
            }
        return ZCG_OK;
    }
};

// read_points / write_points on the product of the lists in C order.  A host
// caller's values pass through one device array of the selection's size.
int run_ortho(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
              const uint64_t* const* lists, const uint64_t* count, uint32_t fill_missing, void* vals,
              uint64_t slot_budget_bytes, uint32_t io_threads, bool host, bool write) {
    const std::string what = write ? "write_ortho" : "read_ortho";
    Plan P;
    OrthoAxis axes[ZCG_MAX_DIMS];
    std::vector<OrthoRange> ranges;
    // before any file is read or written
    const int prc = plan_ortho(ctx, what, meta, root, path, !write && (host || fill_missing), lists, count, vals, write,
                               slot_budget_bytes, P, axes, ranges);
    if (prc != ZCG_OK) return prc;
    if (P.nothing) return ZCG_OK;
    uint64_t bytes = P.es;
    for (uint32_t d = 0; d < P.nd; d++) bytes *= count[d];
    DevMem stage;
    if (host) {
        (void)hipSetDevice(ctx_device(ctx));
        hipError_t e = stage.alloc(bytes);
        if (e == hipSuccess && write) e = hipMemcpy(stage.p, vals, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail_hip(ctx, e, what + " values");
    }
    OrthoPayload X{P, what, axes, ranges, count, host ? stage.p : vals, write};
    const int rc = run_groups(ctx, what, meta, root, path, P, write, io_threads, X);
    if (rc != ZCG_OK || !host || write) return rc;
    const hipError_t e = hipMemcpy(vals, stage.p, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? ZCG_OK : fail_hip(ctx, e, what + " values");
}

}  // namespace

extern "C" int zcg_store_read_ortho_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                           const char* path, const uint64_t* const* lists, const uint64_t* count,
                                           uint32_t fill_missing, void* d_out, uint64_t slot_budget_bytes,
                                           uint32_t io_threads) {
    return run_ortho(ctx, meta, root, path, lists, count, fill_missing, d_out, slot_budget_bytes, io_threads, false,
                     false);
}

extern "C" int zcg_store_read_ortho(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                    const uint64_t* const* lists, const uint64_t* count, void* out,
                                    uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_ortho(ctx, meta, root, path, lists, count, 1, out, slot_budget_bytes, io_threads, true, false);
}

extern "C" int zcg_store_write_ortho_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                            const char* path, const uint64_t* const* lists, const uint64_t* count,
                                            const void* d_in, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_ortho(ctx, meta, root, path, lists, count, 0, (void*)d_in, slot_budget_bytes, io_threads, false, true);
}

extern "C" int zcg_store_write_ortho(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                     const uint64_t* const* lists, const uint64_t* count, const void* in,
                                     uint64_t slot_budget_bytes, uint32_t io_threads) {
    return run_ortho(ctx, meta, root, path, lists, count, 0, (void*)in, slot_budget_bytes, io_threads, true, true);
}
