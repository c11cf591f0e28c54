// zcg_boxes.cpp — read_ndarray for many bounding boxes in one native call
// (ZarrNdarrayReader::read_ndarray, src/ndarray.rs:153-268, once per box in the
// reference): the chunks all boxes visit are read and decoded once
// (zcg_store_read_chunks_device), and every box is assembled from the shared
// chunk table by one zcg_read_regions launch.
//
// Boxes are taken in consecutive groups whose unique chunks fit a budget of
// decoded device slots; a chunk two groups share is decoded in each.
//
// write_ndarray for many boxes (ndarray.rs:276-385) is the same plan the other
// way round: per group the chunks under a partial first box are read (absent
// ones prefilled), the boxes are scattered in the waves of zcg_regions_waves
// (zcg_write_regions per wave, so a later box wins), and every chunk of the
// group is encoded and written once (zcg_store_write_chunks_device).
//
// The _v calls take a shape per box; they share the planner and the two
// drivers with the one-shape calls, which pass one shape for all boxes and
// keep the one-shape kernels (zcg_read_regions / zcg_write_regions); boxes of
// differing shapes go through zcg_read_regions_v / zcg_write_regions_v.
//
// The _s calls add a step per box and dimension: the planner then takes a
// box's chunks from zcg_region_s_chunks (the touched chunks, a product of
// per-dimension index sets) instead of the hull's whole grid range, and the
// boxes are assembled by zcg_read_regions_s or scattered by
// zcg_write_regions_s in the waves of zcg_regions_s_waves.  On the write side
// a touched chunk is read first unless its first box covers it sample by
// sample (step 1, or a chunk extent of 1, along every dimension).
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
    ~DevMem() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)); }
};
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

int fail_hip(zcg_ctx* ctx, hipError_t e, const char* what) {
    ctx_set_error(ctx, std::string(what) + ": " + hipGetErrorString(e));
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
    uint64_t gstr[ZCG_MAX_DIMS];        // linear chunk keys over the array's grid
    bool nothing = false;               // n_boxes == 0: the call is done
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
    if (!ctx || !meta || !root || !path || (!box_shape && !(varied && n_boxes == 0)) ||
        (!host && !strides && !varied))
        return ZCG_ERR_INVALID_INPUT;
    if (n_boxes && (!offsets || !bufs)) return ZCG_ERR_INVALID_INPUT;
    auto say = [&](const std::string& e) { ctx_set_error(ctx, e); };
    const int mrc = meta_args_status(what, meta, say);
    if (mrc != ZCG_OK) return mrc;
    const uint32_t nd = meta->ndim;
    const uint32_t es = meta->array.dtype.elem_size;
    if (es != 1 && es != 2 && es != 4 && es != 8) return ZCG_ERR_INVALID_INPUT;
    P.nd = nd;
    P.es = es;
    if (n_boxes == 0) {
        P.nothing = true;
        return ZCG_OK;
    }

    zcg_region& r = P.r;
    uint64_t* gstr = P.gstr;
    P.varied = varied;
    P.shapes = box_shape;
    P.sstep = varied ? nd : 0;
    P.strides = varied && !host ? strides : nullptr;
    P.steps = box_steps;
    memset(&r, 0, sizeof r);
    r.ndim = nd;
    r.elem_size = es;
    r.chunk_order = meta->chunk_order;
    r.fill_missing = host ? 1u : (fill_missing ? 1u : 0u);
    r.fill_value = meta->has_fill_value ? meta->fill_value : 0;
    uint64_t extent[ZCG_MAX_DIMS];
    for (uint32_t d = 0; d < nd; d++) {
        if (meta->chunk_shape[d] == 0) return ZCG_ERR_INVALID_INPUT;
        r.array_shape[d] = meta->shape[d];
        r.chunk_shape[d] = meta->chunk_shape[d];
        extent[d] = u64_ceil_div(meta->shape[d], meta->chunk_shape[d]);
    }
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
    {   // dense host layout in the chunk memory order; linear chunk keys over the grid
        int64_t acc = 1;
        uint64_t g = 1;
        for (uint32_t k = 0; k < nd; k++) {
            const uint32_t d = meta->chunk_order == 1 ? k : nd - 1 - k;
            r.out_strides[d] = varied ? 0 : host ? acc : strides[d];
            acc *= (int64_t)std::max<uint64_t>(r.bbox_shape[d], 1);
        }
        for (int d = (int)nd - 1; d >= 0; d--) {
            gstr[d] = g;
            if (extent[d] && g > (~0ull) / extent[d]) {
                ctx_set_error(ctx, what + ": the array's chunk grid exceeds 2^64 chunks");
                return ZCG_ERR_UNSUPPORTED;
            }
            g *= extent[d];
        }
    }
    const uint64_t D = P.D = meta->array.chunk_num_elements * (uint64_t)es;
    const uint64_t budget = slot_budget_bytes ? slot_budget_bytes : BOXES_DEFAULT_BUDGET;

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

// host == true: outs are host buffers, each box dense in the chunk memory
// order with fill (read_ndarray); else device views with the caller's strides.
// varied: plan_boxes' (a shape, and as a device view strides, per box).
int read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
               const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* out_strides, bool varied,
               uint32_t fill_missing,
               const uint64_t* offsets, void* const* outs, uint32_t n_boxes, uint64_t slot_budget_bytes,
               uint32_t io_threads, bool host) {
    const std::string what = "read_boxes";
    Plan P;
    // 1. before any file is read
    const int prc = plan_boxes(ctx, what, meta, root, path, box_shape, box_steps, out_strides, varied, fill_missing,
                               offsets, outs, n_boxes, slot_budget_bytes, host, false, P);
    if (prc != ZCG_OK) return prc;
    if (P.nothing || P.at[n_boxes] == 0) return ZCG_OK;

    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, "read_boxes stream");

    // 2. per group: read + decode its chunks once, build the table, one launch
    for (size_t g = 0; g < P.groups.size(); g++) {
        const Group& G = P.groups[g];
        const uint32_t nb = G.b1 - G.b0, m = (uint32_t)G.keys.size();
        const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = P.gentries[g];
        GroupSlots S;
        DevMem meta_dev, staging;
        std::vector<const void*> table(std::max<uint64_t>(entries, 1), nullptr);
        if (m) {
            int rc = group_slots(ctx, what, meta, root, path, P, g, S);
            if (rc != ZCG_OK) return rc;
            std::vector<int32_t> status(m, ZCG_OK);
            rc = zcg_store_read_chunks_device(ctx, &meta->array, m, S.cpaths.data(), S.ptrs.data(), status.data(),
                                              io_threads ? io_threads : 1);
            if (rc != ZCG_OK) return rc;
            for (uint32_t i = 0; i < m; i++) {
                if (status[i] == ZCG_ABSENT) continue;  // read_chunk -> Ok(None): a NULL entry
                if (status[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], status[i]);
                table[S.tidx[i]] = S.ptrs[i];
            }
        }
        // device: [table entries][boxes nb][status nb][scratch of the _v kernels]
        const uint64_t group_bytes = P.at[G.b1] - P.at[G.b0];
        const size_t o_box = (entries * sizeof(void*) + 255) & ~(size_t)255;
        const size_t o_st = (o_box + (size_t)nb * record_bytes(P) + 255) & ~(size_t)255;
        const size_t o_scr = (o_st + (size_t)nb * sizeof(int32_t) + 255) & ~(size_t)255;
        if ((e = meta_dev.alloc(o_scr + (P.varied ? zcg_regions_v_scratch_bytes(nb) : 0))) != hipSuccess)
            return fail_hip(ctx, e, "read_boxes table");
        if (host && (e = staging.alloc(group_bytes)) != hipSuccess)
            return fail_hip(ctx, e, "read_boxes staging");
        const std::vector<uint8_t> boxes = box_records(P, offsets, outs, staging.p, G.b0, nb, host);
        uint8_t* db = (uint8_t*)meta_dev.p;
        if (entries) e = hipMemcpyAsync(db, table.data(), entries * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(db + o_box, boxes.data(), boxes.size(), hipMemcpyHostToDevice, st.s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st.s);  // the host vectors of an enqueued copy end with this scope
            return fail_hip(ctx, e, "read_boxes H2D");
        }
        const int rc = regions_launch(ctx, P, lo, n, db, db + o_box, 0, nb, db + o_scr, (int32_t*)(db + o_st), st.s, 0);
        if (rc != ZCG_OK) {
            (void)hipStreamSynchronize(st.s);
            return rc;
        }
        std::vector<int32_t> bst(nb, ZCG_OK);
        e = hipMemcpyAsync(bst.data(), db + o_st, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st.s);
        std::vector<uint8_t> bounce;
        if (e == hipSuccess && host) {
            // one D2H per group: straight into the caller's boxes when they are
            // consecutive in memory, else through a bounce buffer
            bool dense = true;
            for (uint32_t i = 1; i < nb && dense; i++)
                dense = (uint8_t*)outs[G.b0 + i] == (uint8_t*)outs[G.b0] + (P.at[G.b0 + i] - P.at[G.b0]);
            uint8_t* dst = (uint8_t*)outs[G.b0];
            if (!dense) {
                bounce.resize(group_bytes);
                dst = bounce.data();
            }
            if (group_bytes) e = hipMemcpyAsync(dst, staging.p, group_bytes, hipMemcpyDeviceToHost, st.s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st.s);
        else (void)hipStreamSynchronize(st.s);
        if (e != hipSuccess) return fail_hip(ctx, e, "read_boxes assembly");
        for (uint32_t i = 0; i < nb; i++)
            if (bst[i] != ZCG_OK) {
                ctx_set_error(ctx, "read_boxes: box " + std::to_string(G.b0 + i) + ": status " + std::to_string(bst[i]));
                return bst[i];
            }
        if (!bounce.empty())
            for (uint32_t i = 0; i < nb; i++)
                if (P.box_bytes(G.b0 + i))
                    memcpy(outs[G.b0 + i], bounce.data() + (P.at[G.b0 + i] - P.at[G.b0]), P.box_bytes(G.b0 + i));
    }
    return ZCG_OK;
}

// write_ndarray for the boxes in order (ndarray.rs:276-385).  Per group: the
// slots of chunks whose first visiting box is partial are read (or, absent,
// prefilled); the boxes are scattered wave by wave; every slot is encoded and
// written.  host == true: ins are host buffers, dense in the chunk memory
// order.  varied, box_steps: plan_boxes'.
int write_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                const uint64_t* box_shape, const uint64_t* box_steps, const int64_t* in_strides, bool varied,
                const uint64_t* offsets,
                const void* const* ins, uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads,
                bool host) {
    const std::string what = "write_boxes";
    Plan P;
    // 1. before any file is read or written
    const int prc = plan_boxes(ctx, what, meta, root, path, box_shape, box_steps, in_strides, varied, 0, offsets, ins,
                               n_boxes, slot_budget_bytes, host, true, P);
    if (prc != ZCG_OK) return prc;
    if (P.nothing || P.at[n_boxes] == 0) return ZCG_OK;
    const zcg_region& r = P.r;
    const uint32_t nd = P.nd, es = P.es;
    const uint64_t fillv = meta->has_fill_value ? meta->fill_value : 0;
    const uint32_t threads = io_threads ? io_threads : 1;

    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, "write_boxes stream");
    std::vector<uint32_t> wave_of;

    for (size_t g = 0; g < P.groups.size(); g++) {
        const Group& G = P.groups[g];
        const uint32_t nb = G.b1 - G.b0, m = (uint32_t)G.keys.size();
        if (m == 0) continue;  // no box of the group visits a chunk: nothing to write
        const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = P.gentries[g];
        GroupSlots S;
        DevMem meta_dev, staging;
        int rc = group_slots(ctx, what, meta, root, path, P, g, S);
        if (rc != ZCG_OK) return rc;

        // 2. the existing chunks under a partial first box; absent ones start as fill value
        std::vector<void*> absent;
        {
            std::vector<uint32_t> idx;
            std::vector<const char*> rpaths;
            std::vector<void*> rptrs;
            for (uint32_t i = 0; i < m; i++)
                if (G.read_first[i]) {
                    idx.push_back(i);
                    rpaths.push_back(S.cpaths[i]);
                    rptrs.push_back(S.ptrs[i]);
                }
            if (!idx.empty()) {
                std::vector<int32_t> status(idx.size(), ZCG_OK);
                rc = zcg_store_read_chunks_device(ctx, &meta->array, (uint32_t)idx.size(), rpaths.data(), rptrs.data(),
                                                  status.data(), threads);
                if (rc != ZCG_OK) return rc;
                for (size_t k = 0; k < idx.size(); k++) {
                    if (status[k] == ZCG_ABSENT) absent.push_back(rptrs[k]);  // ndarray.rs:351-364
                    else if (status[k] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[idx[k]], status[k]);
                }
            }
        }

        // 3. device: [table entries][boxes nb][status nb][absent slots][scratch of the _v kernels]; every
        // visited chunk has a slot
        std::vector<void*> table(entries, nullptr);
        for (uint32_t i = 0; i < m; i++) table[S.tidx[i]] = S.ptrs[i];
        const uint64_t group_bytes = P.at[G.b1] - P.at[G.b0];
        const size_t o_box = (entries * sizeof(void*) + 255) & ~(size_t)255;
        const size_t o_st = (o_box + (size_t)nb * record_bytes(P) + 255) & ~(size_t)255;
        const size_t o_abs = (o_st + (size_t)nb * sizeof(int32_t) + 255) & ~(size_t)255;
        const size_t o_scr = (o_abs + absent.size() * sizeof(void*) + 255) & ~(size_t)255;
        if ((e = meta_dev.alloc(o_scr + (P.varied ? zcg_regions_v_scratch_bytes(nb) : 0))) != hipSuccess)
            return fail_hip(ctx, e, "write_boxes table");
        if (host && (e = staging.alloc(group_bytes)) != hipSuccess)
            return fail_hip(ctx, e, "write_boxes staging");
        const std::vector<uint8_t> boxes = box_records(P, offsets, ins, staging.p, G.b0, nb, host);
        uint8_t* db = (uint8_t*)meta_dev.p;
        std::vector<uint8_t> bounce;
        e = hipMemcpyAsync(db, table.data(), entries * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(db + o_box, boxes.data(), boxes.size(), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess && !absent.empty())
            e = hipMemcpyAsync(db + o_abs, absent.data(), absent.size() * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess && host) {
            // one H2D per group: straight from the caller's boxes when they are
            // consecutive in memory, else through a bounce buffer
            bool dense = true;
            for (uint32_t i = 1; i < nb && dense; i++)
                dense = (const uint8_t*)ins[G.b0 + i] == (const uint8_t*)ins[G.b0] + (P.at[G.b0 + i] - P.at[G.b0]);
            const uint8_t* src = (const uint8_t*)ins[G.b0];
            if (!dense) {
                bounce.resize(group_bytes);
                for (uint32_t i = 0; i < nb; i++)
                    if (P.box_bytes(G.b0 + i))
                        memcpy(bounce.data() + (P.at[G.b0 + i] - P.at[G.b0]), ins[G.b0 + i], P.box_bytes(G.b0 + i));
                src = bounce.data();
            }
            if (group_bytes) e = hipMemcpyAsync(staging.p, src, group_bytes, hipMemcpyHostToDevice, st.s);
        }
        if (e == hipSuccess)
            e = launch_slot_fill((void* const*)(db + o_abs), (uint32_t)absent.size(), P.D, es, fillv, st.s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st.s);  // the host vectors of an enqueued copy end with this scope
            return fail_hip(ctx, e, "write_boxes H2D");
        }

        // 4. the scatter, wave by wave: a later box wins what it shares with an earlier one
        wave_of.resize(nb);
        if (P.steps)
            zcg_regions_s_waves(&r, offsets + (size_t)G.b0 * nd, box_shape + (size_t)G.b0 * nd,
                                box_steps + (size_t)G.b0 * nd, nb, wave_of.data());
        else if (P.varied)
            zcg_regions_v_waves(&r, offsets + (size_t)G.b0 * nd, box_shape + (size_t)G.b0 * nd, nb, wave_of.data());
        else
            zcg_regions_waves(&r, offsets + (size_t)G.b0 * nd, nb, wave_of.data());
        for (uint32_t b0 = 0; b0 < nb;) {
            uint32_t b1 = b0 + 1;
            while (b1 < nb && wave_of[b1] == wave_of[b0]) b1++;
            rc = regions_launch(ctx, P, lo, n, db, db + o_box, b0, b1 - b0, db + o_scr, (int32_t*)(db + o_st), st.s, 1);
            if (rc != ZCG_OK) {
                (void)hipStreamSynchronize(st.s);
                return rc;
            }
            b0 = b1;
        }
        std::vector<int32_t> bst(nb, ZCG_OK);
        e = hipMemcpyAsync(bst.data(), db + o_st, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st.s);
        if (e == hipSuccess) e = hipStreamSynchronize(st.s);
        else (void)hipStreamSynchronize(st.s);
        if (e != hipSuccess) return fail_hip(ctx, e, "write_boxes scatter");
        for (uint32_t i = 0; i < nb; i++)
            if (bst[i] != ZCG_OK) {
                ctx_set_error(ctx, "write_boxes: box " + std::to_string(G.b0 + i) + ": status " + std::to_string(bst[i]));
                return bst[i];
            }

        // 5. encode and write every chunk of the group, once
        std::vector<int32_t> wst(m, ZCG_OK);
        rc = zcg_store_write_chunks_device(ctx, &meta->array, m, S.cpaths.data(), (const void* const*)S.ptrs.data(),
                                           wst.data(), threads);
        if (rc != ZCG_OK) return rc;
        for (uint32_t i = 0; i < m; i++)
            if (wst[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], wst[i]);
    }
    return ZCG_OK;
}

// a box's cells along one dimension: first and last cell index
struct CellRange {
    uint64_t lo, hi;
};

typedef unsigned __int128 u128;

// Do the progressions {o1 + i*s1, i < c1} and {o2 + j*s2, j < c2} share an
// index?  c1, c2 >= 1, s1, s2 >= 1, and both last samples are below 2^64.
// Exact, by the congruence x = o1 (mod s1), x = o2 (mod s2): solvable iff
// gcd(s1, s2) divides o2 - o1; the least solution at or above max(o1, o2) must
// not pass either last sample.  No loop over samples.
bool progressions_meet(uint64_t o1, uint64_t c1, uint64_t s1, uint64_t o2, uint64_t c2, uint64_t s2) {
    if (c1 < 2) s1 = 1;  // the step of a lone sample is irrelevant
    if (c2 < 2) s2 = 1;
    if (o1 > o2) { std::swap(o1, o2); std::swap(c1, c2); std::swap(s1, s2); }
    const u128 last1 = (u128)o1 + (u128)(c1 - 1) * s1, last2 = (u128)o2 + (u128)(c2 - 1) * s2;
    const u128 last = std::min(last1, last2);
    if (o2 > last) return false;
    uint64_t g = s1, h = s2;
    while (h) { const uint64_t t = g % h; g = h; h = t; }
    const uint64_t diff = o2 - o1;
    if (diff % g) return false;
    // x = o1 + s1*k with (s1/g)*k = diff/g (mod m), m = s2/g: k = (diff/g) * inverse of s1/g mod m
    const uint64_t m = s2 / g, a = (s1 / g) % m;
    uint64_t k = 0;
    if (m > 1) {
        __int128 t0 = 0, t1 = 1;  // extended Euclid: t1 * a = r1 (mod m)
        uint64_t r0 = m, r1 = a;
        while (r1 > 1) {
            const uint64_t q = r0 / r1, r2 = r0 - q * r1;
            const __int128 t2 = t0 - (__int128)q * t1;
            r0 = r1; r1 = r2; t0 = t1; t1 = t2;
        }
        const uint64_t inv = (uint64_t)(((t1 % (__int128)m) + m) % m);  // gcd(a, m) = 1, so r1 ends at 1
        k = (uint64_t)((u128)((diff / g) % m) * inv % m);
    }
    u128 x = (u128)o1 + (u128)s1 * k;  // the least solution at or above o1; the next ones are lcm apart
    if (x < o2) {
        const u128 lcm = (u128)(s1 / g) * s2, need = (u128)o2 - x;
        if (lcm > last) return false;  // the next solution is past every sample
        x += (need + lcm - 1) / lcm * lcm;
    }
    return x <= last;
}

// zcg_regions_waves, zcg_regions_v_waves and zcg_regions_s_waves: box b's
// shape is shapes + b * sstep (sstep 0: one shape for all); steps (n_boxes *
// ndim, or NULL): shapes are sample counts and two boxes intersect when their
// progressions do.  Cells and hashing go by the hulls.
uint32_t regions_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes, size_t sstep,
                       const uint64_t* steps, uint32_t n_boxes, uint32_t* wave_of) {
    if (!r || !offsets || !shapes || !wave_of || n_boxes == 0) return 0;
    const uint32_t nd = r->ndim;
    if (nd < 1 || nd > ZCG_MAX_DIMS) return 0;
    // strided: the hulls' extents (saturating) stand in for the shapes below;
    // a box with a step of 0 gets a zero extent and intersects nothing
    const uint64_t* counts = shapes;
    std::vector<uint64_t> hulls;
    std::vector<uint8_t> over;  // per box: a hull end passes 2^64
    if (steps) {
        hulls.assign((size_t)n_boxes * nd, 0);
        over.assign(n_boxes, 0);
        for (uint32_t b = 0; b < n_boxes; b++) {
            bool stepped = true;
            for (uint32_t d = 0; d < nd; d++) stepped &= steps[(size_t)b * nd + d] != 0;
            for (uint32_t d = 0; stepped && d < nd; d++) {
                const size_t i = (size_t)b * nd + d;
                const uint64_t c = counts[i];
                const u128 e = c ? (u128)(c - 1) * (c > 1 ? steps[i] : 1) + 1 : 0;
                hulls[i] = e > ~0ull ? ~0ull : (uint64_t)e;
                if (e + offsets[i] > ~0ull) over[b] = 1;
            }
        }
        shapes = hulls.data();
        sstep = nd;
    }
    // Cells: per dimension the smallest multiple of the chunk extent that holds
    // the largest box extent (r->bbox_shape, unless a box exceeds it), so a box
    // lies in at most two cells per dimension and two boxes that intersect
    // share a cell.  A box is compared with the boxes of the current wave that
    // are registered in one of its cells.
    uint64_t cell[ZCG_MAX_DIMS];
    for (uint32_t d = 0; d < nd; d++) {
        uint64_t bs = steps ? 0 : sstep ? r->bbox_shape[d] : shapes[d];
        for (uint32_t b = 0; sstep && b < n_boxes; b++) bs = std::max(bs, shapes[(size_t)b * sstep + d]);
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        const uint64_t k = std::max<uint64_t>(bs / cs + (bs % cs ? 1 : 0), 1);
        cell[d] = k > (~0ull) / cs ? ~0ull : k * cs;
    }
    auto end_of = [&](uint32_t b, uint32_t d) {
        const uint64_t o = offsets[(size_t)b * nd + d], e = o + shapes[(size_t)b * sstep + d];
        return e < o ? ~0ull : e;  // saturating
    };
    std::unordered_map<uint64_t, std::vector<uint32_t>> cells;  // hash of the cell position -> boxes
    uint32_t wave = 0;
    for (uint32_t b = 0; b < n_boxes; b++) {
        const uint64_t* ob = offsets + (size_t)b * nd;
        CellRange cr[ZCG_MAX_DIMS];
        bool has = true;  // false: the saturated extent is empty, the box intersects nothing
        uint32_t ncell = 1;
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t e = end_of(b, d);
            if (e <= ob[d]) { has = false; break; }
            cr[d] = CellRange{ob[d] / cell[d], (e - 1) / cell[d]};
            ncell *= (uint32_t)(cr[d].hi - cr[d].lo + 1);
        }
        if (!has) {
            wave_of[b] = wave;
            continue;
        }
        uint64_t keys[1u << ZCG_MAX_DIMS];
        for (uint32_t c = 0; c < ncell; c++) {
            uint64_t h = 0x9E3779B97F4A7C15ull;
            uint32_t rem = c;
            for (uint32_t d = 0; d < nd; d++) {
                const uint32_t w = (uint32_t)(cr[d].hi - cr[d].lo + 1);
                h = (h ^ (cr[d].lo + rem % w)) * 0xFF51AFD7ED558CCDull;
                h ^= h >> 32;
                rem /= w;
            }
            keys[c] = h;
        }
        bool hit = false;
        for (uint32_t c = 0; c < ncell && !hit; c++) {
            auto it = cells.find(keys[c]);
            if (it == cells.end()) continue;
            for (uint32_t a : it->second) {
                const uint64_t* oa = offsets + (size_t)a * nd;
                bool meet = true;
                const bool exact = steps && !over[a] && !over[b];  // else the (saturated) hulls' intervals
                for (uint32_t d = 0; d < nd && meet; d++)
                    meet = exact ? progressions_meet(oa[d], counts[(size_t)a * nd + d], steps[(size_t)a * nd + d],
                                                     ob[d], counts[(size_t)b * nd + d], steps[(size_t)b * nd + d])
                                 : std::max(oa[d], ob[d]) < std::min(end_of(a, d), end_of(b, d));
                if (meet) { hit = true; break; }
            }
        }
        if (hit) {
            wave++;
            cells.clear();
        }
        wave_of[b] = wave;
        for (uint32_t c = 0; c < ncell; c++) cells[keys[c]].push_back(b);
    }
    return wave + 1;
}

}  // namespace

extern "C" uint32_t zcg_regions_waves(const zcg_region* r, const uint64_t* offsets, uint32_t n_boxes,
                                      uint32_t* wave_of) {
    return regions_waves(r, offsets, r ? r->bbox_shape : nullptr, 0, nullptr, n_boxes, wave_of);
}

extern "C" uint32_t zcg_regions_v_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                                        uint32_t n_boxes, uint32_t* wave_of) {
    return regions_waves(r, offsets, shapes, r ? r->ndim : 0, nullptr, n_boxes, wave_of);
}

extern "C" uint32_t zcg_regions_s_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                                        const uint64_t* steps, uint32_t n_boxes, uint32_t* wave_of) {
    if (!steps) return 0;
    return regions_waves(r, offsets, shapes, r ? r->ndim : 0, steps, n_boxes, wave_of);
}

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
extern "C" uint64_t zcg_points_last(const uint64_t* coords, uint64_t n_points, uint32_t ndim, uint8_t* keep) {
    if (!coords || !keep || ndim < 1 || ndim > ZCG_MAX_DIMS) return 0;
    std::vector<uint64_t> idx(n_points);
    for (uint64_t i = 0; i < n_points; i++) idx[i] = i;
    // equal coordinates next to each other, the latest point last
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
        const uint64_t *ca = coords + a * ndim, *cb = coords + b * ndim;
        for (uint32_t d = 0; d < ndim; d++)
            if (ca[d] != cb[d]) return ca[d] < cb[d];
        return a < b;
    });
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n_points; i++) {
        const bool last = i + 1 == n_points ||
                          memcmp(coords + idx[i] * ndim, coords + idx[i + 1] * ndim, ndim * sizeof(uint64_t)) != 0;
        keep[idx[i]] = last ? 1 : 0;
        kept += last;
    }
    return kept;
}

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
    if (!ctx || !meta || !root || !path) return ZCG_ERR_INVALID_INPUT;
    if (n_points && (!coords || !buf)) return ZCG_ERR_INVALID_INPUT;
    auto say = [&](const std::string& e) { ctx_set_error(ctx, e); };
    const int mrc = meta_args_status(what, meta, say);
    if (mrc != ZCG_OK) return mrc;
    const uint32_t nd = meta->ndim;
    const uint32_t es = meta->array.dtype.elem_size;
    if (es != 1 && es != 2 && es != 4 && es != 8) return ZCG_ERR_INVALID_INPUT;
    P.nd = nd;
    P.es = es;
    if (n_points == 0) {
        P.nothing = true;
        return ZCG_OK;
    }
    if (n_points >= (1ull << 32)) {  // Group::b0 / b1
        ctx_set_error(ctx, what + ": more than 2^32 points in one call");
        return ZCG_ERR_UNSUPPORTED;
    }
    zcg_region& r = P.r;
    memset(&r, 0, sizeof r);
    r.ndim = nd;
    r.elem_size = es;
    r.chunk_order = meta->chunk_order;
    r.fill_missing = fill_missing ? 1u : 0u;
    r.fill_value = meta->has_fill_value ? meta->fill_value : 0;
    uint64_t extent[ZCG_MAX_DIMS], cstr[ZCG_MAX_DIMS];
    for (uint32_t d = 0; d < nd; d++) {
        if (meta->chunk_shape[d] == 0) return ZCG_ERR_INVALID_INPUT;
        r.array_shape[d] = meta->shape[d];
        r.chunk_shape[d] = meta->chunk_shape[d];
        r.bbox_shape[d] = 1;
        extent[d] = u64_ceil_div(meta->shape[d], meta->chunk_shape[d]);
    }
    {
        uint64_t g = 1, c = 1;
        for (int d = (int)nd - 1; d >= 0; d--) {
            P.gstr[d] = g;
            if (extent[d] && g > (~0ull) / extent[d]) {
                ctx_set_error(ctx, what + ": the array's chunk grid exceeds 2^64 chunks");
                return ZCG_ERR_UNSUPPORTED;
            }
            g *= extent[d];
        }
        for (uint32_t k = 0; k < nd; k++) {
            const uint32_t d = meta->chunk_order == 1 ? k : nd - 1 - k;
            cstr[d] = c;
            c *= meta->chunk_shape[d];
        }
    }
    const uint64_t D = P.D = meta->array.chunk_num_elements * (uint64_t)es;
    const uint64_t budget = slot_budget_bytes ? slot_budget_bytes : BOXES_DEFAULT_BUDGET;
    const uint64_t max_chunks = std::max<uint64_t>(budget / std::max<uint64_t>(D, 1), 1);

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

// The device side of one group of sorted points: [table entries][coordinates
// np * nd][original indices np][the word for points outside the table].
struct PointsDev {
    DevMem mem;
    size_t o_co = 0, o_ord = 0, o_fo = 0;
    std::vector<uint64_t> host;  // coordinates, then indices
};

hipError_t points_upload(const Plan& P, const Group& G, const std::vector<SortedPoint>& pts, const uint64_t* coords,
                         const void* const* table, uint64_t entries, PointsDev& X, hipStream_t s) {
    const uint32_t nd = P.nd;
    const size_t np = G.b1 - G.b0;
    X.o_co = (entries * sizeof(void*) + 255) & ~(size_t)255;
    X.o_ord = X.o_co + np * nd * sizeof(uint64_t);
    X.o_fo = X.o_ord + np * sizeof(uint64_t);
    hipError_t e = X.mem.alloc(X.o_fo + sizeof(uint64_t));
    if (e != hipSuccess) return e;
    X.host.resize(np * nd + np);
    for (size_t i = 0; i < np; i++) {
        const SortedPoint& sp = pts[G.b0 + i];
        memcpy(&X.host[i * nd], coords + sp.i * nd, nd * sizeof(uint64_t));
        X.host[np * nd + i] = sp.i;
    }
    uint8_t* db = (uint8_t*)X.mem.p;
    if (entries) e = hipMemcpyAsync(db, table, entries * sizeof(void*), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(db + X.o_co, X.host.data(), X.host.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    return e;
}

int points_outside(zcg_ctx* ctx, const std::string& what, uint64_t first_outside) {
    if (first_outside == ~0ull) return ZCG_OK;
    ctx_set_error(ctx, what + ": sorted point " + std::to_string(first_outside) + " fell outside its group's table");
    return ZCG_ERR_RUNTIME;
}

int read_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path, const uint64_t* coords,
                uint64_t n_points, uint32_t fill_missing, void* out, uint64_t slot_budget_bytes, uint32_t io_threads,
                bool host) {
    const std::string what = "read_points";
    Plan P;
    std::vector<SortedPoint> pts;
    // 1. before any file is read
    const int prc = plan_points(ctx, what, meta, root, path, host ? 1 : fill_missing, coords, out, n_points, nullptr,
                                slot_budget_bytes, P, pts);
    if (prc != ZCG_OK) return prc;
    if (P.nothing) return ZCG_OK;
    const uint32_t es = P.es;

    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, "read_points stream");

    // 2. per group: read + decode its chunks once, build the table, one launch
    std::vector<uint8_t> bounce;
    for (size_t g = 0; g < P.groups.size(); g++) {
        const Group& G = P.groups[g];
        const uint32_t m = (uint32_t)G.keys.size();
        const size_t np = G.b1 - G.b0;
        const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = P.gentries[g];
        GroupSlots S;
        DevMem staging;
        std::vector<const void*> table(std::max<uint64_t>(entries, 1), nullptr);
        if (m) {
            int rc = group_slots(ctx, what, meta, root, path, P, g, S);
            if (rc != ZCG_OK) return rc;
            std::vector<int32_t> status(m, ZCG_OK);
            rc = zcg_store_read_chunks_device(ctx, &meta->array, m, S.cpaths.data(), S.ptrs.data(), status.data(),
                                              io_threads ? io_threads : 1);
            if (rc != ZCG_OK) return rc;
            for (uint32_t i = 0; i < m; i++) {
                if (status[i] == ZCG_ABSENT) continue;  // read_chunk -> Ok(None): a NULL entry
                if (status[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], status[i]);
                table[S.tidx[i]] = S.ptrs[i];
            }
        }
        PointsDev X;
        if (host && (e = staging.alloc(np * es)) != hipSuccess) return fail_hip(ctx, e, "read_points staging");
        e = points_upload(P, G, pts, coords, table.data(), entries, X, st.s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st.s);  // the host vectors of an enqueued copy end with this scope
            return fail_hip(ctx, e, "read_points H2D");
        }
        uint8_t* db = (uint8_t*)X.mem.p;
        // host: the group's values in sorted order, permuted below; device: straight to the caller's order
        const int rc = points_call(ctx, &P.r, lo, n, (const void* const*)db, (const uint64_t*)(db + X.o_co),
                                   host ? nullptr : (const uint64_t*)(db + X.o_ord), np, host ? staging.p : out,
                                   (uint64_t*)(db + X.o_fo), (void*)st.s, 0);
        if (rc != ZCG_OK) {
            (void)hipStreamSynchronize(st.s);
            return rc;
        }
        uint64_t first_outside = ~0ull;
        e = hipMemcpyAsync(&first_outside, db + X.o_fo, sizeof first_outside, hipMemcpyDeviceToHost, st.s);
        if (e == hipSuccess && host) {
            bounce.resize(np * es);
            e = hipMemcpyAsync(bounce.data(), staging.p, np * es, hipMemcpyDeviceToHost, st.s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st.s);
        else (void)hipStreamSynchronize(st.s);
        if (e != hipSuccess) return fail_hip(ctx, e, "read_points assembly");
        const int orc = points_outside(ctx, what, first_outside);
        if (orc != ZCG_OK) return orc;
        if (host)
            for (size_t i = 0; i < np; i++)
                memcpy((uint8_t*)out + pts[G.b0 + i].i * es, bounce.data() + i * es, es);
    }
    return ZCG_OK;
}

// write_ndarray for the 1-element boxes of point 0, 1, ... in order: of two
// points with one coordinate the later one counts (zcg_points_last), so the
// kernel never sees two values for one element.  Per group: every chunk is
// read (or, absent, prefilled) unless it has one element, the points are
// scattered, and every chunk of the group is encoded and written once.
int write_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path, const uint64_t* coords,
                 uint64_t n_points, const void* in, uint64_t slot_budget_bytes, uint32_t io_threads, bool host) {
    const std::string what = "write_points";
    Plan P;
    std::vector<SortedPoint> pts;
    std::vector<uint8_t> keep(n_points, 1);
    if (coords && meta && meta->ndim >= 1 && meta->ndim <= ZCG_MAX_DIMS)
        zcg_points_last(coords, n_points, meta->ndim, keep.data());
    // 1. before any file is read or written
    const int prc = plan_points(ctx, what, meta, root, path, 0, coords, in, n_points, keep.data(), slot_budget_bytes,
                                P, pts);
    if (prc != ZCG_OK) return prc;
    if (P.nothing) return ZCG_OK;
    const uint32_t es = P.es;
    const uint64_t fillv = meta->has_fill_value ? meta->fill_value : 0;
    const uint32_t threads = io_threads ? io_threads : 1;

    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, "write_points stream");

    std::vector<uint8_t> bounce;
    for (size_t g = 0; g < P.groups.size(); g++) {
        const Group& G = P.groups[g];
        const uint32_t m = (uint32_t)G.keys.size();
        const size_t np = G.b1 - G.b0;
        if (m == 0) continue;
        const uint64_t* lo = &P.glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &P.gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = P.gentries[g];
        GroupSlots S;
        DevMem staging, absent_dev;
        int rc = group_slots(ctx, what, meta, root, path, P, g, S);
        if (rc != ZCG_OK) return rc;

        // 2. the existing chunks; absent ones start as fill value
        std::vector<void*> absent;
        if (G.read_first[0]) {
            std::vector<int32_t> status(m, ZCG_OK);
            rc = zcg_store_read_chunks_device(ctx, &meta->array, m, S.cpaths.data(), S.ptrs.data(), status.data(),
                                              threads);
            if (rc != ZCG_OK) return rc;
            for (uint32_t i = 0; i < m; i++) {
                if (status[i] == ZCG_ABSENT) absent.push_back(S.ptrs[i]);  // ndarray.rs:351-364
                else if (status[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], status[i]);
            }
        }

        // 3. the table (every chunk of the group has a slot), the points, the values
        std::vector<void*> table(entries, nullptr);
        for (uint32_t i = 0; i < m; i++) table[S.tidx[i]] = S.ptrs[i];
        PointsDev X;
        if (host && (e = staging.alloc(np * es)) != hipSuccess) return fail_hip(ctx, e, "write_points staging");
        if (!absent.empty() && (e = absent_dev.alloc(absent.size() * sizeof(void*))) != hipSuccess)
            return fail_hip(ctx, e, "write_points table");
        e = points_upload(P, G, pts, coords, (const void* const*)table.data(), entries, X, st.s);
        if (e == hipSuccess && !absent.empty())
            e = hipMemcpyAsync(absent_dev.p, absent.data(), absent.size() * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess && host) {
            bounce.resize(np * es);
            for (size_t i = 0; i < np; i++)
                memcpy(bounce.data() + i * es, (const uint8_t*)in + pts[G.b0 + i].i * es, es);
            e = hipMemcpyAsync(staging.p, bounce.data(), np * es, hipMemcpyHostToDevice, st.s);
        }
        if (e == hipSuccess)
            e = launch_slot_fill((void* const*)absent_dev.p, (uint32_t)absent.size(), P.D, es, fillv, st.s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st.s);  // the host vectors of an enqueued copy end with this scope
            return fail_hip(ctx, e, "write_points H2D");
        }

        // 4. the scatter: no two points of the call share an element
        uint8_t* db = (uint8_t*)X.mem.p;
        rc = points_call(ctx, &P.r, lo, n, (const void* const*)db, (const uint64_t*)(db + X.o_co),
                         host ? nullptr : (const uint64_t*)(db + X.o_ord), np, host ? staging.p : (void*)in,
                         (uint64_t*)(db + X.o_fo), (void*)st.s, 1);
        if (rc != ZCG_OK) {
            (void)hipStreamSynchronize(st.s);
            return rc;
        }
        uint64_t first_outside = ~0ull;
        e = hipMemcpyAsync(&first_outside, db + X.o_fo, sizeof first_outside, hipMemcpyDeviceToHost, st.s);
        if (e == hipSuccess) e = hipStreamSynchronize(st.s);
        else (void)hipStreamSynchronize(st.s);
        if (e != hipSuccess) return fail_hip(ctx, e, "write_points scatter");
        rc = points_outside(ctx, what, first_outside);
        if (rc != ZCG_OK) return rc;

        // 5. encode and write every chunk of the group, once
        std::vector<int32_t> wst(m, ZCG_OK);
        rc = zcg_store_write_chunks_device(ctx, &meta->array, m, S.cpaths.data(), (const void* const*)S.ptrs.data(),
                                           wst.data(), threads);
        if (rc != ZCG_OK) return rc;
        for (uint32_t i = 0; i < m; i++)
            if (wst[i] != ZCG_OK) return chunk_failed(ctx, what, P, G.keys[i], wst[i]);
    }
    return ZCG_OK;
}

}  // namespace

extern "C" int zcg_store_read_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                            const char* path, const uint64_t* coords, uint64_t n_points,
                                            uint32_t fill_missing, void* d_out, uint64_t slot_budget_bytes,
                                            uint32_t io_threads) {
    return read_points(ctx, meta, root, path, coords, n_points, fill_missing, d_out, slot_budget_bytes, io_threads,
                       false);
}

extern "C" int zcg_store_read_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                     const uint64_t* coords, uint64_t n_points, void* out,
                                     uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_points(ctx, meta, root, path, coords, n_points, 1, out, slot_budget_bytes, io_threads, true);
}

extern "C" int zcg_store_write_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                             const char* path, const uint64_t* coords, uint64_t n_points,
                                             const void* d_in, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_points(ctx, meta, root, path, coords, n_points, d_in, slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_write_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                      const uint64_t* coords, uint64_t n_points, const void* in,
                                      uint64_t slot_budget_bytes, uint32_t io_threads) {
    return write_points(ctx, meta, root, path, coords, n_points, in, slot_budget_bytes, io_threads, true);
}
