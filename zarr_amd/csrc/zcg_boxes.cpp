// zcg_boxes.cpp — read_ndarray for many bounding boxes in one native call
// (ZarrNdarrayReader::read_ndarray, src/ndarray.rs:153-268, once per box in the
// reference): the chunks all boxes visit are read and decoded once
// (zcg_store_read_chunks_device), and every box is assembled from the shared
// chunk table by one zcg_read_regions launch.
//
// Boxes are taken in consecutive groups whose unique chunks fit a budget of
// decoded device slots; a chunk two groups share is decoded in each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_set>
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
    std::vector<uint64_t> keys;  // unique visited chunks, as linear indices over the array's grid
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

// host == true: outs are host buffers, each box dense in the chunk memory
// order with fill (read_ndarray); else device views with the caller's strides
int read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
               const uint64_t* box_shape, const int64_t* out_strides, uint32_t fill_missing,
               const uint64_t* offsets, void* const* outs, uint32_t n_boxes, uint64_t slot_budget_bytes,
               uint32_t io_threads, bool host) {
    if (!ctx || !meta || !root || !path || !box_shape || (!host && !out_strides)) return ZCG_ERR_INVALID_INPUT;
    if (n_boxes && (!offsets || !outs)) return ZCG_ERR_INVALID_INPUT;
    if (meta->ndim != meta->chunk_ndim) {
        ctx_set_error(ctx, "read_boxes: shape and chunk_shape differ in their number of dimensions");
        return ZCG_ERR_INVALID_DATA;
    }
    const uint32_t nd = meta->ndim;
    if (nd < 1 || nd > ZCG_MAX_DIMS) return ZCG_ERR_INVALID_INPUT;
    if (meta->dtype_kind == ZCG_DT_RAW) {
        ctx_set_error(ctx, "read_boxes: raw (rN) element types have no ndarray form");
        return ZCG_ERR_INVALID_INPUT;
    }
    const uint32_t es = meta->array.dtype.elem_size;
    if (es != 1 && es != 2 && es != 4 && es != 8) return ZCG_ERR_INVALID_INPUT;
    if (n_boxes == 0) return ZCG_OK;

    zcg_region r;
    memset(&r, 0, sizeof r);
    r.ndim = nd;
    r.elem_size = es;
    r.chunk_order = meta->chunk_order;
    r.fill_missing = host ? 1u : (fill_missing ? 1u : 0u);
    r.fill_value = meta->has_fill_value ? meta->fill_value : 0;
    uint64_t extent[ZCG_MAX_DIMS], gstr[ZCG_MAX_DIMS], box_elems = 1;
    for (uint32_t d = 0; d < nd; d++) {
        if (meta->chunk_shape[d] == 0) return ZCG_ERR_INVALID_INPUT;
        r.array_shape[d] = meta->shape[d];
        r.chunk_shape[d] = meta->chunk_shape[d];
        r.bbox_shape[d] = box_shape[d];
        extent[d] = u64_ceil_div(meta->shape[d], meta->chunk_shape[d]);
        box_elems *= box_shape[d];
    }
    {   // dense host layout in the chunk memory order; linear chunk keys over the grid
        int64_t acc = 1;
        uint64_t g = 1;
        for (uint32_t k = 0; k < nd; k++) {
            const uint32_t d = meta->chunk_order == 1 ? k : nd - 1 - k;
            r.out_strides[d] = host ? acc : out_strides[d];
            acc *= (int64_t)std::max<uint64_t>(box_shape[d], 1);
        }
        for (int d = (int)nd - 1; d >= 0; d--) {
            gstr[d] = g;
            if (extent[d] && g > (~0ull) / extent[d]) {
                ctx_set_error(ctx, "read_boxes: the array's chunk grid exceeds 2^64 chunks");
                return ZCG_ERR_UNSUPPORTED;
            }
            g *= extent[d];
        }
    }
    const uint64_t D = meta->array.chunk_num_elements * (uint64_t)es;
    const uint64_t budget = slot_budget_bytes ? slot_budget_bytes : BOXES_DEFAULT_BUDGET;

    // 1. every box's visited chunks: in bounds (the reference panics at
    //    storage.rs:217), grouped under the slot budget — before any file is read
    std::vector<Group> groups;
    {
        std::unordered_set<uint64_t> seen;
        std::vector<uint64_t> fresh;
        Group cur{0, 0, {}};
        for (uint32_t b = 0; b < n_boxes; b++) {
            uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS], pos[ZCG_MAX_DIMS];
            for (uint32_t d = 0; d < nd; d++) r.bbox_offset[d] = offsets[(size_t)b * nd + d];
            const uint64_t cnt = zcg_region_grid(&r, lo, n);
            for (uint32_t d = 0; cnt && d < nd; d++)
                if (lo[d] + n[d] > extent[d]) {
                    for (uint32_t k = 0; k < nd; k++) pos[k] = lo[k] + n[k] - 1;
                    ctx_set_error(ctx, "read_boxes: box " + std::to_string(b) + " visits chunk " + pos_text(pos, nd) +
                                           " outside the array's chunk grid");
                    return ZCG_ERR_INVALID_INPUT;
                }
            if (cnt > BOXES_MAX_TABLE) {
                ctx_set_error(ctx, "read_boxes: a chunk table above 2^24 entries is not supported");
                return ZCG_ERR_UNSUPPORTED;
            }
            auto visit = [&](std::unordered_set<uint64_t>& set, std::vector<uint64_t>& added) {
                added.clear();
                for (uint64_t i = 0; i < cnt; i++) {
                    uint64_t rem = i, key = 0;
                    for (int d = (int)nd - 1; d >= 0; d--) {
                        key += (lo[d] + rem % n[d]) * gstr[d];
                        rem /= n[d];
                    }
                    if (set.insert(key).second) added.push_back(key);
                }
            };
            visit(seen, fresh);
            if (b > cur.b0 && (uint64_t)seen.size() > budget / std::max<uint64_t>(D, 1)) {
                // this box does not fit beside the others: it starts the next group
                for (uint64_t k : fresh) seen.erase(k);
                cur.b1 = b;
                cur.keys.assign(seen.begin(), seen.end());
                groups.push_back(std::move(cur));
                cur = Group{b, b, {}};
                seen.clear();
                visit(seen, fresh);
            }
        }
        cur.b1 = n_boxes;
        cur.keys.assign(seen.begin(), seen.end());
        groups.push_back(std::move(cur));
    }
    std::vector<uint64_t> glo(groups.size() * ZCG_MAX_DIMS), gn(groups.size() * ZCG_MAX_DIMS), gentries(groups.size());
    for (size_t g = 0; g < groups.size(); g++) {
        Group& G = groups[g];
        std::sort(G.keys.begin(), G.keys.end());
        gentries[g] = zcg_regions_grid(&r, offsets + (size_t)G.b0 * nd, G.b1 - G.b0, &glo[g * ZCG_MAX_DIMS],
                                       &gn[g * ZCG_MAX_DIMS]);
        if (gentries[g] > BOXES_MAX_TABLE) {
            ctx_set_error(ctx, "read_boxes: the boxes' union chunk table (" + std::to_string(gentries[g]) +
                                   " entries) exceeds 2^24; read the boxes in several calls");
            return ZCG_ERR_UNSUPPORTED;
        }
    }
    if (box_elems == 0) return ZCG_OK;

    (void)hipSetDevice(ctx_device(ctx));
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(ctx, e, "read_boxes stream");
    const uint64_t box_bytes = box_elems * es;

    // 2. per group: read + decode its chunks once, build the table, one launch
    for (size_t g = 0; g < groups.size(); g++) {
        const Group& G = groups[g];
        const uint32_t nb = G.b1 - G.b0, m = (uint32_t)G.keys.size();
        const uint64_t* lo = &glo[g * ZCG_MAX_DIMS];
        const uint64_t* n = &gn[g * ZCG_MAX_DIMS];
        const uint64_t entries = gentries[g];
        DevMem slots, meta_dev, staging;
        std::vector<const void*> table(std::max<uint64_t>(entries, 1), nullptr);
        if (m) {
            if ((e = slots.alloc((size_t)m * D)) != hipSuccess) return fail_hip(ctx, e, "read_boxes slots");
            std::vector<std::string> paths(m);
            std::vector<const char*> cpaths(m);
            std::vector<void*> dsts(m);
            std::vector<int32_t> status(m, ZCG_OK);
            std::vector<uint64_t> tidx(m);
            std::string key;
            for (uint32_t i = 0; i < m; i++) {
                uint64_t pos[ZCG_MAX_DIMS], rem = G.keys[i], ti = 0, tstr = 1;
                for (uint32_t d = 0; d < nd; d++) { pos[d] = rem / gstr[d]; rem -= pos[d] * gstr[d]; }
                for (int d = (int)nd - 1; d >= 0; d--) { ti += (pos[d] - lo[d]) * tstr; tstr *= n[d]; }
                tidx[i] = ti;
                key.resize(zcg_chunk_key(path, meta->separator, pos, nd, nullptr, 0) + 1);
                zcg_chunk_key(path, meta->separator, pos, nd, &key[0], key.size());
                uint64_t plen = 0;
                int rc = zcg_store_path(root, key.c_str(), nullptr, 0, &plen);
                if (rc == ZCG_OK) {
                    paths[i].resize(plen + 1);
                    rc = zcg_store_path(root, key.c_str(), &paths[i][0], plen + 1, nullptr);
                }
                if (rc != ZCG_OK) {
                    ctx_set_error(ctx, "read_boxes: chunk " + pos_text(pos, nd) + ": key outside the hierarchy");
                    return rc;
                }
                cpaths[i] = paths[i].c_str();
                dsts[i] = (uint8_t*)slots.p + (size_t)i * D;
            }
            const int rc = zcg_store_read_chunks_device(ctx, &meta->array, m, cpaths.data(), dsts.data(),
                                                        status.data(), io_threads ? io_threads : 1);
            if (rc != ZCG_OK) return rc;
            for (uint32_t i = 0; i < m; i++) {
                if (status[i] == ZCG_ABSENT) continue;  // read_chunk -> Ok(None): a NULL entry
                if (status[i] != ZCG_OK) {
                    uint64_t pos[ZCG_MAX_DIMS], rem = G.keys[i];
                    for (uint32_t d = 0; d < nd; d++) { pos[d] = rem / gstr[d]; rem -= pos[d] * gstr[d]; }
                    ctx_set_error(ctx, "read_boxes: chunk " + pos_text(pos, nd) + ": status " + std::to_string(status[i]));
                    return status[i];
                }
                table[tidx[i]] = dsts[i];
            }
        }
        // device: [table entries][boxes nb][status nb]
        const size_t o_box = (entries * sizeof(void*) + 255) & ~(size_t)255;
        const size_t o_st = (o_box + (size_t)nb * sizeof(zcg_box) + 255) & ~(size_t)255;
        if ((e = meta_dev.alloc(o_st + (size_t)nb * sizeof(int32_t))) != hipSuccess)
            return fail_hip(ctx, e, "read_boxes table");
        if (host && (e = staging.alloc((size_t)nb * box_bytes)) != hipSuccess)
            return fail_hip(ctx, e, "read_boxes staging");
        std::vector<zcg_box> boxes(nb);
        for (uint32_t i = 0; i < nb; i++) {
            memset(&boxes[i], 0, sizeof(zcg_box));
            for (uint32_t d = 0; d < nd; d++) boxes[i].offset[d] = offsets[(size_t)(G.b0 + i) * nd + d];
            boxes[i].out = host ? (void*)((uint8_t*)staging.p + (size_t)i * box_bytes) : outs[G.b0 + i];
        }
        uint8_t* db = (uint8_t*)meta_dev.p;
        if (entries) e = hipMemcpyAsync(db, table.data(), entries * sizeof(void*), hipMemcpyHostToDevice, st.s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(db + o_box, boxes.data(), (size_t)nb * sizeof(zcg_box), hipMemcpyHostToDevice, st.s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st.s);  // the host vectors of an enqueued copy end with this scope
            return fail_hip(ctx, e, "read_boxes H2D");
        }
        const int rc = zcg_read_regions(ctx, &r, lo, n, (const void* const*)db, (const zcg_box*)(db + o_box), nb,
                                        (int32_t*)(db + o_st), (void*)st.s);
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
                dense = (uint8_t*)outs[G.b0 + i] == (uint8_t*)outs[G.b0] + (size_t)i * box_bytes;
            uint8_t* dst = (uint8_t*)outs[G.b0];
            if (!dense) {
                bounce.resize((size_t)nb * box_bytes);
                dst = bounce.data();
            }
            e = hipMemcpyAsync(dst, staging.p, (size_t)nb * box_bytes, hipMemcpyDeviceToHost, st.s);
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
            for (uint32_t i = 0; i < nb; i++) memcpy(outs[G.b0 + i], bounce.data() + (size_t)i * box_bytes, box_bytes);
    }
    return ZCG_OK;
}

}  // namespace

extern "C" int zcg_store_read_boxes_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root,
                                           const char* path, const uint64_t* box_shape, const int64_t* out_strides,
                                           uint32_t fill_missing, const uint64_t* offsets, void* const* d_outs,
                                           uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shape, out_strides, fill_missing, offsets, d_outs, n_boxes,
                      slot_budget_bytes, io_threads, false);
}

extern "C" int zcg_store_read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                    const uint64_t* box_shape, const uint64_t* offsets, void* const* outs,
                                    uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads) {
    return read_boxes(ctx, meta, root, path, box_shape, nullptr, 1, offsets, outs, n_boxes, slot_budget_bytes,
                      io_threads, true);
}
