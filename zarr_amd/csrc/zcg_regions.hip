// zcg_regions.hip — batched region assembly: many bounding boxes of one
// common shape, each at its own offset and into its own output view, read from
// one shared chunk table in one launch (zcg_read_regions).
//
// Per box the semantics are those of zcg_region.hip (bounded_coord_iter's
// grid range, overhanging edge chunks, fill versus untouched): a box behaves
// exactly as a zcg_read_region call with its offset and a table over its own
// grid range would.  The shared table only supplies the pointers; a chunk of
// the table outside the box's own grid range is never read.
//
// Work is the flattened (box, tile) or (box, row piece) space.  The box of a
// work unit is wave-uniform, so everything that depends on the box alone —
// offset mod chunk extent, the box's grid range, its base index in the shared
// table, whether that range lies in the table — is computed once per work
// unit from d_boxes[b].offset on the scalar side; the walk inside the box is
// zcg_region.hip's: the chunks' memory order, 16 bytes per lane, per-element
// runs where a piece crosses a chunk or row boundary.  The per-dimension loops
// are unrolled to ZCG_MAX_DIMS so the per-box terms stay in registers.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"

namespace zcg {

namespace {

// what one box adds to the shared arguments (wave-uniform)
struct BoxTerms {
    u32 orr[ZCG_MAX_DIMS];  // box offset mod chunk extent
    u32 gn[ZCG_MAX_DIMS];   // chunks the box visits along the dim (its own grid range)
    const u8* const* table; // the shared table at the box's first chunk
    u8* out;                // element (0, ..., 0) of the box's view
    bool in_table;          // the box's grid range lies inside the table's
};

__device__ __forceinline__ BoxTerms box_terms(const RegionsArgs& a, const u8* const* __restrict__ table,
                                              const zcg_box* __restrict__ boxes, u64 b) {
    BoxTerms t;
    const zcg_box* bx = boxes + b;
    u64 base = 0;
    bool inside = true, visits = true;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        t.orr[k] = 0;
        t.gn[k] = 0;
        if (k >= a.nd) continue;
        // bounded_coord_iter (ndarray.rs:410-432), as zcg_region_grid states it:
        // the box clipped to the array, floor / ceil by the chunk extent
        const u64 off = ru64(bx->offset[a.dim[k]]);
        const u64 cs = a.cs[k];
        const u64 lo = off / cs;
        const u64 orr = off - lo * cs;
        const u64 end = off + a.bs[k] < a.as[k] ? off + a.bs[k] : a.as[k];
        const u64 s = end > off ? end - off : 0;
        // ceil((off + s) / cs) - lo, in 32 bits: orr + s <= chunk extent - 1 +
        // box extent < 2^32 (checked by the host)
        const u32 span = (u32)orr + (u32)s, nq = span / a.cs[k];
        const u32 n = nq + (span != nq * a.cs[k] ? 1u : 0u);
        t.orr[k] = (u32)orr;
        t.gn[k] = n;
        visits &= n != 0;
        inside &= lo >= a.tlo[k] && lo - a.tlo[k] + n <= a.tn[k];
        base += (lo - a.tlo[k]) * a.tstr[k];
    }
    // a box that visits no chunk reads no table entry: it is filled (or left
    // untouched) wherever the table is
    t.in_table = inside || !visits;
    t.table = table + (visits && inside ? base : 0);
    t.out = (u8*)(uintptr_t)ru64((u64)(uintptr_t)bx->out);
    return t;
}

// where element p of the box is read from (nullptr: no visited chunk), and
// how many elements from it stay in one chunk row and one box row
__device__ __forceinline__ const u8* boxes_src(const RegionsArgs& a, const BoxTerms& t, const Pos& p, u32* run) {
    u64 ti = 0, wi = 0;
    bool ok = true;
    u32 w0 = 0;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= a.nd) break;
        const u32 r = t.orr[k] + p.x[k];
        const u32 q = r / a.cs[k];
        const u32 w = r - q * a.cs[k];
        if (k == 0) w0 = w;
        ok &= q < t.gn[k];
        ti += (u64)q * a.tstr[k];
        wi += (u64)w * a.cstr[k];
    }
    const u32 r1 = a.bs[0] - p.x[0], r2 = a.cs[0] - w0;
    *run = r1 < r2 ? r1 : r2;
    if (!ok) return nullptr;
    const u8* base = t.table[ti];
    return base ? base + wi * a.es : nullptr;
}

__device__ __forceinline__ i64 boxes_dst(const RegionsArgs& a, const Pos& p) {
    i64 o = 0;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= a.nd) break;
        o += (i64)p.x[k] * a.ostr[k];
    }
    return o;
}

// advance p by d elements along the fast-first order (carries)
__device__ __forceinline__ void boxes_advance(const RegionsArgs& a, Pos& p, u32 d) {
    u32 c = d;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= a.nd || !c) break;
        const u64 v = (u64)p.x[k] + c;
        if (v < a.bs[k]) { p.x[k] = (u32)v; c = 0; break; }
        const u64 q = v / a.bs[k];
        p.x[k] = (u32)(v - q * a.bs[k]);
        c = (u32)q;
    }
}

__device__ __forceinline__ u64 fill_pattern(u64 fv, u32 es) {
    if (es == 1) return (fv & 0xFF) * 0x0101010101010101ull;
    if (es == 2) return (fv & 0xFFFF) * 0x0001000100010001ull;
    if (es == 4) return (fv & 0xFFFFFFFFull) * 0x0000000100000001ull;
    return fv;
}

// one lane says how the box fared
__device__ __forceinline__ void box_status(i32* status, u64 b, bool in_table, bool first_lane) {
    if (first_lane) status[b] = in_table ? ZCG_OK : ZCG_ERR_INVALID_INPUT;
}

// Short box rows: work unit = (box, tile of RG_T 16-byte pieces), one
// workgroup per unit (region_kernel's walk).
__global__ __launch_bounds__(RG_T) void regions_kernel(RegionsArgs a, const u8* const* __restrict__ table,
                                                       const zcg_box* __restrict__ boxes,
                                                       i32* __restrict__ status) {
    const u64 tile_elems = (u64)RG_T * a.V;
    const u64 fv = fill_pattern(a.fillv, a.es);
    const u32x4 fill16 = {(u32)fv, (u32)(fv >> 32), (u32)fv, (u32)(fv >> 32)};
    const u64 nunits = (u64)a.nboxes * a.upb;
    for (u64 unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const u64 b = unit / a.upb;
        const u64 tile = unit - b * a.upb;
        const BoxTerms t = box_terms(a, table, boxes, b);
        box_status(status, b, t.in_table, tile == 0 && threadIdx.x == 0);
        if (!t.in_table) continue;
        // decompose the tile start (workgroup-uniform, scalar)
        Pos p;
        u64 e = tile * tile_elems;
#pragma unroll
        for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
            if (k < a.nd) {
                const u64 q = e / a.bs[k];
                p.x[k] = (u32)(e - q * a.bs[k]);
                e = q;
            } else {
                p.x[k] = 0;
            }
        }
        const u64 e0 = tile * tile_elems + (u64)threadIdx.x * a.V;
        if (e0 >= a.total) continue;
        boxes_advance(a, p, threadIdx.x * a.V);
        u32 rem = (u32)((a.total - e0) < a.V ? (a.total - e0) : a.V);
        u32 run;
        const u8* src = boxes_src(a, t, p, &run);
        if (rem == a.V && run >= a.V && a.ostr[0] == 1) {  // one 16-byte piece, both sides contiguous
            u8* d = t.out + boxes_dst(a, p) * (i64)a.es;
            if (src) st16(d, ld16(src));
            else if (a.fill) st16(d, fill16);
            continue;
        }
        while (rem) {  // runs inside one chunk row and one box row
            const u32 k = run < rem ? run : rem;
            u8* d = t.out + boxes_dst(a, p) * (i64)a.es;
            const i64 ds = a.ostr[0] * (i64)a.es;
            for (u32 j = 0; j < k; j++) {
                if (src) copy_elem(d + j * ds, src + (u64)j * a.es, a.es);
                else if (a.fill) fill_elem(d + j * ds, fv, a.es);
            }
            rem -= k;
            if (!rem) break;
            boxes_advance(a, p, k);
            src = boxes_src(a, t, p, &run);
        }
    }
}

// Long box rows: work unit = (box, row, piece of U*64*V elements of it), one
// wave per unit (region_rows_kernel's walk).  The box terms and the row's
// slow-dimension contributions are scalar; lanes stream the piece 16 bytes each.
__global__ __launch_bounds__(RG_T) void regions_rows_kernel(RegionsArgs a, const u8* const* __restrict__ table,
                                                            const zcg_box* __restrict__ boxes,
                                                            i32* __restrict__ status) {
    const u32 lane = threadIdx.x & 63;
    const u64 wid = ((u64)blockIdx.x * RG_T + threadIdx.x) >> 6;
    const u64 nwaves = ((u64)gridDim.x * RG_T) >> 6;
    const u64 fv = fill_pattern(a.fillv, a.es);
    const u32x4 fill16 = {(u32)fv, (u32)(fv >> 32), (u32)fv, (u32)(fv >> 32)};
    const u32 V = a.V, bs0 = a.bs[0], cs0 = a.cs[0];
    const i64 es = a.es;
    constexpr u32 U = ZCG_RG_U;
    const u32 span = U * 64 * V;
    const u32 ppr = (u32)(((u64)bs0 + span - 1) / span);
    const u64 nunits = (u64)a.nboxes * a.upb;
    for (u64 unit = ru64(wid); unit < nunits; unit += nwaves) {
        const u64 b = unit / a.upb;
        const u64 ub = unit - b * a.upb;
        const BoxTerms t = box_terms(a, table, boxes, b);
        box_status(status, b, t.in_table, ub == 0 && lane == 0);
        if (!t.in_table) continue;
        const u64 row = ub / ppr;
        const u32 piece = (u32)(ub - row * ppr);
        const u32 orr0 = t.orr[0];
        // slow-dimension coordinates of this row (scalar)
        u64 e = row, ti = 0, wi = 0;
        i64 drow = 0;
        bool ok = true;
#pragma unroll
        for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
            if (k >= a.nd) break;
            const u64 qd = e / a.bs[k];
            const u32 x = (u32)(e - qd * a.bs[k]);
            e = qd;
            const u32 r = t.orr[k] + x;
            const u32 q = r / a.cs[k];
            ok &= q < t.gn[k];
            ti += (u64)q * a.tstr[k];
            wi += (u64)(r - q * a.cs[k]) * a.cstr[k];
            drow += (i64)x * a.ostr[k];
        }
        u8* drow_p = t.out + drow * es;
        // U pieces per lane in flight: loads first, then stores
        const u64 xb = (u64)piece * span + lane * V;
        u32x4 v[U];
        u8* dp[U];
        u32 mode[U];  // 0 skip, 1 load+store, 2 fill, 3 element runs
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            const u64 xu = xb + (u64)u * 64 * V;
            mode[u] = 0;
            if (xu >= bs0) continue;
            const u32 x0 = (u32)xu;
            dp[u] = drow_p + (i64)x0 * a.ostr[0] * es;
            const u32 r = orr0 + x0;
            const u32 q = r / cs0;
            const u32 w0 = r - q * cs0;
            const bool here = ok && q < t.gn[0];
            const u8* base = here ? t.table[ti + (u64)q * a.tstr[0]] : nullptr;
            if (!(bs0 - x0 >= V && w0 + V <= cs0 && a.ostr[0] == 1)) { mode[u] = 3; continue; }
            if (base) { v[u] = ld16(base + (wi + w0) * (u64)es); mode[u] = 1; }
            else if (a.fill) { v[u] = fill16; mode[u] = 2; }
        }
#pragma unroll
        for (u32 u = 0; u < U; u++)
            if (mode[u] == 1 || mode[u] == 2) st16(dp[u], v[u]);
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            if (mode[u] != 3) continue;
            const u32 x0 = (u32)(xb + (u64)u * 64 * V);
            const u32 rem = bs0 - x0 < V ? bs0 - x0 : V;
            // the piece crosses a chunk boundary or ends the row: per element
            for (u32 j = 0; j < rem; j++) {
                const u32 rj = orr0 + x0 + j;
                const u32 qj = rj / cs0;
                const bool hj = ok && qj < t.gn[0];
                const u8* bj = hj ? t.table[ti + (u64)qj * a.tstr[0]] : nullptr;
                u8* dj = drow_p + (i64)(x0 + j) * a.ostr[0] * es;
                if (bj) copy_elem(dj, bj + (wi + (rj - qj * cs0)) * (u64)es, a.es);
                else if (a.fill) fill_elem(dj, fv, a.es);
            }
        }
    }
}

}  // namespace

// The launch rule is launch_region's: rows of at least 32 16-byte pieces go a
// wave per row piece, shorter ones a workgroup per tile.  One launch whatever
// the number of boxes (the grid is capped; workgroups stride over the units).
hipError_t launch_regions(const RegionsArgs& a0, const void* const* d_table, const zcg_box* d_boxes,
                          int32_t* d_status, hipStream_t s) {
    RegionsArgs a = a0;
    if (a.total == 0 || a.nboxes == 0) return hipSuccess;
    if (a.bs[0] >= 32u * a.V) {
        a.nrows = a.total / a.bs[0];
        const u64 span = (u64)ZCG_RG_U * 64 * a.V;
        a.upb = a.nrows * ((a.bs[0] + span - 1) / span);
        const u64 units = a.upb * a.nboxes;
        const u64 wgs = (units + 3) / 4;
        const u32 grid = (u32)(wgs < (1u << 20) ? wgs : (1u << 20));
        hipLaunchKernelGGL(regions_rows_kernel, dim3(grid), dim3(RG_T), 0, s, a, (const u8* const*)d_table, d_boxes,
                           d_status);
        return hipGetLastError();
    }
    a.nrows = 0;
    a.upb = (a.total + (u64)RG_T * a.V - 1) / ((u64)RG_T * a.V);
    const u64 units = a.upb * a.nboxes;
    const u32 grid = (u32)(units < 262144 ? units : 262144);
    hipLaunchKernelGGL(regions_kernel, dim3(grid), dim3(RG_T), 0, s, a, (const u8* const*)d_table, d_boxes, d_status);
    return hipGetLastError();
}

}  // namespace zcg
