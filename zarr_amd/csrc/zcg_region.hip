// zcg_region.hip — region assembly on the device:
// ZarrNdarrayReader::read_ndarray / read_ndarray_into_with_buffer
// (src/ndarray.rs:153-268) for chunks that the batch decoders already left in
// HBM, for one bounding box per launch (zcg_read_region, zcg_write_region) or
// many boxes of one common shape, each at its own offset and into its own
// output view, from one shared chunk table (zcg_read_regions), or scattered
// into it from its own input view (zcg_write_regions; the slot prefill of
// chunks the store lacks is here too).  Boxes that each have their own shape
// and view (zcg_read_regions_v, zcg_write_regions_v) are zcg_region_v.hip's.
//
// Reference semantics kept: the chunks visited are bounded_coord_iter's grid
// range (ndarray.rs:410-432); each visited chunk covers its full nominal
// bounds, overhang included (get_chunk_bounds, ndarray.rs:434-446), so an
// element at global position g comes from chunk g / chunk_shape, at the
// chunk-local position g % chunk_shape in the chunk's memory order
// (as_ndarray, ndarray.rs:453-476: ColumnMajor = dim 0 fastest); elements no
// visited chunk covers keep Array::from_elem's fill value in read_ndarray
// (ndarray.rs:164-171) and are left untouched by read_ndarray_into.
//
// The kernels are HBM-bound byte movement (2 bytes of traffic per output
// byte).  The walk itself is zcg_region_walk.h's; the four entry points differ
// only in how they obtain a box's terms.  The single-box ones get them from
// the host as kernel arguments (scalar).  The many-box ones work on the
// flattened (box, tile) or (box, row piece) space: the box of a work unit is
// wave-uniform, so everything that depends on the box alone — offset mod chunk
// extent, the box's grid range, its base index in the shared table, whether
// that range lies in the table — is computed once per work unit from
// d_boxes[b].offset on the scalar side.  Per box the semantics are the single
// call's: a box behaves exactly as a zcg_read_region call with its offset and
// a table over its own grid range would.  The shared table only supplies the
// pointers; a chunk of the table outside the box's own grid range is never
// read.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"

namespace zcg {

namespace {

// the terms of box b of a many-box call; false: the box's grid range does not
// lie inside the table's
__device__ __forceinline__ bool box_terms(const RegionWalk& w, const BoxTable& bt,
                                          const u8* const* __restrict__ table,
                                          const zcg_box* __restrict__ boxes, u64 b, BoxTerms& t) {
    const zcg_box* bx = boxes + b;
    u64 base = 0;
    bool inside = true, visits = true;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        t.orr[k] = 0;
        t.gn[k] = 0;
        if (k >= w.nd) continue;
        // bounded_coord_iter (ndarray.rs:410-432), as zcg_region_grid states it:
        // the box clipped to the array, floor / ceil by the chunk extent
        const u64 off = ru64(bx->offset[bt.dim[k]]);
        const u64 cs = w.cs[k];
        const u64 lo = off / cs;
        const u64 orr = off - lo * cs;
        const u64 end = off + w.bs[k] < bt.as[k] ? off + w.bs[k] : bt.as[k];
        const u64 s = end > off ? end - off : 0;
        // ceil((off + s) / cs) - lo, in 32 bits: orr + s <= chunk extent - 1 +
        // box extent < 2^32 (checked by the host)
        const u32 span = (u32)orr + (u32)s, nq = span / w.cs[k];
        const u32 n = nq + (span != nq * w.cs[k] ? 1u : 0u);
        t.orr[k] = (u32)orr;
        t.gn[k] = n;
        visits &= n != 0;
        inside &= lo >= bt.tlo[k] && lo - bt.tlo[k] + n <= bt.tn[k];
        base += (lo - bt.tlo[k]) * w.tstr[k];
    }
    t.table = table + (visits && inside ? base : 0);
    t.out = (u8*)(uintptr_t)ru64((u64)(uintptr_t)bx->out);
    // a box that visits no chunk reads no table entry: it is filled (or left
    // untouched) wherever the table is
    return inside || !visits;
}

// one lane says how the box fared
__device__ __forceinline__ void box_status(i32* status, u64 b, bool in_table, bool first_lane) {
    if (first_lane) status[b] = in_table ? ZCG_OK : ZCG_ERR_INVALID_INPUT;
}

// Short box rows: a workgroup per tile (walk_tile).
__global__ __launch_bounds__(RG_T) void region_kernel(RegionWalk w, BoxTerms t, u64 ntiles, u32 dir) {
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) walk_tile(w, t, Dense{}, tile, dir);
}

// Long box rows: a wave per (row, row piece) (walk_row_piece).
__global__ __launch_bounds__(RG_T) void region_rows_kernel(RegionWalk w, BoxTerms t, u64 nunits, u32 dir) {
    const u64 wid = ((u64)blockIdx.x * RG_T + threadIdx.x) >> 6;
    const u64 nwaves = ((u64)gridDim.x * RG_T) >> 6;
    const u32 ppr = row_pieces(w);
    for (u64 unit = ru64(wid); unit < nunits; unit += nwaves) {
        const u64 row = unit / ppr;
        walk_row_piece<1>(w, t, Dense{}, row, (u32)(unit - row * ppr), dir);
    }
}

// Many boxes, short rows: a workgroup per (box, tile).  DIR is the walk's
// direction, fixed at compile time: the read kernels carry no trace of the
// write direction.
template <u32 DIR>
__global__ __launch_bounds__(RG_T) void regions_kernel(RegionWalk w, BoxTable bt, const u8* const* __restrict__ table,
                                                       const zcg_box* __restrict__ boxes,
                                                       i32* __restrict__ status) {
    const u64 nunits = (u64)bt.nboxes * bt.upb;
    for (u64 unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const u64 b = unit / bt.upb;
        const u64 tile = unit - b * bt.upb;
        BoxTerms t;
        const bool in_table = box_terms(w, bt, table, boxes, b, t);
        box_status(status, b, in_table, tile == 0 && threadIdx.x == 0);
        if (in_table) walk_tile(w, t, Dense{}, tile, DIR);
    }
}

// Many boxes, long rows: a wave per (box, row, row piece).
template <u32 DIR>
__global__ __launch_bounds__(RG_T) void regions_rows_kernel(RegionWalk w, BoxTable bt,
                                                            const u8* const* __restrict__ table,
                                                            const zcg_box* __restrict__ boxes,
                                                            i32* __restrict__ status) {
    const u64 wid = ((u64)blockIdx.x * RG_T + threadIdx.x) >> 6;
    const u64 nwaves = ((u64)gridDim.x * RG_T) >> 6;
    const u32 ppr = row_pieces(w);
    const u64 nunits = (u64)bt.nboxes * bt.upb;
    for (u64 unit = ru64(wid); unit < nunits; unit += nwaves) {
        const u64 b = unit / bt.upb;
        const u64 ub = unit - b * bt.upb;
        BoxTerms t;
        const bool in_table = box_terms(w, bt, table, boxes, b, t);
        box_status(status, b, in_table, ub == 0 && (threadIdx.x & 63) == 0);
        if (!in_table) continue;
        const u64 row = ub / ppr;
        walk_row_piece<ZCG_MAX_DIMS>(w, t, Dense{}, row, (u32)(ub - row * ppr), DIR);
    }
}

// Slot prefill (write_ndarray's chunk that is absent from the store and only
// partly covered, ndarray.rs:351-364): m slots of D bytes, each all fill
// element.  Slots are packed D apart and D is any multiple of the element
// size, so a slot starts at an element boundary but mostly not at a 16-byte
// one.  A slot is cut into a head up to the first 16-byte boundary (element
// stores), aligned 16-byte pieces, and a tail below 16 bytes (element stores);
// the head is a whole number of elements, so every aligned piece holds the
// element pattern in phase.  A workgroup per (slot, run of RG_T pieces); piece
// numbers nb and nb + 1 stand for the head and the tail.  No byte outside
// [slot, slot + D) is written.
__global__ __launch_bounds__(RG_T) void slot_fill_kernel(u8* const* __restrict__ slots, u32 m, u64 D, u32 es,
                                                         u64 fillv, u32 per) {
    const u32x4 f16 = fill_piece(fillv, es);
    const u64 nunits = (u64)m * per;
    for (u64 unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const u64 sl = unit / per;
        u8* p = (u8*)(uintptr_t)ru64((u64)(uintptr_t)slots[sl]);
        const u64 to16 = (16 - ((u64)(uintptr_t)p & 15)) & 15;
        const u64 head = to16 < D ? to16 : D;
        const u64 nb = (D - head) >> 4;
        const u64 i = (unit - sl * per) * RG_T + threadIdx.x;
        if (i < nb) {
            *(u32x4*)(p + head + (i << 4)) = f16;
        } else if (i == nb) {
            for (u64 o = 0; o < head; o += es) fill_elem(p + o, fillv, es);
        } else if (i == nb + 1) {
            for (u64 o = head + (nb << 4); o < D; o += es) fill_elem(p + o, fillv, es);
        }
    }
}

// The launch rule: rows of at least 32 16-byte pieces go a wave per row piece,
// shorter ones a workgroup per tile.  One launch whatever the number of boxes
// (the grid is capped; workgroups stride over the units).
struct LaunchShape {
    bool rows;
    u64 upb;   // work units per box
    u32 grid;
};
LaunchShape launch_shape(const RegionWalk& w, u64 nboxes) {
    LaunchShape g;
    g.rows = w.bs[0] >= 32u * w.V;
    if (g.rows) {
        g.upb = w.total / w.bs[0] * row_pieces(w);
        const u64 wgs = (g.upb * nboxes + 3) / 4;
        g.grid = (u32)(wgs < (1u << 20) ? wgs : (1u << 20));
    } else {
        g.upb = (w.total + (u64)RG_T * w.V - 1) / ((u64)RG_T * w.V);
        const u64 units = g.upb * nboxes;
        g.grid = (u32)(units < 262144 ? units : 262144);
    }
    return g;
}

}  // namespace

hipError_t launch_region(const RegionWalk& w, const BoxTerms& t, uint32_t dir, hipStream_t s) {
    if (w.total == 0) return hipSuccess;
    const LaunchShape g = launch_shape(w, 1);
    hipLaunchKernelGGL(g.rows ? region_rows_kernel : region_kernel, dim3(g.grid), dim3(RG_T), 0, s, w, t, g.upb, dir);
    return hipGetLastError();
}

hipError_t launch_regions(const RegionWalk& w, const BoxTable& bt0, const void* const* d_table,
                          const zcg_box* d_boxes, int32_t* d_status, uint32_t dir, hipStream_t s) {
    if (w.total == 0 || bt0.nboxes == 0) return hipSuccess;
    const LaunchShape g = launch_shape(w, bt0.nboxes);
    BoxTable bt = bt0;
    bt.upb = g.upb;
    auto kernel = g.rows ? (dir ? regions_rows_kernel<1> : regions_rows_kernel<0>)
                         : (dir ? regions_kernel<1> : regions_kernel<0>);
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(RG_T), 0, s, w, bt, (const u8* const*)d_table, d_boxes, d_status);
    return hipGetLastError();
}

hipError_t launch_slot_fill(void* const* d_slots, uint32_t m, uint64_t D, uint32_t es, uint64_t fillv,
                            hipStream_t s) {
    if (m == 0 || D == 0) return hipSuccess;
    if (!(es == 1 || es == 2 || es == 4 || es == 8) || D % es) return hipErrorInvalidValue;
    const u64 per = ((D >> 4) + 2 + RG_T - 1) / RG_T;
    if (per >= (1ull << 32)) return hipErrorInvalidValue;
    const u64 units = per * m;
    hipLaunchKernelGGL(slot_fill_kernel, dim3((u32)(units < 262144 ? units : 262144)), dim3(RG_T), 0, s,
                       (u8* const*)d_slots, m, D, es, fillv, (u32)per);
    return hipGetLastError();
}

const char* cfg_region() { return "region:U=" ZCG_STR(ZCG_RG_U); }

}  // namespace zcg
