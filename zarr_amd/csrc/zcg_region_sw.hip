// zcg_region_sw.hip — region scatter for many boxes that each have their own
// sample count, view and a step per dimension (zcg_write_regions_s): sample i
// of a box along dimension d goes to array index offset[d] + i*step[d], and no
// other byte of a chunk slot is written.  The reference's write_ndarray
// (ndarray.rs:276-385) takes dense boxes only; a caller who wants
// a[o::k] = x reads the hull, overlays the samples and writes the hull back.
// The box terms and the plan are the read side's (zcg_region_sbox.h, the plan
// kernel of zcg_region_s.hip with fill off); the walk is zcg_region_walk_sw.h's.
// The kernel lives in a translation unit of its own, so the code objects of
// the other region kernels do not change with it.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"
#include "zcg_region_sbox.h"
#include "zcg_region_walk_sw.h"

namespace zcg {

namespace {

__global__ __launch_bounds__(RG_T) void regions_sw_kernel(RegionWalk w, BoxTable bt,
                                                          const u8* const* __restrict__ table,
                                                          const zcg_sbox* __restrict__ boxes,
                                                          const u64* __restrict__ prefix) {
    const u64 n = bt.nboxes;
    const u64 all = ru64(prefix[n]);
    const u64 per = (all + gridDim.x - 1) / gridDim.x;
    u64 unit = (u64)blockIdx.x * per;
    const u64 last = unit + per < all ? unit + per : all;
    if (unit >= last) return;
    // the box of the first unit: prefix[b] <= unit < prefix[b + 1]
    u64 b = 0, hi = n;
    while (hi - b > 1) {
        const u64 mid = (b + hi) >> 1;
        if (ru64(prefix[mid]) <= unit) b = mid;
        else hi = mid;
    }
    const u32 wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // any readable, 8-byte aligned device address: where a sample that has no
    // chunk points its table load (the pointer loads stay unconditional)
    const u8* safe = (const u8*)boxes;
    while (unit < last) {
        u64 pe;
        while ((pe = ru64(prefix[b + 1])) <= unit) b++;  // prefix[n] = all > unit ends it
        const u64 pb = ru64(prefix[b]);
        RegionWalk wb;
        BoxTerms t;
        Steps st;
        sbox_terms<true>(w, bt, table, boxes, b, wb, t, st);
        const u64 end = pe < last ? pe : last;
        if (sbox_rows(wb)) {
            const u32 ppr = row_pieces(wb);
            const u64 nwu = sbox_row_units(wb);
            for (; unit < end; unit++) {
                const u64 wu = (unit - pb) * RS_WAVES + wv;
                if (wu >= nwu) continue;
                const u64 row = wu / ppr;
                if (st.st[0] == 1) scatter_row_piece_s(wb, t, st, row, (u32)(wu - row * ppr));
                else scatter_row_piece(wb, t, st, row, (u32)(wu - row * ppr));
            }
        } else if (st.st[0] == 1) {
            for (; unit < end; unit++) scatter_tile_s(wb, t, st, unit - pb);
        } else {
            for (; unit < end; unit++) scatter_tile(wb, t, st, unit - pb, safe);
        }
    }
}

}  // namespace

// launch_regions_s's shape: the plan (fill off, so a box that visits no chunk
// has no unit), and the walk on a grid sized from the bound.
hipError_t launch_regions_sw(const RegionWalk& w, const BoxTable& bt, void* const* d_table, const zcg_sbox* d_boxes,
                             void* d_prefix, int32_t* d_status, hipStream_t s) {
    if (bt.nboxes == 0) return hipSuccess;
    hipError_t e = launch_regions_s_plan(w, bt, (const void* const*)d_table, d_boxes, d_prefix, d_status, s);
    if (e != hipSuccess || w.total == 0) return e;  // a zero extent in the bound: no box has work
    const u64 per_box = (w.total + (u64)RG_T * w.V - 1) / ((u64)RG_T * w.V);
    const u64 units = per_box * bt.nboxes;
    hipLaunchKernelGGL(regions_sw_kernel, dim3((u32)(units < RS_GRID ? units : RS_GRID)), dim3(RG_T), 0, s, w, bt,
                       (const u8* const*)d_table, d_boxes, (const u64*)d_prefix);
    return hipGetLastError();
}

}  // namespace zcg
