// zcg_region_sw.hip — region scatter for many boxes that each have their own
// sample count, view and a step per dimension (zcg_write_regions_s): sample i
// of a box along dimension d goes to array index offset[d] + i*step[d], and no
// other byte of a chunk slot is written.  The reference's write_ndarray
// (ndarray.rs:276-385) takes dense boxes only; a caller who wants
// a[o::k] = x reads the hull, overlays the samples and writes the hull back.
// The box terms and the unit loop are zcg_region_plan.h's, the plan is the
// read side's (the plan kernel of zcg_region_s.hip with fill off); a box with
// fast step 1 goes through the dense walk in its write direction
// (zcg_region_walk.h), any other through the scatter (zcg_region_walk_sw.h).
// The kernel lives in a translation unit of its own.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"
#include "zcg_region_walk_sw.h"
#include "zcg_region_plan.h"

namespace zcg {

namespace {

__global__ __launch_bounds__(RG_T) void regions_sw_kernel(RegionWalk w, BoxTable bt,
                                                          const u8* const* __restrict__ table,
                                                          const zcg_sbox* __restrict__ boxes,
                                                          const u64* __restrict__ prefix) {
    // any readable, 8-byte aligned device address: where a sample that has no
    // chunk points its table load (the pointer loads stay unconditional)
    const u8* safe = (const u8*)boxes;
    walk_units(
        bt.nboxes, prefix,
        [&](u64 b) {
            WalkBox<Steps> x;
            sbox_terms<true>(w, bt, table, boxes, b, x.w, x.t, x.s);
            return x;
        },
        [safe](const WalkBox<Steps>& x, bool rows, u64 at, u32 piece) {
            if (x.s.st[0] == 1) {
                if (rows) walk_row_piece<ZCG_MAX_DIMS>(x.w, x.t, x.s, at, piece, 1);
                else walk_tile(x.w, x.t, x.s, at, 1);
            } else if (rows) {
                scatter_row_piece(x.w, x.t, x.s, at, piece);
            } else {
                scatter_tile(x.w, x.t, x.s, at, safe);
            }
        });
}

}  // namespace

// launch_regions_s's shape: the plan (fill off, so a box that visits no chunk
// has no unit), and the walk on a grid sized from the bound.
hipError_t launch_regions_sw(const RegionWalk& w, const BoxTable& bt, void* const* d_table, const zcg_sbox* d_boxes,
                             void* d_prefix, int32_t* d_status, hipStream_t s) {
    if (bt.nboxes == 0) return hipSuccess;
    hipError_t e = launch_regions_s_plan(w, bt, (const void* const*)d_table, d_boxes, d_prefix, d_status, s);
    if (e != hipSuccess || w.total == 0) return e;  // a zero extent in the bound: no box has work
    hipLaunchKernelGGL(regions_sw_kernel, dim3(walk_grid(w, bt.nboxes)), dim3(RG_T), 0, s, w, bt,
                       (const u8* const*)d_table, d_boxes, (const u64*)d_prefix);
    return hipGetLastError();
}

}  // namespace zcg
