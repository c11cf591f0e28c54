// zcg_region_s.hip — region assembly for many boxes that each have their own
// sample count, view and a step per dimension (zcg_read_regions_s): sample i of
// a box along dimension d is array index offset[d] + i*step[d].  The reference
// hard-codes step 1 in its slices (ndarray.rs:118-127); a caller who wants
// every k-th element reads the dense hull and slices it.  Per box the values
// are those zcg_read_region writes to element i*step of a dense view of the
// hull.  The box terms, the plan / prefix scheme and the unit loop are
// zcg_region_plan.h's; a box with fast step 1 goes through the dense walk
// (zcg_region_walk.h), any other through the gather (zcg_region_walk_s.h).
// The kernels live in a translation unit of their own.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"
#include "zcg_region_plan.h"

namespace zcg {

namespace {

// The plan: regions_v_plan_kernel's (zcg_region_v.hip), with sbox_terms and
// work counted in output elements.
__global__ __launch_bounds__(RP_PLAN_T) void regions_s_plan_kernel(RegionWalk w, BoxTable bt,
                                                                   const u8* const* __restrict__ table,
                                                                   const zcg_sbox* __restrict__ boxes,
                                                                   u64* __restrict__ prefix,
                                                                   i32* __restrict__ status) {
    __shared__ u64 wsum[RP_PLAN_T / 64];
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 carry = 0;
    for (u64 b0 = 0; b0 < bt.nboxes; b0 += RP_PLAN_T) {
        const u64 b = b0 + threadIdx.x;
        u64 units = 0;
        if (b < bt.nboxes) {
            RegionWalk wb;
            BoxTerms t;
            Steps st;
            const SBoxFate f = sbox_terms<false>(w, bt, table, boxes, b, wb, t, st);
            status[b] = f.status;
            if (f.status == ZCG_OK && wb.total && (f.visits || w.fill)) units = box_units(wb);
        }
        u64 x = units;  // inclusive scan over the wave
#pragma unroll
        for (u32 o = 1; o < 64; o <<= 1) {
            const u64 y = __shfl_up((unsigned long long)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        u64 before = carry, all = 0;
#pragma unroll
        for (u32 i = 0; i < RP_PLAN_T / 64; i++) {
            if (i < wv) before += wsum[i];
            all += wsum[i];
        }
        if (b < bt.nboxes) prefix[b] = before + x - units;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[bt.nboxes] = carry;
}

__global__ __launch_bounds__(RG_T) void regions_s_kernel(RegionWalk w, BoxTable bt,
                                                         const u8* const* __restrict__ table,
                                                         const zcg_sbox* __restrict__ boxes,
                                                         const u64* __restrict__ prefix) {
    // any readable, 8-byte aligned device address: where a sample that has no
    // source points its load (the gather keeps every load unconditional)
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
                if (rows) walk_row_piece<ZCG_MAX_DIMS>(x.w, x.t, x.s, at, piece, 0);
                else walk_tile(x.w, x.t, x.s, at, 0);
            } else if (rows) {
                gather_row_piece(x.w, x.t, x.s, at, piece, safe);
            } else {
                gather_tile(x.w, x.t, x.s, at, safe);
            }
        });
}

}  // namespace

// The plan alone: every box's status word and the prefix sum of the work
// units.  With w.fill == 0 a box that visits no chunk has no unit, which is
// the scatter's rule too (zcg_region_sw.hip).
hipError_t launch_regions_s_plan(const RegionWalk& w, const BoxTable& bt, const void* const* d_table,
                                 const zcg_sbox* d_boxes, void* d_prefix, int32_t* d_status, hipStream_t s) {
    hipLaunchKernelGGL(regions_s_plan_kernel, dim3(1), dim3(RP_PLAN_T), 0, s, w, bt, (const u8* const*)d_table,
                       d_boxes, (u64*)d_prefix, d_status);
    return hipGetLastError();
}

// Two launches whatever the boxes (launch_regions_v's shape): the plan, and
// the walk on a grid sized from the bound of the sample counts.
hipError_t launch_regions_s(const RegionWalk& w, const BoxTable& bt, const void* const* d_table,
                            const zcg_sbox* d_boxes, void* d_prefix, int32_t* d_status, hipStream_t s) {
    if (bt.nboxes == 0) return hipSuccess;
    hipError_t e = launch_regions_s_plan(w, bt, d_table, d_boxes, d_prefix, d_status, s);
    if (e != hipSuccess || w.total == 0) return e;  // a zero extent in the bound: no box has work
    hipLaunchKernelGGL(regions_s_kernel, dim3(walk_grid(w, bt.nboxes)), dim3(RG_T), 0, s, w, bt,
                       (const u8* const*)d_table, d_boxes, (const u64*)d_prefix);
    return hipGetLastError();
}

}  // namespace zcg
