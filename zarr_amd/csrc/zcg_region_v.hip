// zcg_region_v.hip — region assembly and scatter for many boxes that each have
// their own shape and view (zcg_read_regions_v, zcg_write_regions_v): the
// reference's read_ndarray / write_ndarray (ndarray.rs:153-385) take any
// BoundingBox per call.  The walk is zcg_region_walk.h's, the constants and
// the unit counts zcg_region_plan.h's, the per-box semantics are those of
// zcg_region.hip's kernels.  The kernels live in a translation unit of their
// own, so the code object that holds zcg_region.hip's kernels does not change
// with them.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_plan.h"

namespace zcg {

namespace {

struct VBoxFate {
    bool ok;      // inside the bound, and its grid range inside the table (or it has no element or visits no chunk)
    bool visits;  // it visits a chunk
};

// The terms of box b: box_terms with the box's own extent, plus the walk's
// per-box part (wb.bs, wb.total, wb.ostr).  UNI: b is wave-uniform and the
// terms go to the scalar side; else every lane has its own box (plan kernel).
// Positions are held in 32 bits only for a box inside the bound w.bs; the
// terms of any other box are not used.
template <bool UNI>
__device__ __forceinline__ VBoxFate vbox_terms(const RegionWalk& w, const BoxTable& bt,
                                               const u8* const* __restrict__ table,
                                               const zcg_vbox* __restrict__ boxes, u64 b, RegionWalk& wb,
                                               BoxTerms& t) {
    const zcg_vbox* bx = boxes + b;
    wb = w;
    u64 base = 0, total = 1;
    bool inside = true, visits = true, bounded = true;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        t.orr[k] = 0;
        t.gn[k] = 0;
        wb.bs[k] = 0;
        wb.ostr[k] = 0;
        if (k >= w.nd) continue;
        const u32 d = bt.dim[k];
        const u64 off = uni<UNI>(bx->offset[d]);
        const u64 ext = uni<UNI>(bx->shape[d]);
        bounded &= ext <= w.bs[k];
        // zcg_region_grid's range of this box (see box_terms)
        const u64 cs = w.cs[k];
        const u64 lo = off / cs;
        const u64 orr = off - lo * cs;
        const u64 end = off + ext < bt.as[k] ? off + ext : bt.as[k];
        const u64 s = end > off ? end - off : 0;
        const u32 span = (u32)orr + (u32)s, nq = span / w.cs[k];
        const u32 n = nq + (span != nq * w.cs[k] ? 1u : 0u);
        t.orr[k] = (u32)orr;
        t.gn[k] = n;
        visits &= n != 0;
        inside &= lo >= bt.tlo[k] && lo - bt.tlo[k] + n <= bt.tn[k];
        base += (lo - bt.tlo[k]) * w.tstr[k];
        wb.bs[k] = (u32)ext;
        wb.ostr[k] = (i64)uni<UNI>((u64)bx->strides[d]);
        total *= ext;
    }
    wb.total = total;
    t.table = table + (visits && inside ? base : 0);
    t.out = (u8*)(uintptr_t)uni<UNI>((u64)(uintptr_t)bx->base);
    // a box with a zero extent has no element to place: it is in order wherever the table is
    return VBoxFate{bounded && (inside || !visits || total == 0), visits};
}

// The plan: status[b] and prefix[b] = work units of the boxes before b, for
// every box; prefix[nboxes] = all units.  A box has no unit when it is
// refused, has a zero extent, or visits no chunk and is not to be filled.  One
// workgroup walks the boxes RP_PLAN_T at a time (a lane per box) and carries
// the running sum.  regions_s_plan_kernel (zcg_region_s.hip) repeats the scan
// with its own terms: as a shared function it costs this kernel two waves per
// SIMD of occupancy.
__global__ __launch_bounds__(RP_PLAN_T) void regions_v_plan_kernel(RegionWalk w, BoxTable bt,
                                                                   const u8* const* __restrict__ table,
                                                                   const zcg_vbox* __restrict__ boxes,
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
            const VBoxFate f = vbox_terms<false>(w, bt, table, boxes, b, wb, t);
            status[b] = f.ok ? ZCG_OK : ZCG_ERR_INVALID_INPUT;
            if (f.ok && wb.total && (f.visits || w.fill)) units = box_units(wb);
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

// The walk.  The unit loop is walk_units' (zcg_region_plan.h) in its own
// lines: through the shared function this kernel's instructions change, and
// the skew rows of tools/boxes_v_bench.py then miss the A/B rule (DESIGN.md
// §6.7f).
template <u32 DIR>
__global__ __launch_bounds__(RG_T) void regions_v_kernel(RegionWalk w, BoxTable bt,
                                                         const u8* const* __restrict__ table,
                                                         const zcg_vbox* __restrict__ boxes,
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
    while (unit < last) {
        u64 pe;
        while ((pe = ru64(prefix[b + 1])) <= unit) b++;  // prefix[n] = all > unit ends it
        const u64 pb = ru64(prefix[b]);
        RegionWalk wb;
        BoxTerms t;
        vbox_terms<true>(w, bt, table, boxes, b, wb, t);
        const u64 end = pe < last ? pe : last;
        if (box_rows(wb)) {
            const u32 ppr = row_pieces(wb);
            const u64 nwu = box_row_units(wb);
            for (; unit < end; unit++) {
                const u64 wu = (unit - pb) * RP_WAVES + wv;
                if (wu >= nwu) continue;
                const u64 row = wu / ppr;
                walk_row_piece<ZCG_MAX_DIMS>(wb, t, Dense{}, row, (u32)(wu - row * ppr), DIR);
            }
        } else {
            for (; unit < end; unit++) walk_tile(wb, t, Dense{}, unit - pb, DIR);
        }
    }
}

}  // namespace

uint64_t regions_v_prefix_bytes(uint32_t nboxes) { return ((u64)nboxes + 1) * sizeof(u64); }

// Two launches whatever the boxes: the plan, and the walk on a grid sized from
// the bound (the host does not know the boxes; any grid is correct, since
// workgroups divide the units the plan counted among themselves).
hipError_t launch_regions_v(const RegionWalk& w, const BoxTable& bt, const void* const* d_table,
                            const zcg_vbox* d_boxes, void* d_prefix, int32_t* d_status, uint32_t dir,
                            hipStream_t s) {
    if (bt.nboxes == 0) return hipSuccess;
    hipLaunchKernelGGL(regions_v_plan_kernel, dim3(1), dim3(RP_PLAN_T), 0, s, w, bt, (const u8* const*)d_table,
                       d_boxes, (u64*)d_prefix, d_status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || w.total == 0) return e;  // a zero extent in the bound: no box has work
    hipLaunchKernelGGL(dir ? regions_v_kernel<1> : regions_v_kernel<0>, dim3(walk_grid(w, bt.nboxes)), dim3(RG_T), 0,
                       s, w, bt, (const u8* const*)d_table, d_boxes, (const u64*)d_prefix);
    return hipGetLastError();
}

}  // namespace zcg
