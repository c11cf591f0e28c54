// zcg_region_plan.h — what the kernels for boxes of differing sizes
// (zcg_region_v.hip, zcg_region_s.hip, zcg_region_sw.hip) share besides the
// walk: the plan / prefix scheme's constants and unit counts, the terms of a
// strided box with its grid range, and the unit loop of the two strided walk kernels.
//
// Work follows the sum of the boxes' sizes: a plan kernel checks every box,
// writes its status word and an exclusive prefix sum of the boxes' work units
// (box_units; the two plan kernels each hold the scan); the
// walk kernel's workgroups each take a consecutive run of units, find the box
// of the first one by a scalar binary search in the prefix array and step to
// the next box as the run crosses its end (walk_units; regions_v_kernel holds
// the same loop in its own lines).  A work unit is
// workgroup-sized whatever the box: one tile (walk_tile) of a box with short
// rows, or four consecutive row pieces (walk_row_piece, one per wave) of a box
// with long rows — launch_shape's rule, applied per box.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"

namespace zcg {

constexpr u32 RP_PLAN_T = 1024;      // threads of the plan kernel's one workgroup
constexpr u32 RP_WAVES = RG_T / 64;  // row pieces per work unit
constexpr u32 RP_GRID = 32768;       // cap of the walk's grid

// UNI: the value is wave-uniform and goes to the scalar side; else every lane
// has its own (plan kernels, a lane per box)
template <bool UNI>
__device__ __forceinline__ u64 uni(u64 x) { return UNI ? ru64(x) : x; }

// The grid range of a box, dimension by dimension: box_terms' lines
// (zcg_region.hip; the comments there say why they are right).  box_terms and
// vbox_terms (zcg_region_v.hip) keep their own, so that their kernels' code
// stays the parent's; written into sbox_terms instead, regions_sw_kernel goes
// from 124 to 135 VGPRs and from 4 to 3 waves per SIMD.
struct GridRange {
    u64 base = 0;        // index of the range's first chunk in the table
    bool inside = true;  // the range lies in the table's
    bool visits = true;  // the box visits a chunk

    // dimension k of a box from off to oe (not yet clipped to the array); sets t.orr[k], t.gn[k]
    __device__ __forceinline__ void dim(const RegionWalk& w, const BoxTable& bt, BoxTerms& t, u32 k, u64 off,
                                        u64 oe) {
        const u64 cs = w.cs[k];
        const u64 lo = off / cs;
        const u64 orr = off - lo * cs;
        const u64 end = oe < bt.as[k] ? oe : bt.as[k];
        const u64 s = end > off ? end - off : 0;
        const u32 span = (u32)orr + (u32)s, nq = span / w.cs[k];
        const u32 n = nq + (span != nq * w.cs[k] ? 1u : 0u);
        t.orr[k] = (u32)orr;
        t.gn[k] = n;
        visits &= n != 0;
        inside &= lo >= bt.tlo[k] && lo - bt.tlo[k] + n <= bt.tn[k];
        base += (lo - bt.tlo[k]) * w.tstr[k];
    }
};

struct SBoxFate {
    i32 status;   // ZCG_OK: the box is walked (if it has work)
    bool visits;  // its hull visits a chunk
};

// The terms of strided box b (zcg_sbox), for the assembly kernels of
// zcg_region_s.hip and the scatter kernel of zcg_region_sw.hip: vbox_terms
// (zcg_region_v.hip) over the box's hull, the box's sample counts in wb.bs /
// wb.total, and its steps in st.  The step of a dimension with fewer than two
// samples is never used and kept as 1.
template <bool UNI>
__device__ __forceinline__ SBoxFate sbox_terms(const RegionWalk& w, const BoxTable& bt,
                                               const u8* const* __restrict__ table,
                                               const zcg_sbox* __restrict__ boxes, u64 b, RegionWalk& wb,
                                               BoxTerms& t, Steps& st) {
    const zcg_sbox* bx = boxes + b;
    wb = w;
    GridRange g;
    u64 total = 1;
    bool bounded = true, stepped = true, near = true;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        t.orr[k] = 0;
        t.gn[k] = 0;
        wb.bs[k] = 0;
        wb.ostr[k] = 0;
        st.st[k] = 1;
        if (k >= w.nd) continue;
        const u32 d = bt.dim[k];
        const u64 off = uni<UNI>(bx->offset[d]);
        const u64 cnt = uni<UNI>(bx->shape[d]);
        const u64 step = uni<UNI>(bx->step[d]);
        stepped &= step != 0;
        bounded &= cnt <= w.bs[k];
        // the hull's extent: (cnt - 1) * step + 1.  cnt <= the bound < 2^32 for a
        // box that is walked, so the product is exact once step < 2^32
        const bool wide = cnt > 1 && step >= (1ull << 32);
        const u64 c1 = cnt > 1 ? (cnt - 1) & 0xFFFFFFFFull : 0;
        const u64 ext = cnt ? c1 * (wide ? 1 : step) + 1 : 0;
        near &= !wide && ext + w.cs[k] - 1 < (1ull << 32);
        g.dim(w, bt, t, k, off, off + ext < off ? ~0ull : off + ext);
        wb.bs[k] = (u32)cnt;
        wb.ostr[k] = (i64)uni<UNI>((u64)bx->strides[d]);
        st.st[k] = cnt > 1 ? (u32)step : 1u;
        total *= cnt & 0xFFFFFFFFull;
    }
    wb.total = total;
    t.out = (u8*)(uintptr_t)uni<UNI>((u64)(uintptr_t)bx->base);
    i32 status = ZCG_OK;
    if (!stepped || !bounded) status = ZCG_ERR_INVALID_INPUT;
    else if (!near) status = ZCG_ERR_UNSUPPORTED;
    // a box with a zero extent has no element to place: it is in order wherever the table is
    else if (!(g.inside || !g.visits || total == 0)) status = ZCG_ERR_INVALID_INPUT;
    const bool use = status == ZCG_OK && g.visits && g.inside;
    t.table = table + (use ? g.base : 0);
    return SBoxFate{status, status == ZCG_OK && g.visits};
}

// launch_shape's rule for one box: long rows go a wave per row piece
__device__ __forceinline__ bool box_rows(const RegionWalk& wb) { return wb.bs[0] >= 32u * wb.V; }
// wave-sized units of a box with long rows
__device__ __forceinline__ u64 box_row_units(const RegionWalk& wb) { return wb.total / wb.bs[0] * row_pieces(wb); }
// workgroup-sized work units of a box that has elements
__device__ __forceinline__ u64 box_units(const RegionWalk& wb) {
    return box_rows(wb) ? (box_row_units(wb) + RP_WAVES - 1) / RP_WAVES
                        : (wb.total + (u64)RG_T * wb.V - 1) / ((u64)RG_T * wb.V);
}

// a box as the walk sees it: its part of RegionWalk, its terms, its step policy
template <class S>
struct WalkBox {
    RegionWalk w;
    BoxTerms t;
    S s;
};

// The walk kernel's body: this workgroup's run of the units the plan counted.
// box_of(b) gives box b's WalkBox (wave-uniform: the terms go to the scalar
// side); walk(box, rows, at, piece) does one wave's share of a unit — with
// rows, piece `piece` of row `at`; else tile `at`, by the whole workgroup.
// The search and the stepping are wave-uniform and stay scalar.
template <class BoxOf, class Walk>
__device__ __forceinline__ void walk_units(u64 n, const u64* __restrict__ prefix, BoxOf box_of, Walk walk) {
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
        const auto box = box_of(b);
        const u64 end = pe < last ? pe : last;
        if (box_rows(box.w)) {
            const u32 ppr = row_pieces(box.w);
            const u64 nwu = box_row_units(box.w);
            for (; unit < end; unit++) {
                const u64 wu = (unit - pb) * RP_WAVES + wv;
                if (wu >= nwu) continue;
                const u64 row = wu / ppr;
                walk(box, true, row, (u32)(wu - row * ppr));
            }
        } else {
            for (; unit < end; unit++) walk(box, false, unit - pb, 0u);
        }
    }
}

// The walk's grid, sized from the bound w.bs (the host does not know the
// boxes; any grid is correct, since workgroups divide the units the plan
// counted among themselves).
inline u32 walk_grid(const RegionWalk& w, u64 nboxes) {
    const u64 per_box = (w.total + (u64)RG_T * w.V - 1) / ((u64)RG_T * w.V);
    const u64 units = per_box * nboxes;
    return (u32)(units < RP_GRID ? units : RP_GRID);
}

}  // namespace zcg
