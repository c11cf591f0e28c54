// zcg_region_sbox.h — the per-box terms of a strided box (zcg_sbox), shared by
// the assembly kernels of zcg_region_s.hip and the scatter kernel of
// zcg_region_sw.hip: one definition of what a box's status is, which chunks
// its hull visits and how its work is counted.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"

namespace zcg {

constexpr u32 RS_PLAN_T = 1024;      // threads of the plan kernel's one workgroup
constexpr u32 RS_WAVES = RG_T / 64;  // row pieces per work unit
constexpr u32 RS_GRID = 32768;       // cap of the walk's grid

template <bool UNI>
__device__ __forceinline__ u64 uni(u64 x) { return UNI ? ru64(x) : x; }

struct SBoxFate {
    i32 status;   // ZCG_OK: the box is walked (if it has work)
    bool visits;  // its hull visits a chunk
};

// The terms of box b: vbox_terms (zcg_region_v.hip) over the box's hull, the
// box's sample counts in wb.bs / wb.total, and its steps in st.  The step of a
// dimension with fewer than two samples is never used and kept as 1.
template <bool UNI>
__device__ __forceinline__ SBoxFate sbox_terms(const RegionWalk& w, const BoxTable& bt,
                                               const u8* const* __restrict__ table,
                                               const zcg_sbox* __restrict__ boxes, u64 b, RegionWalk& wb,
                                               BoxTerms& t, Steps& st) {
    const zcg_sbox* bx = boxes + b;
    wb = w;
    u64 base = 0, total = 1;
    bool inside = true, visits = true, bounded = true, stepped = true, near = true;
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
        const u64 cs = w.cs[k];
        const bool wide = cnt > 1 && step >= (1ull << 32);
        const u64 c1 = cnt > 1 ? (cnt - 1) & 0xFFFFFFFFull : 0;
        const u64 ext = cnt ? c1 * (wide ? 1 : step) + 1 : 0;
        near &= !wide && ext + cs - 1 < (1ull << 32);
        // zcg_region_grid's range of the hull (see box_terms)
        const u64 lo = off / cs;
        const u64 orr = off - lo * cs;
        const u64 oe = off + ext < off ? ~0ull : off + ext;
        const u64 end = oe < bt.as[k] ? oe : bt.as[k];
        const u64 s = end > off ? end - off : 0;
        const u32 span = (u32)orr + (u32)s, nq = span / w.cs[k];
        const u32 n = nq + (span != nq * w.cs[k] ? 1u : 0u);
        t.orr[k] = (u32)orr;
        t.gn[k] = n;
        visits &= n != 0;
        inside &= lo >= bt.tlo[k] && lo - bt.tlo[k] + n <= bt.tn[k];
        base += (lo - bt.tlo[k]) * w.tstr[k];
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
    else if (!(inside || !visits || total == 0)) status = ZCG_ERR_INVALID_INPUT;
    const bool use = status == ZCG_OK && visits && inside;
    t.table = table + (use ? base : 0);
    return SBoxFate{status, status == ZCG_OK && visits};
}

__device__ __forceinline__ bool sbox_rows(const RegionWalk& wb) { return wb.bs[0] >= 32u * wb.V; }
__device__ __forceinline__ u64 sbox_row_units(const RegionWalk& wb) { return wb.total / wb.bs[0] * row_pieces(wb); }

}  // namespace zcg
