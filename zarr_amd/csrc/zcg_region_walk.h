// zcg_region_walk.h — the dense region walk, written once for every region
// kernel: the four of zcg_region.hip (one box or many boxes per launch; a
// workgroup per tile or a wave per row piece), zcg_region_v.hip's (boxes of
// differing shapes) and, for boxes whose fast step is 1, the strided kernels
// of zcg_region_s.hip and zcg_region_sw.hip.  A kernel only decides where a
// box's terms (BoxTerms, for differing shapes the box's part of RegionWalk,
// for strided boxes its Steps) come from; what is done with them is here.
//
// A step policy S says how far apart two samples of the box lie along
// dimension k: Dense (the constant 1, an empty struct that leaves no trace in
// the code) or Steps (a step per dimension).  Sample x of the box along k sits
// at orr[k] + x * s(k) of the box's first chunk.  The walk itself needs the
// fast dimension dense: a box with a fast step above 1 goes through
// zcg_region_walk_s.h (gather) or zcg_region_walk_sw.h (scatter).
//
// The walk goes through a box in the chunks' memory order, 16 bytes per lane,
// so reads from a chunk row and writes to an output row with unit stride are
// both coalesced 16-byte accesses; a 16-byte piece that crosses a row or a
// chunk boundary is copied in per-element runs.  The per-dimension loops are
// unrolled to ZCG_MAX_DIMS, so positions and box terms stay in registers; the
// one exception is walk_row_piece's UNR.
#pragma once

#include "zcg_common.h"

namespace zcg {

constexpr u32 RG_T = 256;
// pieces per lane in flight per work unit (A/B: 1 / 2 / 4 / 8 / 16 -> 1 753 /
// 2 249 / 2 385 / 1 852 / 1 254 GiB/s of box on the bench leg)
#ifndef ZCG_RG_U
#define ZCG_RG_U 4
#endif

struct Pos {
    u32 x[ZCG_MAX_DIMS];
};

struct Dense {
    __device__ __forceinline__ u32 operator()(u32) const { return 1; }
};
struct Steps {
    u32 st[ZCG_MAX_DIMS];  // per dim, fast-first order; 1 where the box has fewer than two samples
    __device__ __forceinline__ u32 operator()(u32 k) const { return st[k]; }
};

__device__ __forceinline__ void copy_elem(u8* dst, const u8* src, u32 es) {
    switch (es) {
    case 1: *dst = *src; break;
    case 2: *(u16*)dst = *(const u16*)src; break;
    case 4: *(u32*)dst = *(const u32*)src; break;
    default: *(u64*)dst = *(const u64*)src; break;
    }
}
__device__ __forceinline__ void fill_elem(u8* dst, u64 v, u32 es) {
    switch (es) {
    case 1: *dst = (u8)v; break;
    case 2: *(u16*)dst = (u16)v; break;
    case 4: *(u32*)dst = (u32)v; break;
    default: *(u64*)dst = v; break;
    }
}

// 16 bytes of the fill element
__device__ __forceinline__ u32x4 fill_piece(u64 fv, u32 es) {
    if (es == 1) fv = (fv & 0xFF) * 0x0101010101010101ull;
    else if (es == 2) fv = (fv & 0xFFFF) * 0x0001000100010001ull;
    else if (es == 4) fv = (fv & 0xFFFFFFFFull) * 0x0000000100000001ull;
    return u32x4{(u32)fv, (u32)(fv >> 32), (u32)fv, (u32)(fv >> 32)};
}
__device__ __forceinline__ u32x4 fill_piece(const RegionWalk& w) { return fill_piece(w.fillv, w.es); }

// where element p of the box is read from (nullptr: no visited chunk), and
// how many elements from it stay in one chunk row and one box row (*run is
// meaningful for a fast step of 1 only)
template <class S>
__device__ __forceinline__ const u8* walk_src(const RegionWalk& w, const BoxTerms& t, const S& s, const Pos& p,
                                              u32* run) {
    u64 ti = 0, wi = 0;
    bool ok = true;
    u32 w0 = 0;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        const u32 r = t.orr[k] + p.x[k] * s(k);
        const u32 q = r / w.cs[k];
        const u32 c = r - q * w.cs[k];
        if (k == 0) w0 = c;
        ok &= q < t.gn[k];
        ti += (u64)q * w.tstr[k];
        wi += (u64)c * w.cstr[k];
    }
    const u32 r1 = w.bs[0] - p.x[0], r2 = w.cs[0] - w0;
    *run = r1 < r2 ? r1 : r2;
    if (!ok) return nullptr;
    const u8* base = t.table[ti];
    return base ? base + wi * w.es : nullptr;
}

__device__ __forceinline__ i64 walk_dst(const RegionWalk& w, const Pos& p) {
    i64 o = 0;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        o += (i64)p.x[k] * w.ostr[k];
    }
    return o;
}

// advance p by d elements along the fast-first order (carries)
__device__ __forceinline__ void walk_advance(const RegionWalk& w, Pos& p, u32 d) {
    u32 c = d;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd || !c) break;
        const u64 v = (u64)p.x[k] + c;
        if (v < w.bs[k]) { p.x[k] = (u32)v; c = 0; break; }
        const u64 q = v / w.bs[k];
        p.x[k] = (u32)(v - q * w.bs[k]);
        c = (u32)q;
    }
}

// The tile's first position (workgroup-uniform, scalar) plus this thread's
// offset, added with carries; false: past the box.  For the tile functions of
// zcg_region_walk_s.h and zcg_region_walk_sw.h.  walk_tile spells the same
// lines out: calling this from it changes the register allocation of every
// tile kernel of zcg_region.hip.
__device__ __forceinline__ bool tile_start(const RegionWalk& w, u64 tile, Pos& p, u32* rem) {
    const u64 tile_elems = (u64)RG_T * w.V;
    u64 e = tile * tile_elems;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k < w.nd) {
            const u64 q = e / w.bs[k];
            p.x[k] = (u32)(e - q * w.bs[k]);
            e = q;
        } else {
            p.x[k] = 0;
        }
    }
    const u64 e0 = tile * tile_elems + (u64)threadIdx.x * w.V;
    if (e0 >= w.total) return false;
    walk_advance(w, p, threadIdx.x * w.V);
    *rem = (u32)((w.total - e0) < w.V ? (w.total - e0) : w.V);
    return true;
}

// Short box rows: one tile of RG_T 16-byte pieces of the box, by a workgroup.
// The tile start is decomposed once (workgroup-uniform, scalar), threads add
// their offset with carries (tile_start's lines).  dir 0: chunks -> box
// (read_ndarray), 1: box -> chunks (write_ndarray).
template <class S>
__device__ __forceinline__ void walk_tile(const RegionWalk& w, const BoxTerms& t, const S& s, u64 tile, u32 dir) {
    const u64 tile_elems = (u64)RG_T * w.V;
    Pos p;
    u64 e = tile * tile_elems;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k < w.nd) {
            const u64 q = e / w.bs[k];
            p.x[k] = (u32)(e - q * w.bs[k]);
            e = q;
        } else {
            p.x[k] = 0;
        }
    }
    const u64 e0 = tile * tile_elems + (u64)threadIdx.x * w.V;
    if (e0 >= w.total) return;
    walk_advance(w, p, threadIdx.x * w.V);
    u32 rem = (u32)((w.total - e0) < w.V ? (w.total - e0) : w.V);
    u32 run;
    const u8* src = walk_src(w, t, s, p, &run);
    if (rem == w.V && run >= w.V && w.ostr[0] == 1) {  // one 16-byte piece, both sides contiguous
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        if (dir) { if (src) st16((u8*)src, ld16(d)); }
        else if (src) st16(d, ld16(src));
        else if (w.fill) st16(d, fill_piece(w));
        return;
    }
    while (rem) {  // runs inside one chunk row and one box row
        const u32 k = run < rem ? run : rem;
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        const i64 ds = w.ostr[0] * (i64)w.es;
        for (u32 j = 0; j < k; j++) {
            if (dir) { if (src) copy_elem((u8*)src + (u64)j * w.es, d + j * ds, w.es); }
            else if (src) copy_elem(d + j * ds, src + (u64)j * w.es, w.es);
            else if (w.fill) fill_elem(d + j * ds, w.fillv, w.es);
        }
        rem -= k;
        if (!rem) break;
        walk_advance(w, p, k);
        src = walk_src(w, t, s, p, &run);
    }
}

// pieces of U*64*V elements in a box row
__host__ __device__ __forceinline__ u32 row_pieces(const RegionWalk& w) {
    const u64 span = (u64)ZCG_RG_U * 64 * w.V;
    return (u32)((w.bs[0] + span - 1) / span);
}

// the slow dimensions' part of a box row (scalar when the row is wave-uniform)
struct RowTerms {
    u64 ti;     // chunk-table index, slow dimensions
    u64 wi;     // element index inside the chunk, slow dimensions
    i64 drow;   // element offset of the row in the view
    bool ok;    // every slow coordinate lies in a visited chunk

    // sample x of slow dimension k
    template <class S>
    __device__ __forceinline__ void add(const RegionWalk& w, const BoxTerms& t, const S& s, u32 k, u32 x) {
        const u32 r = t.orr[k] + x * s(k);
        const u32 q = r / w.cs[k];
        ok &= q < t.gn[k];
        ti += (u64)q * w.tstr[k];
        wi += (u64)(r - q * w.cs[k]) * w.cstr[k];
        drow += (i64)x * w.ostr[k];
    }
};

// from the row's index.  UNR: unroll count of the loop (walk_row_piece)
template <u32 UNR, class S>
__device__ __forceinline__ RowTerms row_terms(const RegionWalk& w, const BoxTerms& t, const S& s, u64 row) {
    u64 e = row;
    RowTerms R{0, 0, 0, true};
#pragma unroll UNR
    for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        const u64 qd = e / w.bs[k];
        R.add(w, t, s, k, (u32)(e - qd * w.bs[k]));
        e = qd;
    }
    return R;
}

// from a position in the box
template <class S>
__device__ __forceinline__ RowTerms row_terms_at(const RegionWalk& w, const BoxTerms& t, const S& s, const Pos& p) {
    RowTerms R{0, 0, 0, true};
#pragma unroll
    for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        R.add(w, t, s, k, p.x[k]);
    }
    return R;
}

// Long box rows (the common case: the fast dimension spans many 16-byte
// pieces): one piece of U*64*V elements of one box row, by a wave.  Many short
// units keep more loads in flight per CU than one long walk per row.  The
// row's coordinates, chunk-table and chunk-offset contributions of the slow
// dimensions are scalar, computed once per unit; lanes stream the piece 16
// bytes each.  Positions along the row are 64-bit until they are known to lie
// inside it.  UNR: unroll count of the slow-dimension loop.  ZCG_MAX_DIMS
// where the box terms are computed in registers (many boxes); 1 where they are
// kernel arguments (one box): unrolled, that kernel keeps every argument in
// SGPRs, spills them to VGPR lanes and runs 7 % slower on the bench leg.
template <u32 UNR, class S>
__device__ __forceinline__ void walk_row_piece(const RegionWalk& w, const BoxTerms& t, const S& s, u64 row,
                                               u32 piece, u32 dir) {
    const u32 lane = threadIdx.x & 63;
    const u32x4 fill16 = fill_piece(w);
    const u32 V = w.V, bs0 = w.bs[0], cs0 = w.cs[0], orr0 = t.orr[0];
    const i64 es = w.es;
    constexpr u32 U = ZCG_RG_U;
    const u32 span = U * 64 * V;
    const RowTerms R = row_terms<UNR>(w, t, s, row);
    const bool ok = R.ok;
    const u64 ti = R.ti, wi = R.wi;
    u8* drow_p = t.out + R.drow * es;
    // U pieces per lane in flight: loads first, then stores
    const u64 xb = (u64)piece * span + lane * V;
    u32x4 v[U];
    u8* dp[U];
    u32 mode[U];  // 0 skip, 1 load+store, 2 fill, 3 element runs
#pragma unroll
    for (u32 u = 0; u < U; u++) {
        const u64 xu = xb + (u64)u * 64 * V;
        mode[u] = 0;
        const u32 x0 = (u32)xu;
        dp[u] = drow_p + (i64)x0 * w.ostr[0] * es;  // also for a skipped piece: leaving it unset costs registers
        if (xu >= bs0) continue;
        const u32 r = orr0 + x0;
        const u32 q = r / cs0;
        const u32 w0 = r - q * cs0;
        const bool here = ok && q < t.gn[0];
        const u8* base = here ? t.table[ti + (u64)q * w.tstr[0]] : nullptr;
        if (!(bs0 - x0 >= V && w0 + V <= cs0 && w.ostr[0] == 1)) { mode[u] = 3; continue; }
        if (dir) {  // write_ndarray: box -> chunk
            if (base) { v[u] = ld16(dp[u]); dp[u] = (u8*)base + (wi + w0) * (u64)es; mode[u] = 1; }
        } else if (base) { v[u] = ld16(base + (wi + w0) * (u64)es); mode[u] = 1; }
        else if (w.fill) { v[u] = fill16; mode[u] = 2; }
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
            const u8* bj = hj ? t.table[ti + (u64)qj * w.tstr[0]] : nullptr;
            u8* dj = drow_p + (i64)(x0 + j) * w.ostr[0] * es;
            if (dir) { if (bj) copy_elem((u8*)bj + (wi + (rj - qj * cs0)) * (u64)es, dj, w.es); }
            else if (bj) copy_elem(dj, bj + (wi + (rj - qj * cs0)) * (u64)es, w.es);
            else if (w.fill) fill_elem(dj, w.fillv, w.es);
        }
    }
}

}  // namespace zcg
