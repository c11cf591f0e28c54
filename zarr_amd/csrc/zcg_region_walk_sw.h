// zcg_region_walk_sw.h — the strided region walk in the write direction
// (zcg_region_sw.hip): sample x of the box along dimension k goes to hull
// position x * st[k].  Positions, box terms and the chunk table are
// zcg_region_walk_s.h's; its read functions are not touched and call nothing
// from here.
//
// Two paths, chosen per box by the step of the fast dimension:
//  - step 1: the dense walk, box -> chunks.  A 16-byte load from the view and a
//    16-byte store into the chunk row; per-element runs where a piece crosses a
//    chunk boundary, ends the row, or the view's fast stride is not 1.
//  - step > 1: between two samples lie bytes that are not the box's, so no
//    store is wider than an element.  Long rows: lane l takes sample
//    64*j + l of the row piece, so every store instruction of a wave covers
//    one run of 64*step*es bytes (measured against a lane owning a 16-byte
//    piece of the input row, the mirror of gather_run: 0.068 against 0.088 ms
//    on the bench's step-2 and step-4 boxes).  Short rows (tiles): a thread's
//    16-byte piece of the input, one load, V chunk pointers resolved together,
//    V element stores.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"

namespace zcg {

// Fast step 1, short box rows: walk_tile_s, box -> chunks.
__device__ __forceinline__ void scatter_tile_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    u8* dst = (u8*)walk_src_s(w, t, s, p, &run);
    if (rem == w.V && run >= w.V && w.ostr[0] == 1) {  // one 16-byte piece, both sides contiguous
        if (dst) st16(dst, ld16(t.out + walk_dst(w, p) * (i64)w.es));
        return;
    }
    while (rem) {  // runs inside one chunk row and one box row
        const u32 k = run < rem ? run : rem;
        const u8* v = t.out + walk_dst(w, p) * (i64)w.es;
        const i64 vs = w.ostr[0] * (i64)w.es;
        if (dst)
            for (u32 j = 0; j < k; j++) copy_elem(dst + (u64)j * w.es, v + j * vs, w.es);
        rem -= k;
        if (!rem) break;
        walk_advance(w, p, k);
        dst = (u8*)walk_src_s(w, t, s, p, &run);
    }
}

// Fast step 1, long box rows: walk_row_piece_s, box -> chunks.
__device__ __forceinline__ void scatter_row_piece_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                    u32 piece) {
    const u32 lane = threadIdx.x & 63;
    const u32 V = w.V, bs0 = w.bs[0], cs0 = w.cs[0], orr0 = t.orr[0];
    const i64 es = w.es;
    constexpr u32 U = ZCG_RG_U;
    const u32 span = U * 64 * V;
    const RowTerms R = row_terms_s(w, t, s, row);
    const bool ok = R.ok;
    const u64 ti = R.ti, wi = R.wi;
    const u8* vrow = t.out + R.drow * es;
    // U pieces per lane in flight: loads first, then stores
    const u64 xb = (u64)piece * span + lane * V;
    u32x4 v[U];
    u8* dp[U];
    u32 mode[U];  // 0 skip, 1 load+store, 3 element runs
#pragma unroll
    for (u32 u = 0; u < U; u++) {
        const u64 xu = xb + (u64)u * 64 * V;
        mode[u] = 0;
        dp[u] = nullptr;
        if (xu >= bs0) continue;
        const u32 x0 = (u32)xu;
        const u32 r = orr0 + x0;
        const u32 q = r / cs0;
        const u32 w0 = r - q * cs0;
        if (!(bs0 - x0 >= V && w0 + V <= cs0 && w.ostr[0] == 1)) { mode[u] = 3; continue; }
        const bool here = ok && q < t.gn[0];
        const u8* base = here ? t.table[ti + (u64)q * w.tstr[0]] : nullptr;
        if (base) {
            v[u] = ld16(vrow + (i64)x0 * es);
            dp[u] = (u8*)base + (wi + w0) * (u64)es;
            mode[u] = 1;
        }
    }
#pragma unroll
    for (u32 u = 0; u < U; u++)
        if (mode[u] == 1) st16(dp[u], v[u]);
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
            if (bj) copy_elem((u8*)bj + (wi + (rj - qj * cs0)) * (u64)es, vrow + (i64)(x0 + j) * w.ostr[0] * es, w.es);
        }
    }
}

// Fast step > 1, a tile's piece: samples x0 .. x0 + cnt (cnt <= V = 16/ES) of
// one box row, whose slow part is R; src is element x0 of the row in the view.
// The piece is loaded once when it is whole and the view's stride is 1, else
// element by element.  The samples' chunk pointers are loaded unconditionally
// and together (a sample without a chunk reads `safe`); then one store per
// sample that has a chunk, never wider than the element.
template <u32 ES>
__device__ __forceinline__ void scatter_run(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x0,
                                            u32 cnt, const u8* src, const u8* safe) {
    typedef typename ElemOf<ES>::T E;
    constexpr u32 V = 16 / ES;
    const u32 cs0 = w.cs[0];
    const u32 qs = st0 / cs0, rs = st0 - qs * cs0;
    const u32 r = t.orr[0] + x0 * st0;
    u32 q = r / cs0, c = r - q * cs0;
    const u8* const* ent[V];
    u64 at[V];
    bool here[V];
#pragma unroll
    for (u32 j = 0; j < V; j++) {
        here[j] = R.ok && j < cnt && q < t.gn[0];
        ent[j] = here[j] ? t.table + (R.ti + (u64)q * w.tstr[0]) : (const u8* const*)safe;
        at[j] = (R.wi + c) * (u64)ES;
        c += rs;
        q += qs;
        if (c >= cs0) { c -= cs0; q++; }
    }
    const u8* base[V];
#pragma unroll
    for (u32 j = 0; j < V; j++) base[j] = *ent[j];
    E v[V];
    if (cnt == V && w.ostr[0] == 1) {
        const u32x4 p = ld16(src);
        const u32 p4[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (u32 j = 0; j < V; j++) {
            if (ES == 8) v[j] = (E)((u64)p4[(2 * j) & 3] | ((u64)p4[(2 * j + 1) & 3] << 32));
            else v[j] = (E)(p4[(j * ES) / 4] >> (8 * ((j * ES) & 3)));
        }
    } else {
        const i64 vs = w.ostr[0] * (i64)ES;
#pragma unroll
        for (u32 j = 0; j < V; j++) v[j] = j < cnt ? *(const E*)(src + (i64)j * vs) : (E)0;
    }
#pragma unroll
    for (u32 j = 0; j < V; j++)
        if (here[j] && base[j]) *(E*)((u8*)base[j] + at[j]) = v[j];
}

// Fast step > 1, long rows: sample x of one box row, by the lane that owns it.
template <u32 ES>
__device__ __forceinline__ void scatter_one(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x,
                                            const u8* src) {
    typedef typename ElemOf<ES>::T E;
    const u32 r = t.orr[0] + x * st0;
    const u32 q = r / w.cs[0];
    if (!(R.ok && q < t.gn[0])) return;
    const E v = *(const E*)src;
    const u8* base = t.table[R.ti + (u64)q * w.tstr[0]];
    if (base) *(E*)((u8*)base + (R.wi + (r - q * w.cs[0])) * (u64)ES) = v;
}

// Fast step > 1, long box rows: one piece of U*64*V samples of one box row, by
// a wave; lane l takes samples l, 64 + l, ... of the piece.
template <u32 ES>
__device__ __forceinline__ void scatter_row_piece_es(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                     u32 piece) {
    constexpr u32 V = 16 / ES, U = ZCG_RG_U, span = U * 64 * V;
    const u32 lane = threadIdx.x & 63, bs0 = w.bs[0];
    const RowTerms R = row_terms_s(w, t, s, row);
    const u8* vrow = t.out + R.drow * (i64)ES;
    const u64 xb = (u64)piece * span + lane;
#pragma unroll 4
    for (u32 j = 0; j < U * V; j++) {
        const u64 xu = xb + (u64)j * 64;
        if (xu >= bs0) break;
        scatter_one<ES>(w, t, s.st[0], R, (u32)xu, vrow + (i64)xu * w.ostr[0] * (i64)ES);
    }
}

__device__ __forceinline__ void scatter_row_piece(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                  u32 piece) {
    switch (w.es) {
    case 1: scatter_row_piece_es<1>(w, t, s, row, piece); break;
    case 2: scatter_row_piece_es<2>(w, t, s, row, piece); break;
    case 4: scatter_row_piece_es<4>(w, t, s, row, piece); break;
    default: scatter_row_piece_es<8>(w, t, s, row, piece); break;
    }
}

// Fast step > 1, short box rows: a thread's V elements of the tile.  A piece
// that lies in one box row is scattered as in a long row; one that crosses a
// row's end, or ends the box, goes sample by sample.
__device__ __forceinline__ void scatter_tile(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile,
                                             const u8* safe) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    if (rem == w.V && w.bs[0] - p.x[0] >= w.V) {
        const RowTerms R = row_terms_at(w, t, s, p);
        const u8* v = t.out + (R.drow + (i64)p.x[0] * w.ostr[0]) * (i64)w.es;
        switch (w.es) {
        case 1: scatter_run<1>(w, t, s.st[0], R, p.x[0], 16, v, safe); break;
        case 2: scatter_run<2>(w, t, s.st[0], R, p.x[0], 8, v, safe); break;
        case 4: scatter_run<4>(w, t, s.st[0], R, p.x[0], 4, v, safe); break;
        default: scatter_run<8>(w, t, s.st[0], R, p.x[0], 2, v, safe); break;
        }
        return;
    }
    for (;;) {
        u8* dst = (u8*)walk_src_s(w, t, s, p, &run);
        if (dst) copy_elem(dst, t.out + walk_dst(w, p) * (i64)w.es, w.es);
        if (!--rem) break;
        walk_advance(w, p, 1);
    }
}

}  // namespace zcg
