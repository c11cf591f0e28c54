// zcg_region_walk_sw.h — the scatter of a box whose fast step is above 1
// (zcg_region_sw.hip): sample x of the box along dimension k goes to hull
// position x * st[k].  A box with fast step 1 goes through the dense walk of
// zcg_region_walk.h in its write direction; positions, row terms and
// tile_start are that header's, the element-size dispatch and a piece's chunk
// pointers zcg_region_walk_s.h's.
//
// Between two samples lie bytes that are not the box's, so no store is wider
// than an element.  Long rows: lane l takes sample 64*j + l
// of the row piece, so every store instruction of a wave covers one run of
// 64*step*es bytes (measured against a lane owning a 16-byte piece of the
// input row, the mirror of gather_run: 0.068 against 0.088 ms on the bench's
// step-2 and step-4 boxes).  Short rows (tiles): a thread's 16-byte piece of
// the input, one load, V chunk pointers resolved together, V element stores.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"
#include "zcg_region_walk_s.h"

namespace zcg {

// A tile's piece: samples x0 .. x0 + cnt (cnt <= V = 16/ES) of one box row,
// whose slow part is R; src is element x0 of the row in the view.  The piece
// is loaded once when it is whole and the view's stride is 1, else element by
// element.  The samples' chunk pointers are loaded unconditionally and
// together (run_chunks); then one store per sample that has a chunk, never
// wider than the element.
template <u32 ES>
__device__ __forceinline__ void scatter_run(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x0,
                                            u32 cnt, const u8* src, const u8* safe) {
    typedef typename ElemOf<ES>::T E;
    constexpr u32 V = 16 / ES;
    u8* at[V];
    run_chunks<ES>(w, t, st0, R, x0, cnt, safe, at);
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
        if (at[j]) *(E*)at[j] = v[j];
}

// Long rows: sample x of one box row, by the lane that owns it.
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

// Long box rows: one piece of U*64*V samples of one box row, by a wave; lane l
// takes samples l, 64 + l, ... of the piece.
template <u32 ES>
__device__ __forceinline__ void scatter_row_piece_es(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                     u32 piece) {
    constexpr u32 V = 16 / ES, U = ZCG_RG_U, span = U * 64 * V;
    const u32 lane = threadIdx.x & 63, bs0 = w.bs[0];
    const RowTerms R = row_terms<ZCG_MAX_DIMS>(w, t, s, row);
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
    by_es(w.es, [&](auto e) { scatter_row_piece_es<decltype(e)::ES>(w, t, s, row, piece); });
}

// Short box rows: a thread's V elements of the tile.  A piece that lies in one
// box row is scattered as in a long row; one that crosses a row's end, or ends
// the box, goes sample by sample.
__device__ __forceinline__ void scatter_tile(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile,
                                             const u8* safe) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    if (rem == w.V && w.bs[0] - p.x[0] >= w.V) {
        const RowTerms R = row_terms_at(w, t, s, p);
        const u8* v = t.out + (R.drow + (i64)p.x[0] * w.ostr[0]) * (i64)w.es;
        by_es(w.es, [&](auto e) {
            constexpr u32 ES = decltype(e)::ES;
            scatter_run<ES>(w, t, s.st[0], R, p.x[0], 16 / ES, v, safe);
        });
        return;
    }
    for (;;) {
        u8* dst = (u8*)walk_src(w, t, s, p, &run);
        if (dst) copy_elem(dst, t.out + walk_dst(w, p) * (i64)w.es, w.es);
        if (!--rem) break;
        walk_advance(w, p, 1);
    }
}

}  // namespace zcg
