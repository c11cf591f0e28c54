// zcg_region_walk_s.h — the gather of a box whose fast step is above 1
// (zcg_region_s.hip), and what it shares with the scatter of such a box
// (zcg_region_walk_sw.h): the element-size dispatch and a piece's chunk
// pointers.  A box with fast step 1 goes through the dense walk of
// zcg_region_walk.h with its Steps; positions, row terms and tile_start are
// that header's too.
//
// A lane owns one 16-byte piece of the OUTPUT row (V = 16/es samples), gathers
// its V samples with V element loads and stores the piece once.  Every sample
// has its own chunk index, so a step of the chunk extent or more needs no
// special case.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"

namespace zcg {

template <u32 N> struct ElemOf;
template <> struct ElemOf<1> { typedef u8 T; static constexpr u32 ES = 1; };
template <> struct ElemOf<2> { typedef u16 T; static constexpr u32 ES = 2; };
template <> struct ElemOf<4> { typedef u32 T; static constexpr u32 ES = 4; };
template <> struct ElemOf<8> { typedef u64 T; static constexpr u32 ES = 8; };

// f(ElemOf<es>{}): the run-time element size onto a compile-time one
template <class F>
__device__ __forceinline__ void by_es(u32 es, F f) {
    switch (es) {
    case 1: f(ElemOf<1>{}); break;
    case 2: f(ElemOf<2>{}); break;
    case 4: f(ElemOf<4>{}); break;
    default: f(ElemOf<8>{}); break;
    }
}

// Where samples x0 .. x0 + cnt (cnt <= V = 16/ES) of one box row, whose slow
// part is R, lie in their chunks; nullptr: the sample has no chunk (or j >=
// cnt).  One divide finds the first sample's chunk; the others follow by
// adding the step's quotient and remainder by the chunk extent.  The V table
// entries are loaded unconditionally and together: a sample that is outside
// the box's grid range loads from `safe` (any readable, 8-byte aligned device
// address) and the value is dropped.
template <u32 ES>
__device__ __forceinline__ void run_chunks(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x0,
                                           u32 cnt, const u8* safe, u8* (&at)[16 / ES]) {
    constexpr u32 V = 16 / ES;
    const u32 cs0 = w.cs[0];
    const u32 qs = st0 / cs0, rs = st0 - qs * cs0;
    const u32 r = t.orr[0] + x0 * st0;
    u32 q = r / cs0, c = r - q * cs0;
    const u8* const* ent[V];
    u64 off[V];
    bool here[V];
#pragma unroll
    for (u32 j = 0; j < V; j++) {
        here[j] = R.ok && j < cnt && q < t.gn[0];
        ent[j] = here[j] ? t.table + (R.ti + (u64)q * w.tstr[0]) : (const u8* const*)safe;
        off[j] = (R.wi + c) * (u64)ES;
        c += rs;
        q += qs;
        if (c >= cs0) { c -= cs0; q++; }
    }
    const u8* base[V];
#pragma unroll
    for (u32 j = 0; j < V; j++) base[j] = *ent[j];
#pragma unroll
    for (u32 j = 0; j < V; j++) at[j] = here[j] && base[j] ? (u8*)base[j] + off[j] : nullptr;
}

// Samples x0 .. x0 + cnt of one box row; dst is element x0 of the row in the
// view.  Both rounds of loads — the samples' chunk pointers (run_chunks), then
// the samples — are issued unconditionally and together: a sample without a
// source loads from `safe` and its value is dropped.  A whole piece into a
// unit-stride view leaves as one 16-byte store unless, with fill off, a sample
// has no source and must stay untouched.
template <u32 ES>
__device__ __forceinline__ void gather_run(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x0,
                                           u32 cnt, u8* dst, const u8* safe) {
    typedef typename ElemOf<ES>::T E;
    constexpr u32 V = 16 / ES;
    u8* at[V];
    run_chunks<ES>(w, t, st0, R, x0, cnt, safe, at);
    E v[V];
    bool all = true;
#pragma unroll
    for (u32 j = 0; j < V; j++) {
        all &= at[j] != nullptr;
        v[j] = *(const E*)(at[j] ? at[j] : safe);
    }
    if (cnt == V && w.ostr[0] == 1 && (all || w.fill)) {
#pragma unroll
        for (u32 j = 0; j < V; j++)
            if (!at[j]) v[j] = (E)w.fillv;
        u32 p4[4];
#pragma unroll
        for (u32 i = 0; i < 4; i++) {  // the piece's four words, from registers
            if (ES == 8) p4[i] = (u32)((u64)v[(i * 4) / ES] >> (32 * (i & 1)));
            else if (ES == 4) p4[i] = (u32)v[(i * 4) / ES];
            else {
                p4[i] = 0;
#pragma unroll
                for (u32 j = 0; j < 4 / (ES < 4 ? ES : 4); j++)
                    p4[i] |= (u32)v[(i * 4) / ES + j] << (8 * ES * j);
            }
        }
        st16(dst, u32x4{p4[0], p4[1], p4[2], p4[3]});
        return;
    }
    const i64 ds = w.ostr[0] * (i64)ES;
#pragma unroll
    for (u32 j = 0; j < V; j++) {
        if (j < cnt) {
            if (at[j]) *(E*)(dst + (i64)j * ds) = v[j];
            else if (w.fill) *(E*)(dst + (i64)j * ds) = (E)w.fillv;
        }
    }
}

// Long box rows: one piece of U*64*V samples of one box row, by a wave; lane l
// owns the V consecutive samples of its 16-byte output piece.
template <u32 ES>
__device__ __forceinline__ void gather_row_piece_es(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                    u32 piece, const u8* safe) {
    constexpr u32 V = 16 / ES, U = ZCG_RG_U, span = U * 64 * V;
    const u32 lane = threadIdx.x & 63, bs0 = w.bs[0];
    const RowTerms R = row_terms<ZCG_MAX_DIMS>(w, t, s, row);
    u8* drow_p = t.out + R.drow * (i64)ES;
    const u64 xb = (u64)piece * span + lane * V;
#pragma unroll 1
    for (u32 u = 0; u < U; u++) {
        const u64 xu = xb + (u64)u * 64 * V;
        if (xu >= bs0) break;
        const u32 x0 = (u32)xu;
        gather_run<ES>(w, t, s.st[0], R, x0, bs0 - x0 < V ? bs0 - x0 : V, drow_p + (i64)x0 * w.ostr[0] * (i64)ES, safe);
    }
}

__device__ __forceinline__ void gather_row_piece(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                 u32 piece, const u8* safe) {
    by_es(w.es, [&](auto e) { gather_row_piece_es<decltype(e)::ES>(w, t, s, row, piece, safe); });
}

// Short box rows: a thread's V elements of the tile.  A piece that lies in one
// box row is gathered as in a long row; one that crosses a row's end, or ends
// the box, goes sample by sample.
__device__ __forceinline__ void gather_tile(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile,
                                            const u8* safe) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    if (rem == w.V && w.bs[0] - p.x[0] >= w.V) {
        const RowTerms R = row_terms_at(w, t, s, p);
        u8* d = t.out + (R.drow + (i64)p.x[0] * w.ostr[0]) * (i64)w.es;
        by_es(w.es, [&](auto e) {
            constexpr u32 ES = decltype(e)::ES;
            gather_run<ES>(w, t, s.st[0], R, p.x[0], 16 / ES, d, safe);
        });
        return;
    }
    for (;;) {
        const u8* src = walk_src(w, t, s, p, &run);
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        if (src) copy_elem(d, src, w.es);
        else if (w.fill) fill_elem(d, w.fillv, w.es);
        if (!--rem) break;
        walk_advance(w, p, 1);
    }
}

}  // namespace zcg
