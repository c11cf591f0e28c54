// zcg_region_walk_s.h — the region walk with a step per dimension
// (zcg_region_s.hip).  Element x of the box along dimension k sits at hull
// position x * st[k]; everything else — the box terms, the chunk table, fill
// versus untouched, the view — is zcg_region_walk.h's, read direction only.
//
// Two paths, chosen per box by the step of the fast dimension:
//  - step 1: the dense walk.  Rows of the box are contiguous runs of chunk
//    rows, moved 16 bytes per lane; only the slow coordinates are scaled.
//  - step > 1: a lane owns one 16-byte piece of the OUTPUT row (V = 16/es
//    samples), gathers its V samples with V element loads and stores the piece
//    once.  Every sample has its own chunk index, so a step of the chunk
//    extent or more needs no special case.
#pragma once

#include "zcg_common.h"
#include "zcg_region_walk.h"

namespace zcg {

struct Steps {
    u32 st[ZCG_MAX_DIMS];  // per dim, fast-first order; 1 where the box has fewer than two samples
};

// walk_src with scaled coordinates; *run is meaningful for st[0] == 1 only
__device__ __forceinline__ const u8* walk_src_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, const Pos& p,
                                                u32* run) {
    u64 ti = 0, wi = 0;
    bool ok = true;
    u32 w0 = 0;
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        const u32 r = t.orr[k] + p.x[k] * s.st[k];
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

// the tile's first position (workgroup-uniform) plus this thread's offset; false: past the box
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

// Fast step 1, short box rows: walk_tile, chunks -> box.
__device__ __forceinline__ void walk_tile_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    const u8* src = walk_src_s(w, t, s, p, &run);
    if (rem == w.V && run >= w.V && w.ostr[0] == 1) {  // one 16-byte piece, both sides contiguous
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        if (src) st16(d, ld16(src));
        else if (w.fill) st16(d, fill_piece(w));
        return;
    }
    while (rem) {  // runs inside one chunk row and one box row
        const u32 k = run < rem ? run : rem;
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        const i64 ds = w.ostr[0] * (i64)w.es;
        for (u32 j = 0; j < k; j++) {
            if (src) copy_elem(d + j * ds, src + (u64)j * w.es, w.es);
            else if (w.fill) fill_elem(d + j * ds, w.fillv, w.es);
        }
        rem -= k;
        if (!rem) break;
        walk_advance(w, p, k);
        src = walk_src_s(w, t, s, p, &run);
    }
}

// the slow dimensions' part of a box row, from the row's index (scalar when the row is wave-uniform)
struct RowTerms {
    bool ok;    // every slow coordinate lies in a visited chunk
    u64 ti;     // chunk-table index, slow dimensions
    u64 wi;     // element index inside the chunk, slow dimensions
    i64 drow;   // element offset of the row in the view
};

__device__ __forceinline__ RowTerms row_terms_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row) {
    RowTerms R{true, 0, 0, 0};
    u64 e = row;
#pragma unroll
    for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        const u64 qd = e / w.bs[k];
        const u32 x = (u32)(e - qd * w.bs[k]);
        e = qd;
        const u32 r = t.orr[k] + x * s.st[k];
        const u32 q = r / w.cs[k];
        R.ok &= q < t.gn[k];
        R.ti += (u64)q * w.tstr[k];
        R.wi += (u64)(r - q * w.cs[k]) * w.cstr[k];
        R.drow += (i64)x * w.ostr[k];
    }
    return R;
}

// Fast step 1, long box rows: walk_row_piece, chunks -> box.
__device__ __forceinline__ void walk_row_piece_s(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                 u32 piece) {
    const u32 lane = threadIdx.x & 63;
    const u32x4 fill16 = fill_piece(w);
    const u32 V = w.V, bs0 = w.bs[0], cs0 = w.cs[0], orr0 = t.orr[0];
    const i64 es = w.es;
    constexpr u32 U = ZCG_RG_U;
    const u32 span = U * 64 * V;
    const RowTerms R = row_terms_s(w, t, s, row);
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
        dp[u] = drow_p + (i64)x0 * w.ostr[0] * es;
        if (xu >= bs0) continue;
        const u32 r = orr0 + x0;
        const u32 q = r / cs0;
        const u32 w0 = r - q * cs0;
        const bool here = ok && q < t.gn[0];
        const u8* base = here ? t.table[ti + (u64)q * w.tstr[0]] : nullptr;
        if (!(bs0 - x0 >= V && w0 + V <= cs0 && w.ostr[0] == 1)) { mode[u] = 3; continue; }
        if (base) { v[u] = ld16(base + (wi + w0) * (u64)es); mode[u] = 1; }
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
            if (bj) copy_elem(dj, bj + (wi + (rj - qj * cs0)) * (u64)es, w.es);
            else if (w.fill) fill_elem(dj, w.fillv, w.es);
        }
    }
}

template <u32 ES> struct ElemOf;
template <> struct ElemOf<1> { typedef u8 T; };
template <> struct ElemOf<2> { typedef u16 T; };
template <> struct ElemOf<4> { typedef u32 T; };
template <> struct ElemOf<8> { typedef u64 T; };

// Fast step > 1: samples x0 .. x0 + cnt (cnt <= V = 16/ES) of one box row,
// whose slow part is R; dst is element x0 of the row in the view.  Both rounds
// of loads — the samples' chunk pointers, then the samples — are issued
// unconditionally and together: a sample without a source loads from `safe`
// and its value is dropped.  One divide finds the first sample's chunk; the
// others follow by adding the step's quotient and remainder by the chunk
// extent.  A whole piece into a unit-stride view leaves as one 16-byte store
// unless, with fill off, a sample has no source and must stay untouched.
template <u32 ES>
__device__ __forceinline__ void gather_run(const RegionWalk& w, const BoxTerms& t, u32 st0, const RowTerms& R, u32 x0,
                                           u32 cnt, u8* dst, const u8* safe) {
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
    bool all = true;
#pragma unroll
    for (u32 j = 0; j < V; j++) {
        here[j] = here[j] && base[j] != nullptr;
        all &= here[j];
        v[j] = *(const E*)(here[j] ? base[j] + at[j] : safe);
    }
    if (cnt == V && w.ostr[0] == 1 && (all || w.fill)) {
#pragma unroll
        for (u32 j = 0; j < V; j++)
            if (!here[j]) v[j] = (E)w.fillv;
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
            if (here[j]) *(E*)(dst + (i64)j * ds) = v[j];
            else if (w.fill) *(E*)(dst + (i64)j * ds) = (E)w.fillv;
        }
    }
}

// Fast step > 1, long box rows: one piece of U*64*V samples of one box row,
// by a wave; lane l owns the V consecutive samples of its 16-byte output piece.
template <u32 ES>
__device__ __forceinline__ void gather_row_piece_es(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 row,
                                                    u32 piece, const u8* safe) {
    constexpr u32 V = 16 / ES, U = ZCG_RG_U, span = U * 64 * V;
    const u32 lane = threadIdx.x & 63, bs0 = w.bs[0];
    const RowTerms R = row_terms_s(w, t, s, row);
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
    switch (w.es) {
    case 1: gather_row_piece_es<1>(w, t, s, row, piece, safe); break;
    case 2: gather_row_piece_es<2>(w, t, s, row, piece, safe); break;
    case 4: gather_row_piece_es<4>(w, t, s, row, piece, safe); break;
    default: gather_row_piece_es<8>(w, t, s, row, piece, safe); break;
    }
}

// row_terms_s from a position instead of a row index
__device__ __forceinline__ RowTerms row_terms_at(const RegionWalk& w, const BoxTerms& t, const Steps& s,
                                                 const Pos& p) {
    RowTerms R{true, 0, 0, 0};
#pragma unroll
    for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
        if (k >= w.nd) break;
        const u32 r = t.orr[k] + p.x[k] * s.st[k];
        const u32 q = r / w.cs[k];
        R.ok &= q < t.gn[k];
        R.ti += (u64)q * w.tstr[k];
        R.wi += (u64)(r - q * w.cs[k]) * w.cstr[k];
        R.drow += (i64)p.x[k] * w.ostr[k];
    }
    return R;
}

// Fast step > 1, short box rows: a thread's V elements of the tile.  A piece
// that lies in one box row is gathered as in a long row; one that crosses a
// row's end, or ends the box, goes sample by sample.
__device__ __forceinline__ void gather_tile(const RegionWalk& w, const BoxTerms& t, const Steps& s, u64 tile,
                                            const u8* safe) {
    Pos p;
    u32 rem, run;
    if (!tile_start(w, tile, p, &rem)) return;
    if (rem == w.V && w.bs[0] - p.x[0] >= w.V) {
        const RowTerms R = row_terms_at(w, t, s, p);
        u8* d = t.out + (R.drow + (i64)p.x[0] * w.ostr[0]) * (i64)w.es;
        switch (w.es) {
        case 1: gather_run<1>(w, t, s.st[0], R, p.x[0], 16, d, safe); break;
        case 2: gather_run<2>(w, t, s.st[0], R, p.x[0], 8, d, safe); break;
        case 4: gather_run<4>(w, t, s.st[0], R, p.x[0], 4, d, safe); break;
        default: gather_run<8>(w, t, s.st[0], R, p.x[0], 2, d, safe); break;
        }
        return;
    }
    for (;;) {
        const u8* src = walk_src_s(w, t, s, p, &run);
        u8* d = t.out + walk_dst(w, p) * (i64)w.es;
        if (src) copy_elem(d, src, w.es);
        else if (w.fill) fill_elem(d, w.fillv, w.es);
        if (!--rem) break;
        walk_advance(w, p, 1);
    }
}

}  // namespace zcg
