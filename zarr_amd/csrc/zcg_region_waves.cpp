// zcg_region_waves.cpp — the host mathematics of the write side's order, no
// GPU and no file: zcg_regions_waves / _v_waves / _s_waves split a list of
// boxes into consecutive runs of pairwise disjoint boxes, so that scatters of
// the runs, in order on one stream, let a later box win (write_ndarray box by
// box, ndarray.rs:276-385); zcg_points_last marks, among points with one
// coordinate, the last.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/zchunk_gpu.h"

namespace {

// a box's cells along one dimension: first and last cell index
struct CellRange {
    uint64_t lo, hi;
};

typedef unsigned __int128 u128;

// Do the progressions {o1 + i*s1, i < c1} and {o2 + j*s2, j < c2} share an
// index?  c1, c2 >= 1, s1, s2 >= 1, and both last samples are below 2^64.
// Exact, by the congruence x = o1 (mod s1), x = o2 (mod s2): solvable iff
// gcd(s1, s2) divides o2 - o1; the least solution at or above max(o1, o2) must
// not pass either last sample.  No loop over samples.
bool progressions_meet(uint64_t o1, uint64_t c1, uint64_t s1, uint64_t o2, uint64_t c2, uint64_t s2) {
    if (c1 < 2) s1 = 1;  // the step of a lone sample is irrelevant
    if (c2 < 2) s2 = 1;
    if (o1 > o2) { std::swap(o1, o2); std::swap(c1, c2); std::swap(s1, s2); }
    const u128 last1 = (u128)o1 + (u128)(c1 - 1) * s1, last2 = (u128)o2 + (u128)(c2 - 1) * s2;
    const u128 last = std::min(last1, last2);
    if (o2 > last) return false;
    uint64_t g = s1, h = s2;
    while (h) { const uint64_t t = g % h; g = h; h = t; }
    const uint64_t diff = o2 - o1;
    if (diff % g) return false;
    // x = o1 + s1*k with (s1/g)*k = diff/g (mod m), m = s2/g: k = (diff/g) * inverse of s1/g mod m
    const uint64_t m = s2 / g, a = (s1 / g) % m;
    uint64_t k = 0;
    if (m > 1) {
        __int128 t0 = 0, t1 = 1;  // extended Euclid: t1 * a = r1 (mod m)
        uint64_t r0 = m, r1 = a;
        while (r1 > 1) {
            const uint64_t q = r0 / r1, r2 = r0 - q * r1;
            const __int128 t2 = t0 - (__int128)q * t1;
            r0 = r1; r1 = r2; t0 = t1; t1 = t2;
        }
        const uint64_t inv = (uint64_t)(((t1 % (__int128)m) + m) % m);  // gcd(a, m) = 1, so r1 ends at 1
        k = (uint64_t)((u128)((diff / g) % m) * inv % m);
    }
    u128 x = (u128)o1 + (u128)s1 * k;  // the least solution at or above o1; the next ones are lcm apart
    if (x < o2) {
        const u128 lcm = (u128)(s1 / g) * s2, need = (u128)o2 - x;
        if (lcm > last) return false;  // the next solution is past every sample
        x += (need + lcm - 1) / lcm * lcm;
    }
    return x <= last;
}

// zcg_regions_waves, zcg_regions_v_waves and zcg_regions_s_waves: box b's
// shape is shapes + b * sstep (sstep 0: one shape for all); steps (n_boxes *
// ndim, or NULL): shapes are sample counts and two boxes intersect when their
// progressions do.  Cells and hashing go by the hulls.
uint32_t regions_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes, size_t sstep,
                       const uint64_t* steps, uint32_t n_boxes, uint32_t* wave_of) {
    if (!r || !offsets || !shapes || !wave_of || n_boxes == 0) return 0;
    const uint32_t nd = r->ndim;
    if (nd < 1 || nd > ZCG_MAX_DIMS) return 0;
    // strided: the hulls' extents (saturating) stand in for the shapes below;
    // a box with a step of 0 gets a zero extent and intersects nothing
    const uint64_t* counts = shapes;
    std::vector<uint64_t> hulls;
    std::vector<uint8_t> over;  // per box: a hull end passes 2^64
    if (steps) {
        hulls.assign((size_t)n_boxes * nd, 0);
        over.assign(n_boxes, 0);
        for (uint32_t b = 0; b < n_boxes; b++) {
            bool stepped = true;
            for (uint32_t d = 0; d < nd; d++) stepped &= steps[(size_t)b * nd + d] != 0;
            for (uint32_t d = 0; stepped && d < nd; d++) {
                const size_t i = (size_t)b * nd + d;
                const uint64_t c = counts[i];
                const u128 e = c ? (u128)(c - 1) * (c > 1 ? steps[i] : 1) + 1 : 0;
                hulls[i] = e > ~0ull ? ~0ull : (uint64_t)e;
                if (e + offsets[i] > ~0ull) over[b] = 1;
            }
        }
        shapes = hulls.data();
        sstep = nd;
    }
    // Cells: per dimension the smallest multiple of the chunk extent that holds
    // the largest box extent (r->bbox_shape, unless a box exceeds it), so a box
    // lies in at most two cells per dimension and two boxes that intersect
    // share a cell.  A box is compared with the boxes of the current wave that
    // are registered in one of its cells.
    uint64_t cell[ZCG_MAX_DIMS];
    for (uint32_t d = 0; d < nd; d++) {
        uint64_t bs = steps ? 0 : sstep ? r->bbox_shape[d] : shapes[d];
        for (uint32_t b = 0; sstep && b < n_boxes; b++) bs = std::max(bs, shapes[(size_t)b * sstep + d]);
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        const uint64_t k = std::max<uint64_t>(bs / cs + (bs % cs ? 1 : 0), 1);
        cell[d] = k > (~0ull) / cs ? ~0ull : k * cs;
    }
    auto end_of = [&](uint32_t b, uint32_t d) {
        const uint64_t o = offsets[(size_t)b * nd + d], e = o + shapes[(size_t)b * sstep + d];
        return e < o ? ~0ull : e;  // saturating
    };
    std::unordered_map<uint64_t, std::vector<uint32_t>> cells;  // hash of the cell position -> boxes
    uint32_t wave = 0;
    for (uint32_t b = 0; b < n_boxes; b++) {
        const uint64_t* ob = offsets + (size_t)b * nd;
        CellRange cr[ZCG_MAX_DIMS];
        bool has = true;  // false: the saturated extent is empty, the box intersects nothing
        uint32_t ncell = 1;
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t e = end_of(b, d);
            if (e <= ob[d]) { has = false; break; }
            cr[d] = CellRange{ob[d] / cell[d], (e - 1) / cell[d]};
            ncell *= (uint32_t)(cr[d].hi - cr[d].lo + 1);
        }
        if (!has) {
            wave_of[b] = wave;
            continue;
        }
        uint64_t keys[1u << ZCG_MAX_DIMS];
        for (uint32_t c = 0; c < ncell; c++) {
            uint64_t h = 0x9E3779B97F4A7C15ull;
            uint32_t rem = c;
            for (uint32_t d = 0; d < nd; d++) {
                const uint32_t w = (uint32_t)(cr[d].hi - cr[d].lo + 1);
                h = (h ^ (cr[d].lo + rem % w)) * 0xFF51AFD7ED558CCDull;
                h ^= h >> 32;
                rem /= w;
            }
            keys[c] = h;
        }
        bool hit = false;
        for (uint32_t c = 0; c < ncell && !hit; c++) {
            auto it = cells.find(keys[c]);
            if (it == cells.end()) continue;
            for (uint32_t a : it->second) {
                const uint64_t* oa = offsets + (size_t)a * nd;
                bool meet = true;
                const bool exact = steps && !over[a] && !over[b];  // else the (saturated) hulls' intervals
                for (uint32_t d = 0; d < nd && meet; d++)
                    meet = exact ? progressions_meet(oa[d], counts[(size_t)a * nd + d], steps[(size_t)a * nd + d],
                                                     ob[d], counts[(size_t)b * nd + d], steps[(size_t)b * nd + d])
                                 : std::max(oa[d], ob[d]) < std::min(end_of(a, d), end_of(b, d));
                if (meet) { hit = true; break; }
            }
        }
        if (hit) {
            wave++;
            cells.clear();
        }
        wave_of[b] = wave;
        for (uint32_t c = 0; c < ncell; c++) cells[keys[c]].push_back(b);
    }
    return wave + 1;
}

}  // namespace

extern "C" uint32_t zcg_regions_waves(const zcg_region* r, const uint64_t* offsets, uint32_t n_boxes,
                                      uint32_t* wave_of) {
    return regions_waves(r, offsets, r ? r->bbox_shape : nullptr, 0, nullptr, n_boxes, wave_of);
}

extern "C" uint32_t zcg_regions_v_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                                        uint32_t n_boxes, uint32_t* wave_of) {
    return regions_waves(r, offsets, shapes, r ? r->ndim : 0, nullptr, n_boxes, wave_of);
}

extern "C" uint32_t zcg_regions_s_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                                        const uint64_t* steps, uint32_t n_boxes, uint32_t* wave_of) {
    if (!steps) return 0;
    return regions_waves(r, offsets, shapes, r ? r->ndim : 0, steps, n_boxes, wave_of);
}

extern "C" uint64_t zcg_points_last(const uint64_t* coords, uint64_t n_points, uint32_t ndim, uint8_t* keep) {
    if (!coords || !keep || ndim < 1 || ndim > ZCG_MAX_DIMS) return 0;
    std::vector<uint64_t> idx(n_points);
    for (uint64_t i = 0; i < n_points; i++) idx[i] = i;
    // equal coordinates next to each other, the latest point last
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
        const uint64_t *ca = coords + a * ndim, *cb = coords + b * ndim;
        for (uint32_t d = 0; d < ndim; d++)
            if (ca[d] != cb[d]) return ca[d] < cb[d];
        return a < b;
    });
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n_points; i++) {
        const bool last = i + 1 == n_points ||
                          memcmp(coords + idx[i] * ndim, coords + idx[i + 1] * ndim, ndim * sizeof(uint64_t)) != 0;
        keep[idx[i]] = last ? 1 : 0;
        kept += last;
    }
    return kept;
}
