// zcg_region_o.hip — region assembly and scatter for an orthogonal selection
// (zcg_read_ortho, zcg_write_ortho): numpy's a[np.ix_(rows, cols, planes)], one
// list of indices per dimension, the result their Cartesian product.  Element
// (i_0, .., i_{n-1}) of the selection is the point (L_0[i_0], .., L_{n-1}[i_{n-1}])
// of zcg_region_p.hip, bit for bit; but where the point kernel divides every
// coordinate of every element, a product needs one division per list entry.
//
// Two kernels.  The axis kernel takes a lane per list entry,
// divides its index by the chunk extent (point_div) and writes a 32-byte
// record: what the entry adds to the chunk-table index, to the element index
// inside the chunk and to the element offset in the view, and whether it
// visits a chunk and whether that chunk is inside the table.  The walk kernel
// goes through the selection in the chunks' memory order, a lane per 16-byte
// piece of a row (V = 16 / element size elements): it sums the slow
// dimensions' records (one load per dimension, the same address for the lanes
// of a row), reads its V fast records, and then issues the V table loads and
// the V element loads before the first value is used.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_point.h"
#include "zcg_region_walk.h"

namespace zcg {

namespace {

constexpr u32 OR_T = 256;
constexpr u32 OR_MAX_GRID = 1u << 16;

enum : u32 { OR_VISITS = 1, OR_INSIDE = 2 };

// One list entry.  ti is 0 unless the entry's chunk is inside the table, so a
// sum of records never indexes past it.
struct OrthoRec {
    u64 ti;     // (chunk index - table_lo) * table stride
    u64 wi;     // index inside the chunk * element stride inside a chunk
    i64 vo;     // position in the list * the view's stride, elements
    u32 flags;  // OR_VISITS | OR_INSIDE
    u32 pad;
};
static_assert(sizeof(OrthoRec) == ORTHO_REC_BYTES, "zcg_ortho_scratch_bytes sizes the records");

__device__ __forceinline__ OrthoRec load_rec(const OrthoRec* p) {
    const u32x4 a = ld16((const u8*)p), b = ld16((const u8*)p + 16);
    OrthoRec r;
    r.ti = (u64)a.x | (u64)a.y << 32;
    r.wi = (u64)a.z | (u64)a.w << 32;
    r.vo = (i64)((u64)b.x | (u64)b.y << 32);
    r.flags = b.z;
    r.pad = 0;
    return r;
}

// A lane per list entry; entry e belongs to the dimension k (fast-first) with
// ax.off[k] <= e < ax.off[k + 1].  w.ostr[k] is the view's stride.
__global__ __launch_bounds__(OR_T) void ortho_axis_kernel(RegionWalk w, BoxTable bt, PointRecip rc, OrthoAxes ax,
                                                          OrthoRec* __restrict__ recs,
                                                          u64* __restrict__ outside_words) {
    const u32 nd = w.nd;
    const u64 step = (u64)gridDim.x * OR_T;
    u64 outside = ~0ull;  // this lane's lowest position outside the table, along dimension mine
    u32 mine = 0;
    for (u64 e = (u64)blockIdx.x * OR_T + threadIdx.x; e < ax.off[nd]; e += step) {
        u32 k = 0;
#pragma unroll
        for (u32 j = 1; j < ZCG_MAX_DIMS; j++)
            if (j < nd && e >= ax.off[j]) k = j;
        // the dimension's terms, picked without indexing the arguments by a lane's value
        u32 cs = 0;
        u64 m = 0, as = 0, tlo = 0, tn = 0, tstr = 0, cstr = 0, base = 0;
        i64 ostr = 0;
        const u64* idx = nullptr;
        const u64* pos = nullptr;
#pragma unroll
        for (u32 j = 0; j < ZCG_MAX_DIMS; j++)
            if (j == k) {
                cs = w.cs[j]; m = rc.m[j]; as = bt.as[j]; tlo = bt.tlo[j]; tn = bt.tn[j];
                tstr = w.tstr[j]; cstr = w.cstr[j]; ostr = w.ostr[j]; base = ax.off[j];
                idx = ax.idx[j]; pos = ax.pos[j];
            }
        const u64 i = e - base;
        const u64 c = idx[i];
        u64 q;
        u32 rem;
        point_div(c, cs, m, &q, &rem);
        // points_kernel's rule, one dimension of it
        const bool visits = c < as || rem != 0;
        const bool inside = q >= tlo && q - tlo < tn;
        OrthoRec r;
        r.ti = inside ? (q - tlo) * tstr : 0;
        r.wi = (u64)rem * cstr;
        r.vo = (i64)((pos ? pos[i] : i) * (u64)ostr);
        r.flags = (visits ? OR_VISITS : 0u) | (inside ? OR_INSIDE : 0u);
        r.pad = 0;
        recs[e] = r;
        if (visits && !inside && (k != mine || i < outside)) {
            // a lane meets a second dimension only after gridDim.x * OR_T entries: flush the first
            if (k != mine && outside != ~0ull)
                atomicMin((unsigned long long*)&outside_words[bt.dim[mine]], (unsigned long long)outside);
            mine = k;
            outside = i;
        }
    }
    // per dimension: a wave reduction, one atomic per wave that has an entry outside
#pragma unroll
    for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
        if (k >= nd) break;
        u64 o = mine == k ? outside : ~0ull;
        if (!__any(o != ~0ull)) continue;
#pragma unroll
        for (u32 s = 32; s; s >>= 1) {
            const u64 y = __shfl_xor((unsigned long long)o, s, 64);
            o = y < o ? y : o;
        }
        if ((threadIdx.x & 63) == 0) atomicMin((unsigned long long*)&outside_words[bt.dim[k]], (unsigned long long)o);
    }
}

// DIR 0: chunks -> view (gather), 1: view -> chunks (scatter).  w.bs[k]: the
// list lengths, fast-first; w.total: pieces in all (rows x ax.ppr).
template <u32 DIR, u32 ES>
__global__ __launch_bounds__(OR_T) void ortho_walk_kernel(RegionWalk w, PointRecip rc, OrthoAxes ax,
                                                          const u8* const* __restrict__ table,
                                                          const OrthoRec* __restrict__ recs, u8* view) {
    constexpr u32 V = 16 / ES;
    const u32 nd = w.nd;
    const u64 step = (u64)gridDim.x * OR_T;
    for (u64 pc = (u64)blockIdx.x * OR_T + threadIdx.x; pc < w.total; pc += step) {
        // the piece's place: a multiplication per dimension (point_div with the list lengths'
        // reciprocals), the 64-bit division only from 2^32 pieces on
        u64 e;
        u32 x0;
        point_div(pc, ax.ppr, ax.mppr, &e, &x0);
        u64 ti = 0, wi = 0;
        i64 vo = 0;
        u32 fl = OR_VISITS | OR_INSIDE;
#pragma unroll
        for (u32 k = 1; k < ZCG_MAX_DIMS; k++) {
            if (k >= nd) break;
            u32 x;
            point_div(e, w.bs[k], rc.m[k], &e, &x);
            const OrthoRec r = load_rec(recs + ax.off[k] + x);
            ti += r.ti; wi += r.wi; vo += r.vo; fl &= r.flags;
        }
        // 1. the V fast records
        const u64 xe = (u64)x0 * V;
        const u32 rem = w.bs[0] - xe < V ? (u32)(w.bs[0] - xe) : V;
        const OrthoRec* fast = recs + ax.off[0] + xe;
        u64 tj[V], wj[V];
        i64 vj[V];
        u32 fj[V];
#pragma unroll
        for (u32 j = 0; j < V; j++) {
            tj[j] = wj[j] = 0; vj[j] = 0; fj[j] = 0;
            if (j < rem) {
                const OrthoRec r = load_rec(fast + j);
                tj[j] = ti + r.ti; wj[j] = wi + r.wi; vj[j] = vo + r.vo; fj[j] = fl & r.flags;
            }
        }
        // 2. table entries; an element that is not in a chunk of the table has none
        const u8* base[V];
#pragma unroll
        for (u32 j = 0; j < V; j++) base[j] = fj[j] == (OR_VISITS | OR_INSIDE) ? table[tj[j]] : nullptr;
        // 3. elements: loads first, then stores
        u64 v[V];
#pragma unroll
        for (u32 j = 0; j < V; j++) {
            if (DIR) v[j] = base[j] ? load_elem(view + vj[j] * (i64)ES, ES) : 0;
            else v[j] = base[j] ? load_elem(base[j] + wj[j] * ES, ES) : w.fillv;
        }
        if (DIR) {
#pragma unroll
            for (u32 j = 0; j < V; j++)
                if (base[j]) fill_elem((u8*)base[j] + wj[j] * ES, v[j], ES);
            continue;
        }
        // an element is written if it has a source, or with fill unless its chunk is outside the table
        bool whole = rem == V;
        bool has[V];
#pragma unroll
        for (u32 j = 0; j < V; j++) {
            has[j] = j < rem && (base[j] || (w.fill && !((fj[j] & OR_VISITS) && !(fj[j] & OR_INSIDE))));
            whole &= has[j] && vj[j] == vj[0] + (i64)j;
        }
        if (whole) {  // V elements side by side in the view: one 16-byte store
            u64 lo = 0, hi = 0;
#pragma unroll
            for (u32 j = 0; j < V; j++) {
                const u64 bits = ES == 8 ? v[j] : v[j] & ((1ull << (8 * (ES & 7))) - 1);
                if (j * ES < 8) lo |= bits << (8 * (j * ES & 7));
                else hi |= bits << (8 * (j * ES & 7));
            }
            st16(view + vj[0] * (i64)ES, u32x4{(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)});
            continue;
        }
#pragma unroll
        for (u32 j = 0; j < V; j++)
            if (has[j]) fill_elem(view + vj[j] * (i64)ES, v[j], ES);
    }
}

template <u32 DIR>
void launch_walk(u32 grid, hipStream_t s, const RegionWalk& w, const PointRecip& rc, const OrthoAxes& ax,
                 const u8* const* table, const OrthoRec* recs, u8* view) {
    switch (w.es) {
    case 1: hipLaunchKernelGGL((ortho_walk_kernel<DIR, 1>), dim3(grid), dim3(OR_T), 0, s, w, rc, ax, table, recs, view); break;
    case 2: hipLaunchKernelGGL((ortho_walk_kernel<DIR, 2>), dim3(grid), dim3(OR_T), 0, s, w, rc, ax, table, recs, view); break;
    case 4: hipLaunchKernelGGL((ortho_walk_kernel<DIR, 4>), dim3(grid), dim3(OR_T), 0, s, w, rc, ax, table, recs, view); break;
    default: hipLaunchKernelGGL((ortho_walk_kernel<DIR, 8>), dim3(grid), dim3(OR_T), 0, s, w, rc, ax, table, recs, view); break;
    }
}

}  // namespace

// The reset of the nd words (launch_points has the reason for a copy) and two
// launches, whatever the counts are: workgroups stride over the entries and
// over the pieces.
hipError_t launch_ortho(const RegionWalk& w, const BoxTable& bt, const PointRecip& rc, const PointRecip& rcount,
                        const OrthoAxes& ax, const void* const* d_table, void* d_view, void* d_scratch,
                        uint64_t* d_outside, const uint64_t* d_all_ones, uint32_t dir, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(d_outside, d_all_ones, w.nd * sizeof(u64), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    const u64 ag = (ax.off[w.nd] + OR_T - 1) / OR_T;
    hipLaunchKernelGGL(ortho_axis_kernel, dim3((u32)(ag < OR_MAX_GRID ? ag : OR_MAX_GRID)), dim3(OR_T), 0, s, w, bt, rc,
                       ax, (OrthoRec*)d_scratch, (u64*)d_outside);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const u64 wg = (w.total + OR_T - 1) / OR_T;
    const u32 grid = (u32)(wg < OR_MAX_GRID ? wg : OR_MAX_GRID);
    if (dir) launch_walk<1>(grid, s, w, rcount, ax, (const u8* const*)d_table, (const OrthoRec*)d_scratch, (u8*)d_view);
    else launch_walk<0>(grid, s, w, rcount, ax, (const u8* const*)d_table, (const OrthoRec*)d_scratch, (u8*)d_view);
    return hipGetLastError();
}

}  // namespace zcg
