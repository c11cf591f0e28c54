// zcg_region_p.hip — region assembly and scatter for a list of coordinates
// (zcg_read_points, zcg_write_points): numpy's a[i, j, k] with index arrays,
// one element per point.  A point is the box of shape (1, ..., 1) at its
// coordinate (read_ndarray / write_ndarray, ndarray.rs:153-385), so the chunk a
// point visits and what happens when there is none are zcg_read_regions_v's for
// that box (vbox_terms, zcg_region_v.hip); but nothing of a box is built: no
// record, no plan kernel, no work unit.  A lane takes a point, divides its
// coordinate by the chunk extent per dimension and moves one element.
//
// The kernel waits for memory, not for arithmetic: 64 lanes read 64 different
// lines.  A lane therefore holds ZCG_PT_U independent points per iteration,
// and the three dependent reads of a point (coordinate, table entry, element)
// are issued for all of them before the first is used.
#include <hip/hip_runtime.h>

#include "zcg_common.h"
#include "zcg_region_point.h"
#include "zcg_region_walk.h"

namespace zcg {

namespace {

constexpr u32 PT_T = 256;
// points per lane in flight
#ifndef ZCG_PT_U
#define ZCG_PT_U 4
#endif
constexpr u32 PT_MAX_GRID = 1u << 16;

enum : u32 { PT_NONE = 0, PT_CHUNK = 1, PT_OUTSIDE = 2 };

// DIR 0: chunks -> values (gather), 1: values -> chunks (scatter).  Point p's
// value is element order[p] of `vals`, or element p when order is NULL.
template <u32 DIR>
__global__ __launch_bounds__(PT_T) void points_kernel(RegionWalk w, BoxTable bt, PointRecip rc, u64 n,
                                                      const u8* const* __restrict__ table,
                                                      const u64* __restrict__ coords,
                                                      const u64* __restrict__ order, u8* vals,
                                                      u64* __restrict__ first_outside) {
    constexpr u32 U = ZCG_PT_U;
    const u32 nd = w.nd, es = w.es;
    const u64 step = (u64)gridDim.x * PT_T * U;
    u64 outside = ~0ull;  // this lane's lowest point outside the table
    for (u64 b0 = (u64)blockIdx.x * PT_T * U; b0 < n; b0 += step) {
        u64 p[U], ti[U], wi[U];
        u32 state[U];
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            p[u] = b0 + (u64)u * PT_T + threadIdx.x;
            ti[u] = wi[u] = 0;
            state[u] = PT_NONE;
        }
        // 1. coordinates -> table index, element index in the chunk, fate
        u64 c[U][ZCG_MAX_DIMS];
#pragma unroll
        for (u32 u = 0; u < U; u++) {
#pragma unroll
            for (u32 k = 0; k < ZCG_MAX_DIMS; k++)
                if (k < nd && p[u] < n) c[u][k] = coords[p[u] * nd + bt.dim[k]];
        }
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            if (p[u] >= n) continue;
            bool visits = true, inside = true;
#pragma unroll
            for (u32 k = 0; k < ZCG_MAX_DIMS; k++) {
                if (k >= nd) break;
                u64 q;
                u32 rem;
                point_div(c[u][k], w.cs[k], rc.m[k], &q, &rem);
                // the 1-element box's zcg_region_grid range: one chunk when the coordinate is inside the array,
                // or, beyond it, when it is not a multiple of the chunk extent (bounded_coord_iter's ceiling)
                visits &= c[u][k] < bt.as[k] || rem != 0;
                inside &= q >= bt.tlo[k] && q - bt.tlo[k] < bt.tn[k];
                ti[u] += (q - bt.tlo[k]) * w.tstr[k];
                wi[u] += (u64)rem * w.cstr[k];
            }
            state[u] = !visits ? PT_NONE : inside ? PT_CHUNK : PT_OUTSIDE;
            if (state[u] == PT_OUTSIDE && p[u] < outside) outside = p[u];
        }
        // 2. table entries and the values' places
        const u8* base[U];
        u64 j[U];
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            base[u] = state[u] == PT_CHUNK ? table[ti[u]] : nullptr;
            j[u] = order && p[u] < n ? order[p[u]] : p[u];
        }
        // 3. elements: loads first, then stores
        u64 v[U];
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            if (DIR) v[u] = base[u] ? load_elem(vals + j[u] * es, es) : 0;
            else v[u] = base[u] ? load_elem(base[u] + wi[u] * es, es) : w.fillv;
        }
#pragma unroll
        for (u32 u = 0; u < U; u++) {
            if (DIR) { if (base[u]) fill_elem((u8*)base[u] + wi[u] * es, v[u], es); }
            else if (p[u] < n && (base[u] || (w.fill && state[u] != PT_OUTSIDE))) fill_elem(vals + j[u] * es, v[u], es);
        }
    }
    // the lowest point outside the table: a wave reduction, one atomic per wave that has one
    if (__any(outside != ~0ull)) {
#pragma unroll
        for (u32 o = 32; o; o >>= 1) {
            const u64 y = __shfl_xor((unsigned long long)outside, o, 64);
            outside = y < outside ? y : outside;
        }
        if ((threadIdx.x & 63) == 0) atomicMin((unsigned long long*)first_outside, (unsigned long long)outside);
    }
}

}  // namespace

// One reset of the word and one launch whatever n is: workgroups stride over
// the points.  The reset is an 8-byte device-to-device copy of UINT64_MAX, not
// a memset: on the MI355X a memset node of a captured graph wrote 0 instead of
// its fill byte from the second replay on (the atomic minimum then kept the
// 0), while a copy node names only its two addresses.
hipError_t launch_points(const RegionWalk& w, const BoxTable& bt, const PointRecip& rc, uint64_t n,
                         const void* const* d_table, const uint64_t* d_coords, const uint64_t* d_order, void* d_vals,
                         uint64_t* d_first_outside, const uint64_t* d_all_ones, uint32_t dir, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemcpyAsync(d_first_outside, d_all_ones, sizeof(u64), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    const u64 per = (u64)PT_T * ZCG_PT_U, groups = (n + per - 1) / per;
    const u32 grid = (u32)(groups < PT_MAX_GRID ? groups : PT_MAX_GRID);
    hipLaunchKernelGGL(dir ? points_kernel<1> : points_kernel<0>, dim3(grid), dim3(PT_T), 0, s, w, bt, rc, (u64)n,
                       (const u8* const*)d_table, (const u64*)d_coords, (const u64*)d_order, (u8*)d_vals,
                       (u64*)d_first_outside);
    return hipGetLastError();
}

}  // namespace zcg
