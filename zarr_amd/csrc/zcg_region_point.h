// zcg_region_point.h — what the kernels that address single elements share
// (zcg_region_p.hip: a list of coordinates; zcg_region_o.hip: an index list
// per dimension): one element's load, and the division of a coordinate by the
// chunk extent.
#pragma once

#include "zcg_common.h"

namespace zcg {

namespace {

__device__ __forceinline__ u64 load_elem(const u8* src, u32 es) {
    switch (es) {
    case 1: return *src;
    case 2: return *(const u16*)src;
    case 4: return *(const u32*)src;
    default: return *(const u64*)src;
    }
}

// c / cs and c % cs.  A coordinate below 2^32 (every coordinate inside an
// array whose extents are below 2^32) is divided by a multiplication with
// m = ceil(2^64 / cs), which the host precomputes: the high 64 bits of c * m
// are the exact quotient for any 32-bit c and any cs in 2 .. 2^32-1 (64
// fraction bits >= 32 + log2 cs).  Any other coordinate takes the 64-bit
// division; lanes of one wave may differ.
__device__ __forceinline__ void point_div(u64 c, u32 cs, u64 m, u64* q, u32* rem) {
    if ((c >> 32) == 0) {
        const u32 c32 = (u32)c;
        const u32 q32 = cs == 1 ? c32 : (u32)(((u64)c32 * (u32)(m >> 32) + __umulhi(c32, (u32)m)) >> 32);
        *q = q32;
        *rem = c32 - q32 * cs;
    } else {
        const u64 q64 = c / cs;
        *q = q64;
        *rem = (u32)(c - q64 * cs);
    }
}

}  // namespace

}  // namespace zcg
