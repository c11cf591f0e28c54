// zcg_region_walk.h — what the region assembly kernels share (zcg_region.hip:
// one box per launch; zcg_regions.hip: many boxes per launch): the workgroup
// size, the pieces-per-lane tunable, the per-lane box position and the
// per-element copies of the run path.
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

}  // namespace zcg
