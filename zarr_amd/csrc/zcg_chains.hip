// zcg_chains.hip — the encoders' shared match-finder front end (zcg_chains.h):
// the hipCUB radix sort of (key, position) pairs and the chain-link kernel.
#include <hipcub/hipcub.hpp>

#include "zcg_chains.h"

namespace zcg {

u64 sort_pairs_scratch(u64 tot) {
    size_t cb = 0;
    hipcub::DoubleBuffer<u32> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, cb, k, v, (int)(tot ? tot : 1), 0, 32);
    return (cb + 511) & ~255ull;
}

ChainWs carve_chain_ws(WsCarve& ws, u64 tot, bool links) {
    ChainWs c{};
    c.ka = ws.take(4 * tot);
    c.kb = ws.take(4 * tot);
    c.va = ws.take(4 * tot);
    c.vb = ws.take(4 * tot);
    c.cub_bytes = sort_pairs_scratch(tot);
    c.cub = ws.take(c.cub_bytes);
    if (links) c.prev = ws.take(4 * tot);
    return c;
}

hipError_t sort_pairs_u32(void* scratch, u64 scratch_bytes, u32* ka, u32* kb, u32* va, u32* vb, u64 tot, u32 end_bit,
                          hipStream_t s, u32** keys_out, u32** vals_out) {
    hipcub::DoubleBuffer<u32> dk(ka, kb), dv(va, vb);
    size_t cb = scratch_bytes;
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(scratch, cb, dk, dv, (int)tot, 0, (int)end_bit, s);
    *keys_out = dk.Current();
    *vals_out = dv.Current();
    return e;
}

__global__ void chain_links(u64 tot, const u32* __restrict__ keys, const u32* __restrict__ vals,
                            u32* __restrict__ prev) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= tot) return;
    prev[vals[j]] = (j > 0 && keys[j] == keys[j - 1]) ? vals[j - 1] : 0xFFFFFFFFu;
}

hipError_t launch_chain_links(u64 tot, const u32* keys, const u32* vals, u32* prev, hipStream_t s) {
    hipLaunchKernelGGL(chain_links, dim3((u32)((tot + 255) / 256)), dim3(256), 0, s, tot, keys, vals, prev);
    return hipGetLastError();
}

}  // namespace zcg
