// zcg_chains.h — the match-finder front end shared by the gzip and xz encoders
// (zcg_chains.hip).  A coder's own key kernel writes one (chunk id | hash,
// position) pair per position of a sub-batch; a stable radix sort groups the
// pairs by key with ascending positions; chain_links turns each group into a
// hash chain.  The key and search kernels stay with their coders.
#pragma once
#include "zcg_common.h"
#include "zcg_encode_plan.h"

namespace zcg {
// radix-sort scratch bytes for `tot` (key, position) pairs
u64 sort_pairs_scratch(u64 tot);
// Workspace offsets of the front end's buffers for sub-batches of up to `tot`
// positions: the sort's double buffers and scratch and (links) the chain links.
struct ChainWs { u64 ka, kb, va, vb, cub, cub_bytes, prev; };
ChainWs carve_chain_ws(WsCarve& ws, u64 tot, bool links);
// Stable sort of `tot` pairs by key bits [0, end_bit): keys in ka, values in va,
// (kb, vb) the alternate buffers; *keys_out / *vals_out hold the result.
hipError_t sort_pairs_u32(void* scratch, u64 scratch_bytes, u32* ka, u32* kb, u32* va, u32* vb, u64 tot, u32 end_bit,
                          hipStream_t s, u32** keys_out, u32** vals_out);
// prev[vals[j]] = vals[j - 1] where keys[j] == keys[j - 1], else 0xFFFFFFFF
hipError_t launch_chain_links(u64 tot, const u32* keys, const u32* vals, u32* prev, hipStream_t s);
}  // namespace zcg
