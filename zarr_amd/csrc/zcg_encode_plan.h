// zcg_encode_plan.h — host-side planning shared by the encoders: the workspace
// carve and the batch sizing of the match-finder front end.  Plain C++17 with
// no HIP include (tests/hostcore compiles it with g++).
#pragma once
#include <stdint.h>

namespace zcg {

// Bump allocator over a workspace: every region starts on a 256-byte boundary.
struct WsCarve {
    uint64_t p = 0;
    uint64_t take(uint64_t bytes) {
        const uint64_t o = p;
        p = (p + bytes + 255) & ~255ull;
        return o;
    }
    uint64_t total() const { return p; }
};

// Chunks of D input bytes go through a coder in super-batches of sm chunks (one
// coder launch, the match results kept for all of them) and through its match
// finder in sub-batches of m chunks = tot positions (one sort).  m: sub_bytes of
// input and at most max_m chunks (the chunk id shares the 32-bit sort key with
// the hash); sm: super_bytes of input, a multiple of m.
struct SubBatch {
    uint32_t m, sm;
    uint64_t tot;
};
inline SubBatch sub_batch_plan(uint64_t D, uint32_t n, uint64_t sub_bytes, uint64_t super_bytes, uint32_t max_m) {
    uint64_t m = D ? sub_bytes / D : n;
    if (m < 1) m = 1;
    if (m > n) m = n;
    if (m > max_m) m = max_m;
    uint64_t sm = D ? super_bytes / D : n;
    sm = sm / m * m;
    if (sm < m) sm = m;
    if (sm > n) sm = n;
    return SubBatch{(uint32_t)m, (uint32_t)sm, m * D};
}
// chunks of the batch [at, at + step) that lie before `end`
inline uint32_t batch_count(uint32_t at, uint32_t end, uint32_t step) { return end - at < step ? end - at : step; }
// bits that hold 0 .. cnt-1 (the chunk id's share of a sort key)
inline uint32_t id_bits(uint32_t cnt) {
    uint32_t b = 0;
    while ((1u << b) < cnt) b++;
    return b;
}

}  // namespace zcg
