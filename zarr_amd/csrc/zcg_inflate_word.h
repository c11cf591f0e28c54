// zcg_inflate_word.h — the parts of the gzip member frame that are plain
// arithmetic on words: the serial table entry, the token word of the parallel
// kernels, the wave kernel's token-ready table entries, and zlib's look-ahead
// window.  Host/device C++ with no HIP include, so tests/hostcore compiles it
// with g++ and the CPU suite checks it exhaustively.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define ZI_INL __host__ __device__ __forceinline__
#else
#define ZI_INL inline __attribute__((always_inline))
#endif

namespace zcg {

typedef uint32_t u32;
typedef uint64_t u64;

// ---- serial table entry (build_table, zcg_inflate_common.h) -----------------------
// [31:28] code length | [27:24] kind | [23:16] extra bits | [15:0] value
//        K_SUB: [23:16] subtable bits, [15:0] subtable offset (code length 0)
enum : u32 { K_LIT = 0, K_LEN = 1, K_EOB = 2, K_BAD = 3, K_DIST = 4, K_SUB = 5 };
ZI_INL u32 mk_entry(u32 len, u32 kind, u32 extra, u32 val) {
    return (len << 28) | (kind << 24) | (extra << 16) | val;
}

// ---- token word (the 256-lane and the wave kernel) -----------------------------------
//   literal  = bits << 24 | byte
//   match    = 1 << 31 | bits << 24 | (len - 3) << 16 | (dist - 1)
//   marker   = 1 << 30 | bits << 24 | code   (EOB / invalid code / input exhausted)
// bits = the token's stream bits (<= 48), so a token's start is the lane's
// segment start plus the bits of the tokens before it in the lane's list.
// (The 256-lane kernel's markers carry bits = 0: it takes positions from the
// lane that stopped.)
constexpr u32 W_MATCH = 0x80000000u;
constexpr u32 W_MARK = 0x40000000u;
enum : u32 { M_EOB = 0, M_BAD = 1, M_EXH = 2, M_END = 3 /* synthetic: no more tokens in the round */ };
constexpr u32 W_EOB = W_MARK | M_EOB, W_BAD = W_MARK | M_BAD, W_EXH = W_MARK | M_EXH;
ZI_INL bool w_marker(u32 t) { return (t & 0xC0000000u) == W_MARK; }
ZI_INL u32 w_bits(u32 t) { return (t >> 24) & 63; }
ZI_INL u32 w_dist(u32 t) { return (t & 0x7FFF) + 1; }
// output bytes of a token (a marker has none); w_len_tok: of a word known to be
// a literal or a match
ZI_INL u32 w_len_tok(u32 t) { return (t & W_MATCH) ? ((t >> 16) & 0xFF) + 3 : 1u; }
ZI_INL u32 w_len(u32 t) { return (t & W_MATCH) ? ((t >> 16) & 0xFF) + 3 : (w_marker(t) ? 0u : 1u); }

// ---- token-ready table entries (the wave kernel) ------------------------------------------
// build_table lays entries out for the serial reader, and a token word would
// have to be put together from those fields once per token.  After the header
// of a Huffman block the wave kernel rewrites both tables in place into a
// layout of its own, tagged like a token word by bits 31:30:
//   ltab  literal   l << 24 | byte                          (the token word)
//         EOB / bad W_MARK | l << 24 | M_EOB / M_BAD        (the token word)
//         length    W_MATCH | (l + ex) << 24 | (base - 3) << 16 | ex << 8 | l
//         link      T_SUB | offset << 8 | subtable bits
//   dtab  distance  (dl + dex) << 24 | dex << 20 | dl << 16 | (base - 1)
//         bad       W_MARK | dl << 24 | M_BAD
//         link      as above
// Every reachable entry of the serial layout has exactly one image (literals
// carry no extra bits and a value < 256, a code length is >= 1 except on a
// link, base - 3 + extra <= 255, base - 1 < 2^15), so the *_serial maps give
// the serial entries back exactly: zlib's look-ahead decodes with these same
// tables in the serial layout when the output fills inside a block.
// tests/test_hostcore.py walks every reachable entry.
constexpr u32 T_SUB = 0xC0000000u;
ZI_INL u32 iw_l_wave(u32 e) {
    const u32 l = e >> 28, kind = (e >> 24) & 15, ex = (e >> 16) & 0xFF, val = e & 0xFFFF;
    if (kind == K_LIT) return (l << 24) | (val & 0xFF);
    if (kind == K_EOB) return W_MARK | (l << 24) | M_EOB;
    if (kind == K_LEN) return W_MATCH | ((l + ex) << 24) | (((val - 3) & 0xFF) << 16) | ((ex & 7) << 8) | l;
    if (kind == K_SUB) return T_SUB | (val << 8) | (ex & 31);
    return W_MARK | (l << 24) | M_BAD;
}
ZI_INL u32 iw_l_serial(u32 x) {
    const u32 tag = x >> 30, l = (x >> 24) & 15;
    if (tag == 0) return mk_entry(l, K_LIT, 0, x & 0xFF);
    if (tag == 1) return mk_entry(l, (x & 3) == M_EOB ? K_EOB : K_BAD, 0, 0);
    if (tag == 2) return mk_entry(x & 15, K_LEN, (x >> 8) & 7, ((x >> 16) & 0xFF) + 3);
    return mk_entry(0, K_SUB, x & 31, (x >> 8) & 0xFFFF);
}
ZI_INL u32 iw_d_wave(u32 e) {
    const u32 l = e >> 28, kind = (e >> 24) & 15, ex = (e >> 16) & 0xFF, val = e & 0xFFFF;
    if (kind == K_DIST) return ((l + ex) << 24) | ((ex & 15) << 20) | (l << 16) | ((val - 1) & 0x7FFF);
    if (kind == K_SUB) return T_SUB | (val << 8) | (ex & 31);
    return W_MARK | (l << 24) | M_BAD;
}
ZI_INL u32 iw_d_serial(u32 x) {
    const u32 tag = x >> 30;
    if (tag == 0) return mk_entry((x >> 16) & 15, K_DIST, (x >> 20) & 15, (x & 0x7FFF) + 1);
    if (tag == 1) return mk_entry((x >> 24) & 15, K_BAD, 0, 0);
    return mk_entry(0, K_SUB, x & 31, (x >> 8) & 0xFFFF);
}

// ---- zlib's look-ahead window ------------------------------------------------------------
// After the output is full zlib goes on validating with the input it was
// given, which is the rest of flate2's current 32 KiB BufReader window: the
// window of the member's bytes that holds the last consumed bit.  h = gzip
// header bytes, consumed = deflate-stream bits consumed, n_in = member bytes.
// Returns the deflate-stream bit the look-ahead may read up to.
ZI_INL u64 inf_lookahead_limit(u64 h, u64 consumed, u64 n_in) {
    const u64 last_byte = h + (consumed ? (consumed - 1) / 8 : 0);
    u64 wend = (last_byte / 32768 + 1) * 32768;
    if (wend > n_in) wend = n_in;
    return (wend - h) * 8;
}

}  // namespace zcg
