// zcg_inflate_common.h — RFC 1951 / gzip machinery shared by the serial
// (zcg_inflate.hip), 256-lane (zcg_inflate_par.hip) and wave
// (zcg_inflate_wave.hip) inflate kernels: Huffman tables in LDS, the
// wave-uniform bit reader, and the gzip MEMBER FRAME that all three run their
// own block loops inside (and its zlib counterpart, RFC 1950: another header
// and trailer around the same deflate body, picked by inf_open's and
// inf_close's `zlib` argument):
//   inf_open           guards, flate2's gzip (zlib's) header rules -> InfMember
//   read_block_header  BFINAL/BTYPE, stored lengths, fixed tables; the dynamic
//                      header reader is the kernel's own (a parameter)
//   inf_stored_copy    a stored block through a kernel's stage (256-lane, wave)
//   stage_commit       a stage of 16-bit entries -> dst, byte order fused
//   inf_close          zlib's post-N look-ahead, result -> status
// The word-level parts (table entry, token word, look-ahead window) are in
// zcg_inflate_word.h, which the CPU suite also compiles.
#pragma once
#include "zcg_common.h"
#include "zcg_inflate_word.h"

namespace zcg {


constexpr int INF_LBITS = 10;  // literal/length root table bits
constexpr int INF_DBITS = 8;   // distance root table bits
constexpr u32 INF_LTAB = 1536; // root 1024 + subtables (zlib enough(286,10,15) = 1334)
constexpr u32 INF_DTAB = 512;  // root 256 + subtables (enough(30,8,15) = 402)
constexpr u32 INF_RING = 32768;
constexpr u32 INF_FLUSH = 16384;

// Two-level tables: every code decodes in <= 2 LDS lookups (no bit-serial
// path: a rare per-lane slow path would stall whole 64-lane waves).  The entry
// layout (mk_entry, K_*) is in zcg_inflate_word.h.

__constant__ u16 c_len_base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ u8 c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2,
                                   2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ u16 c_dist_base[30] = {1,    2,    3,    4,    5,    7,     9,     13,    17,  25,
                                    33,   49,   65,   97,   129,  193,   257,   385,   513, 769,
                                    1025, 1537, 2049, 3073, 4097, 6145,  8193,  12289, 16385,
                                    24577};
__constant__ u8 c_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2,  3,  3,  4,  4,  5,  5,  6,
                                    6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ u8 c_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Canonical Huffman code description in LDS (built per block).
struct HuffLds {
    u32 count[16];
    u32 first[16];     // first canonical code of each length
    u32 cpre[5 * 16];  // per 64-symbol chunk: codes of each length in earlier chunks
};

// Entry for symbol `s` of table type `dist`.
__device__ __forceinline__ u32 sym_entry(u32 s, u32 len, bool dist) {
    if (!dist) {
        if (s < 256) return mk_entry(len, K_LIT, 0, s);
        if (s == 256) return mk_entry(len, K_EOB, 0, 0);
        if (s <= 285) return mk_entry(len, K_LEN, c_len_extra[s - 257], c_len_base[s - 257]);
        return mk_entry(len, K_BAD, 0, 0);
    }
    if (s < 30) return mk_entry(len, K_DIST, c_dist_extra[s], c_dist_base[s]);
    return mk_entry(len, K_BAD, 0, 0);
}

__device__ __forceinline__ u32 bitrev(u32 v, int n) { return __builtin_bitreverse32(v) >> (32 - n); }
// popcount of the mask bits below this lane
__device__ __forceinline__ u32 mbcnt64(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
}

// Build the canonical code and the two-level table from lens[0..nsym)
// (nsym <= 320; block-cooperative: every thread of the workgroup calls this
// uniformly).  Symbol-driven, like zlib's inflate_table: a symbol's rank among
// the codes of its length comes from wave ballots, a short code fills its
// 2^(root-L) root slots, each long-code prefix gets a subtable sized by its
// longest code (atomicMax) and placed by a block scan.  `cap` = table entries.
// Returns 0 ok, -1 over-subscribed or incomplete (zlib inflate_table rules:
// an incomplete code is only allowed when it is a single length-1 code).
__device__ int build_table(const u8* lens, u32 nsym, HuffLds* h, u32* table, int root, bool dist,
                           u32 cap) {
    const u32 tid = threadIdx.x, nth = blockDim.x;
    const u32 lane = tid & 63, wv = tid >> 6, nwv = nth >> 6;
    const u32 nchunk = (nsym + 63) >> 6;
    const u32 nroot = 1u << root;
    __shared__ u32 s_part[256 / 64 + 1];
    __syncthreads();
    // 1. per-chunk counts of each code length; rank of my symbol in its chunk
    constexpr u32 MAXC = 5;
    u32 myL[MAXC], myR[MAXC];
#pragma unroll
    for (u32 i = 0; i < MAXC; i++) {
        const u32 c = wv + i * nwv;
        myL[i] = 0;
        myR[i] = 0;
        if (c < nchunk) {
            const u32 s = c * 64 + lane;
            const u32 L = s < nsym ? lens[s] : 0;
            myL[i] = L;
            for (u32 l = 1; l < 16; l++) {
                const unsigned long long m = __ballot(L == l);
                if (L == l) myR[i] = mbcnt64(m);
                if (lane == 0) h->cpre[c * 16 + l] = (u32)__popcll(m);
            }
        }
    }
    for (u32 k = tid; k < nroot; k += nth) table[k] = 0;
    __syncthreads();
    if (tid < 16) {  // exclusive prefix over chunks, totals
        u32 acc = 0;
        if (tid > 0)
            for (u32 c = 0; c < nchunk; c++) {
                const u32 v = h->cpre[c * 16 + tid];
                h->cpre[c * 16 + tid] = acc;
                acc += v;
            }
        h->count[tid] = acc;
    }
    __syncthreads();
    int ok = 1, maxlen = 0;
    {
        int left = 1;
        for (int l = 1; l <= 15; l++) {
            left <<= 1;
            left -= (int)h->count[l];
            if (left < 0) ok = 0;  // over-subscribed
            if (h->count[l]) maxlen = l;
        }
        if (ok && left > 0 && maxlen > 1) ok = 0;
    }
    if (tid == 0) {
        u32 f = 0;
        for (int l = 1; l < 16; l++) {
            f = (f + h->count[l - 1]) << 1;
            h->first[l] = f;
        }
    }
    __syncthreads();
    if (!ok) return -1;
    u32 rev[MAXC];
#pragma unroll
    for (u32 i = 0; i < MAXC; i++) {
        const u32 c = wv + i * nwv, L = myL[i];
        rev[i] = 0;
        if (L) rev[i] = bitrev(h->first[L] + h->cpre[c * 16 + L] + myR[i], (int)L);
    }
    // 2. subtable size of each long-code prefix
    if (maxlen > root) {
#pragma unroll
        for (u32 i = 0; i < MAXC; i++)
            if (myL[i] > (u32)root) atomicMax(&table[rev[i] & (nroot - 1)], myL[i] - root);
        __syncthreads();
    }
    // 3. root slots: subtable heads (placed by a block scan) or invalid
    const u32 per = (nroot + nth - 1) / nth;  // contiguous slots per thread
    u32 mysum = 0;
    for (u32 k = 0; k < per; k++) {
        const u32 slot = tid * per + k;
        if (slot < nroot && table[slot]) mysum += 1u << table[slot];
    }
    u32 x = mysum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d, 64);
        if ((int)lane >= d) x += y;
    }
    if (lane == 63) s_part[wv] = x;
    __syncthreads();
    u32 off = nroot, tot = 0;
    for (u32 w = 0; w < nwv; w++) {
        const u32 v = s_part[w];
        if (w < wv) off += v;
        tot += v;
    }
    off += x - mysum;
    for (u32 k = 0; k < per; k++) {
        const u32 slot = tid * per + k;
        if (slot >= nroot) break;
        const u32 sb = table[slot];
        table[slot] = sb ? mk_entry(0, K_SUB, sb, off) : mk_entry(1, K_BAD, 0, 0);
        off += sb ? (1u << sb) : 0u;
    }
    __syncthreads();
    if (nroot + tot > cap) return -1;  // cannot happen for a complete code (zlib ENOUGH)
    // 4. fill: short codes into the root, long codes into their subtable
#pragma unroll
    for (u32 i = 0; i < MAXC; i++) {
        const u32 L = myL[i];
        if (!L) continue;
        const u32 s = (wv + i * nwv) * 64 + lane;
        const u32 e = sym_entry(s, L, dist);
        if (L <= (u32)root) {
            for (u32 k = rev[i]; k < nroot; k += 1u << L) table[k] = e;
        } else {
            const u32 te = table[rev[i] & (nroot - 1)];
            const u32 base = te & 0xFFFF, sb = (te >> 16) & 0xFF;
            for (u32 k = rev[i] >> root; k < (1u << sb); k += 1u << (L - root)) table[base + k] = e;
        }
    }
    __syncthreads();
    return 0;
}

// Look up a symbol from >= 15 stream bits `v` (two levels).
__device__ __forceinline__ u32 table_lookup(const u32* tab, int root, u32 v) {
    u32 e = tab[v & ((1u << root) - 1)];
    if (((e >> 24) & 15) == K_SUB) e = tab[(e & 0xFFFF) + ((v >> root) & ((1u << ((e >> 16) & 0xFF)) - 1))];
    return e;
}

// Wave-uniform bit reader (every lane holds the same state).  Input words
// come from a 256-byte LDS cache that the whole wave refills with one
// coalesced load, so a refill costs an LDS read, not a global round trip.
constexpr u32 BI_CACHE_WORDS = 64;
struct BitIn {
    const u8* src;
    u64 n;        // input bytes
    u64 pos;      // next byte to load into the buffer (multiple of 4)
    u64 buf;      // bit buffer (LSB = next bit)
    u32 cnt;      // valid bits in buf
    u64 consumed; // bits consumed from the stream start
    u64 limit;    // bits that may be consumed (input end, or look-ahead window end)
    u32* cache;   // LDS [BI_CACHE_WORDS]
    u64 cbase;    // byte offset of cache[0]
};

__device__ __forceinline__ void bi_init(BitIn& b, const u8* src, u64 n, u32* cache) {
    b.src = src; b.n = n; b.pos = 0; b.buf = 0; b.cnt = 0; b.consumed = 0; b.limit = n * 8;
    b.cache = cache; b.cbase = ~0ull;
}

// Little-endian load of sizeof(W) = 4, 8 or 16 bytes at src + q from a buffer
// of n bytes: the whole word when it fits, else the bytes that exist (the rest
// read as 0).  W is the unaligned word view in src's address space (u32_ua,
// gu64_ua, u32x4_ua ...); the result is u32, u64 or u32x4.
template <class W, class B>
__device__ __forceinline__ auto ld_tail(const B* src, u64 q, u64 n) {
    constexpr u32 NB = sizeof(W);
    static_assert(NB == 4 || NB == 8 || NB == 16, "word size");
    if constexpr (NB == 4) {
        u32 w = 0;
        if (q + 4 <= n) w = *(const W*)(src + q);
        else
            for (u32 i = 0; i < 4; i++)
                if (q + i < n) w |= (u32)src[q + i] << (8 * i);
        return w;
    } else if constexpr (NB == 8) {
        const bool whole = q + 8 <= n;
        u64 w = 0;
        if (!whole)
            for (u32 i = 0; i < 8; i++)
                if (q + i < n) w |= (u64)src[q + i] << (8 * i);
        if (whole) w = *(const W*)(src + q);
        return w;
    } else {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (q + 16 <= n) w = *(const W*)(src + q);
        else {
            u64 lo = 0, hi = 0;
            for (u32 i = 0; i < 16; i++)
                if (q + i < n) {
                    const u64 b8 = (u64)src[q + i] << (8 * (i & 7));
                    if (i < 8) lo |= b8; else hi |= b8;
                }
            w = u32x4{(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
        }
        return w;
    }
}

__device__ __forceinline__ u32 bi_word(BitIn& b, u64 pos) {
    if (pos < b.cbase || pos + 4 > b.cbase + 4 * BI_CACHE_WORDS) {
        const int lane = lane_id();
        const u32 w = ld_tail<u32_ua>(b.src, pos + 4 * (u64)lane, b.n);
        __builtin_amdgcn_wave_barrier();
        b.cache[lane] = w;
        __builtin_amdgcn_wave_barrier();
        b.cbase = pos;
    }
    return __builtin_amdgcn_readfirstlane(b.cache[(pos - b.cbase) >> 2]);
}

__device__ __forceinline__ void bi_refill(BitIn& b) {
    if (b.cnt <= 32) {
        const u32 w = bi_word(b, b.pos);
        b.buf |= (u64)w << b.cnt;
        b.cnt += 32;
        b.pos += 4;
    }
}

// Position the reader at absolute stream bit `bit`.
__device__ __forceinline__ void bi_seek(BitIn& b, u64 bit) {
    b.pos = (bit >> 5) << 2;
    b.buf = 0;
    b.cnt = 0;
    b.consumed = bit & ~31ull;
    bi_refill(b);
    const u32 drop = (u32)(bit & 31);
    b.buf >>= drop;
    b.cnt -= drop;
    b.consumed += drop;
}

__device__ __forceinline__ bool bi_has(const BitIn& b, u32 k) { return b.consumed + k <= b.limit; }
__device__ __forceinline__ u32 bi_peek(BitIn& b, u32 k) { return (u32)(b.buf & ((1ull << k) - 1)); }
__device__ __forceinline__ void bi_drop(BitIn& b, u32 k) {
    b.buf >>= k;
    b.cnt -= k;
    b.consumed += k;
}
__device__ __forceinline__ u32 bi_bits(BitIn& b, u32 k) {  // k <= 32
    bi_refill(b);
    u32 v = bi_peek(b, k);
    bi_drop(b, k);
    return v;
}

struct InfOut {
    u8* ring;   // LDS ring [INF_RING]
    u64 P;      // logical bytes produced
    u64 F;      // logical bytes flushed to dst
    u8* dst;
    u64 D;
    DType t;
};

// Flush [F, upto) (upto element-aligned or == D) from the ring to dst.
__device__ void inf_flush(InfOut& o, u64 upto) {
    const int lane = lane_id();
    __syncthreads();
    const u64 F = o.F;
    for (u64 p = F + (u64)lane * 16; p < upto; p += 64 * 16) {
        if (p + 16 <= upto) {
            const u32 r = (u32)(p & (INF_RING - 1));  // 16-aligned, never wraps mid-vector
            u32x4 v = *(const u32x4*)(o.ring + r);
            st16(o.dst + p, transform16(v, o.t));
        } else {
            for (u64 q = p; q < upto; q++)
                o.dst[swap_pos(q, o.t)] = norm_byte(o.ring[q & (INF_RING - 1)], o.t);
        }
    }
    o.F = upto;
    __syncthreads();
}

__device__ __forceinline__ void inf_maybe_flush(InfOut& o) {
    if (o.P - o.F >= INF_FLUSH) inf_flush(o, o.F + INF_FLUSH);
}

__device__ __forceinline__ void put_lit(InfOut& o, u32 byte) {
    if (lane_id() == 0) o.ring[o.P & (INF_RING - 1)] = (u8)byte;
    o.P++;
}

__device__ __forceinline__ void put_match(InfOut& o, u32 len, u32 dist) {
    const int lane = lane_id();
    const u32 m = dist < 64 ? dist : 64;
    const u64 P = o.P;
    for (u32 base = 0; base < len; base += m) {
        const u32 k = base + lane;
        if ((u32)lane < m && k < len) {
            const u64 q = P + k;
            o.ring[q & (INF_RING - 1)] = o.ring[(q - dist) & (INF_RING - 1)];
        }
        __builtin_amdgcn_wave_barrier();
    }
    o.P = P + len;
}

// Result of a bit-level step: ok, ran out of bits (EOF in the main decode,
// "zlib waits for input" in the look-ahead), or corrupt.
enum : int { R_OK = 0, R_EXHAUSTED = 1, R_INVALID = 2 };

// Decode one symbol (two-level table) with the wave-uniform reader.
__device__ __forceinline__ int decode_sym(BitIn& b, const u32* tab, int root, u32* out) {
    bi_refill(b);
    const u32 e = __builtin_amdgcn_readfirstlane(table_lookup(tab, root, bi_peek(b, 15)));
    const u32 l = e >> 28;
    if (!bi_has(b, l)) return R_EXHAUSTED;
    if (((e >> 24) & 15) == K_BAD) return R_INVALID;
    bi_drop(b, l);
    *out = e;
    return R_OK;
}

// Table geometry: literal/length root bits + table capacity, distance root
// bits + capacity (defaults: the serial and 256-lane kernels' 10/8-bit roots).
// Dynamic block header (RFC 1951 3.2.7) -> tables; zlib's validity rules.
template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB>
__device__ __attribute__((always_inline)) int read_dynamic(BitIn& b, u8* lens, HuffLds* lh, u32* ltab, HuffLds* dh, u32* dtab) {
    const u32 tid = threadIdx.x, nth = blockDim.x;
    if (!bi_has(b, 14)) return R_EXHAUSTED;
    const u32 nlen = bi_bits(b, 5) + 257, ndist = bi_bits(b, 5) + 1, ncode = bi_bits(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return R_INVALID;  // "too many length or distance symbols"
    u8 cl[19];
    for (int i = 0; i < 19; i++) cl[i] = 0;
    if (!bi_has(b, 3 * ncode)) return R_EXHAUSTED;
    for (u32 i = 0; i < ncode; i++) cl[c_clen_order[i]] = (u8)bi_bits(b, 3);
    {  // code-length code must be complete ("invalid code lengths set")
        u32 cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 19; i++) cnt[cl[i]]++;
        int left = 1;
        for (int l = 1; l <= 7; l++) { left <<= 1; left -= cnt[l]; if (left < 0) break; }
        if (left != 0) return R_INVALID;
    }
    __syncthreads();
    for (u32 i = tid; i < 19; i += nth) lens[i] = cl[i];
    __syncthreads();
    build_table(lens, 19, lh, ltab, 7, false, LCAP);
    u32 idx = 0;
    u8 prev = 0;
    while (idx < nlen + ndist) {
        u32 e;
        int r = decode_sym(b, ltab, 7, &e);
        if (r != R_OK) return r;
        const u32 sym = e & 0xFFFF;
        if (sym < 16) {
            if (tid == 0) lens[idx] = (u8)sym;
            prev = (u8)sym;
            idx++;
            continue;
        }
        u32 rep;
        u8 v = 0;
        if (sym == 16) {
            if (idx == 0) return R_INVALID;  // "invalid bit length repeat"
            if (!bi_has(b, 2)) return R_EXHAUSTED;
            v = prev;
            rep = 3 + bi_bits(b, 2);
        } else if (sym == 17) {
            if (!bi_has(b, 3)) return R_EXHAUSTED;
            rep = 3 + bi_bits(b, 3);
        } else {
            if (!bi_has(b, 7)) return R_EXHAUSTED;
            rep = 11 + bi_bits(b, 7);
        }
        if (idx + rep > nlen + ndist) return R_INVALID;
        if (tid < 64)
            for (u32 k = tid; k < rep; k += 64) lens[idx + k] = v;
        idx += rep;
        prev = v;
    }
    __syncthreads();
    u8 dl = 0;
    if (tid < ndist) dl = lens[nlen + tid];
    __syncthreads();
    for (u32 i = nlen + tid; i < 288; i += nth) lens[i] = 0;
    if (tid < 32) lens[288 + tid] = tid < ndist ? dl : 0;
    __syncthreads();
    if (lens[256] == 0) return R_INVALID;  // "invalid code -- missing end-of-block"
    if (build_table(lens, 288, lh, ltab, LB, false, LCAP) != 0) return R_INVALID;
    if (build_table(lens + 288, 30, dh, dtab, DB, true, DCAP) != 0) return R_INVALID;
    return R_OK;
}

template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB>
__device__ void fixed_tables(u8* lens, HuffLds* lh, u32* ltab, HuffLds* dh, u32* dtab) {
    const u32 tid = threadIdx.x, nth = blockDim.x;
    __syncthreads();
    for (u32 i = tid; i < 320; i += nth)
        lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
    __syncthreads();
    build_table(lens, 288, lh, ltab, LB, false, LCAP);
    // all 32 five-bit distance codes (30 and 31 decode as invalid), as zlib
    // builds the fixed table: the 30-symbol code alone would be incomplete
    build_table(lens + 288, 32, dh, dtab, DB, true, DCAP);
}

// Block header: 3 bits, then stored-length check / table construction.
// *type receives BTYPE; for stored blocks *slen the LEN field.  A dynamic
// header is read by `dyn(b)`, the calling kernel's own reader (read_dynamic
// above, or its block- or wave-parallel restatement: same rules, same result).
template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB, class Dyn>
__device__ __attribute__((always_inline)) int read_block_header(BitIn& b, bool* last, u32* type, u32* slen, u8* lens, HuffLds* lh,
                                 u32* ltab, HuffLds* dh, u32* dtab, Dyn dyn) {
    if (!bi_has(b, 3)) return R_EXHAUSTED;
    const u32 hdr = bi_bits(b, 3);
    *last = hdr & 1;
    *type = hdr >> 1;
    if (*type == 0) {
        const u32 pad = (u32)((8 - (b.consumed & 7)) & 7);  // to byte boundary
        if (!bi_has(b, pad + 32)) return R_EXHAUSTED;
        bi_bits(b, pad);
        const u32 len = bi_bits(b, 16), nlen = bi_bits(b, 16);
        if ((len ^ 0xFFFF) != nlen) return R_INVALID;  // "invalid stored block lengths"
        *slen = len;
        return R_OK;
    }
    if (*type == 3) return R_INVALID;  // "invalid block type"
    if (*type == 1) { fixed_tables<LB, LCAP, DB, DCAP>(lens, lh, ltab, dh, dtab); return R_OK; }
    return dyn(b);
}
// ... with the serial dynamic-header reader
template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB>
__device__ __attribute__((always_inline)) int read_block_header(BitIn& b, bool* last, u32* type, u32* slen, u8* lens, HuffLds* lh,
                                 u32* ltab, HuffLds* dh, u32* dtab) {
    return read_block_header<LB, LCAP, DB, DCAP>(b, last, type, slen, lens, lh, ltab, dh, dtab,
        [&](BitIn& bb) __attribute__((always_inline)) { return read_dynamic<LB, LCAP, DB, DCAP>(bb, lens, lh, ltab, dh, dtab); });
}

// zlib keeps decoding after the output is full until it needs to emit a
// byte (LIT / MATCH with left == 0) or needs input it was not given: the
// next literal/length code, length extra bits, distance code, distance
// extra bits, and whole block headers are validated.  The input it was
// given is the rest of flate2's current 32 KiB BufReader window.
template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB>
__device__ __attribute__((always_inline)) int inf_lookahead(BitIn& b, bool last, bool at_header, u8* lens, HuffLds* lh,
                             u32* ltab, HuffLds* dh, u32* dtab, bool* at_end) {
    // *at_end: R_OK because the stream ended (the final block's last bit is
    // consumed), not because the next step would emit a byte
    *at_end = false;
    for (;;) {
        if (at_header) {  // after a stored block: straight to the next header
            at_header = false;
            if (last) { *at_end = true; return R_OK; }
            u32 type = 0, slen = 0;
            int r = read_block_header<LB, LCAP, DB, DCAP>(b, &last, &type, &slen, lens, lh, ltab, dh, dtab);
            if (r != R_OK) return r;
            if (type == 0) {
                if (slen != 0) return R_OK;
                at_header = true;
                continue;
            }
        }
        u32 e;
        int r = decode_sym(b, ltab, LB, &e);
        if (r != R_OK) return r;
        const u32 kind = (e >> 24) & 15;
        if (kind == K_LIT) return R_OK;
        if (kind == K_BAD) return R_INVALID;  // "invalid literal/length code"
        if (kind == K_LEN) {
            const u32 ex = (e >> 16) & 0xFF;
            if (!bi_has(b, ex)) return R_EXHAUSTED;
            if (ex) bi_bits(b, ex);
            u32 de;
            r = decode_sym(b, dtab, DB, &de);
            if (r != R_OK) return r;
            if (((de >> 24) & 15) != K_DIST) return R_INVALID;  // "invalid distance code"
            return R_OK;  // DISTEXT then MATCH: zlib leaves there (left == 0)
        }
        // end of block: the next block header is parsed without output
        for (;;) {
            if (last) { *at_end = true; return R_OK; }  // stream end
            u32 type = 0, slen = 0;
            r = read_block_header<LB, LCAP, DB, DCAP>(b, &last, &type, &slen, lens, lh, ltab, dh, dtab);
            if (r != R_OK) return r;
            if (type != 0) break;         // decode symbols of the new block
            if (slen != 0) return R_OK;   // COPY with left == 0: leave
        }
    }
}


// flate2 read_gz_header (wave-uniform): returns status, *hlen = header bytes.
__device__ inline int gzip_header(const u8* s, u64 n_in, u64* hlen) {
    u64 h = 10;
    if (n_in < 10) return ZCG_ERR_UNEXPECTED_EOF;
    if (s[0] != 0x1f || s[1] != 0x8b || s[2] != 8) return ZCG_ERR_INVALID_DATA;
    const u32 flg = s[3];
    if (flg & 4) {
        if (h + 2 > n_in) return ZCG_ERR_UNEXPECTED_EOF;
        h += 2 + ((u64)s[h] | ((u64)s[h + 1] << 8));
        if (h > n_in) return ZCG_ERR_UNEXPECTED_EOF;
    }
    if (flg & 8) {
        while (h < n_in && s[h]) h++;
        if (h >= n_in) return ZCG_ERR_UNEXPECTED_EOF;
        h++;
    }
    if (flg & 16) {
        while (h < n_in && s[h]) h++;
        if (h >= n_in) return ZCG_ERR_UNEXPECTED_EOF;
        h++;
    }
    if (flg & 2) {
        if (h + 2 > n_in) return ZCG_ERR_UNEXPECTED_EOF;
        u32 crc = 0xFFFFFFFFu;
        for (u64 i = 0; i < h; i++) crc = g_crc32_table[(crc ^ s[i]) & 255] ^ (crc >> 8);
        crc ^= 0xFFFFFFFFu;
        if ((crc & 0xFFFF) != ((u32)s[h] | ((u32)s[h + 1] << 8))) return ZCG_ERR_INVALID_DATA;
        h += 2;
    }
    *hlen = h;
    return ZCG_OK;
}

// zlib's inflate() HEAD state (RFC 1950; flate2's ZlibDecoder runs the same
// code): two bytes, a multiple of 31, CM 8, a window of at most 15 bits; a
// preset dictionary is not supported.  The declared window is not enforced.
__device__ inline int zlib_header(const u8* s, u64 n_in, u64* hlen) {
    if (n_in < 2) return ZCG_ERR_UNEXPECTED_EOF;
    const u32 b0 = s[0], b1 = s[1];
    if (((b0 << 8) | b1) % 31 != 0) return ZCG_ERR_INVALID_DATA;  // "incorrect header check"
    if ((b0 & 15) != 8) return ZCG_ERR_INVALID_DATA;              // "unknown compression method"
    if ((b0 >> 4) > 7) return ZCG_ERR_INVALID_DATA;               // "invalid window size"
    if (b1 & 0x20) return ZCG_ERR_UNSUPPORTED;                    // FDICT
    *hlen = 2;
    return ZCG_OK;
}

// The header of the frame kind.  `zlib` is a compile-time constant in the wave
// and 256-lane kernels (one instantiation per kind, picked by the launcher from
// INF_FRAME_ZLIB in the flag word, zcg_common.h: the gzip kernels' code is then
// what it was before the second kind existed) and that flag bit in the serial
// kernel.  The kind is read here and in inf_close, nowhere else.
__device__ __forceinline__ int inf_header(const u8* s, u64 n_in, bool zlib, u64* hlen) {
    return zlib ? zlib_header(s, n_in, hlen) : gzip_header(s, n_in, hlen);
}

// ---- the member frame ----------------------------------------------------------------------
// An open member: the deflate stream ds[0, n_ds) after h header bytes of the
// n_in member bytes, and the output with the transform a kernel commits with
// (bool waits for the end of the chunk where the output is the LZ77 window).
struct InfMember {
    const u8* ds;
    u64 n_ds, h, n_in;
    u8* dst;
    DType tw;
};

// The guards every kernel starts with and flate2's header.  false: *st is the
// chunk's final status (ZCG_OK for an empty chunk).  A kernel's own size
// limits come after this.
__device__ __forceinline__ bool inf_open(const zcg_chunk& ch, u64 D, DType t, bool zlib, InfMember& m, int* st) {
    if (D == 0) { *st = ZCG_OK; return false; }
    if (ch.dst_cap < D) { *st = ZCG_ERR_INVALID_INPUT; return false; }
    const u8* s = (const u8*)ch.src;
    u64 h = 0;
    *st = inf_header(s, ch.src_len, zlib, &h);
    if (*st != ZCG_OK) return false;
    m.ds = s + h;
    m.n_ds = ch.src_len - h;
    m.h = h;
    m.n_in = ch.src_len;
    m.dst = (u8*)ch.dst;
    m.tw = t;
    m.tw.isbool = 0;
    return true;
}

// The end of every kernel's block loop: r = the loop's result, P = bytes
// produced, boundary = the output filled exactly at a token boundary (then
// zlib looks ahead, inf_lookahead, inside inf_lookahead_limit), last /
// after_stored = the block the loop stopped in.  Returns the chunk's status.
// Under the frame's trailer verify flag (rules in zchunk_gpu.h; one bit in
// vflags for both kinds, zcg_common.h; `zlib` picks the trailer's layout) the look-ahead walks to the member's end
// with the whole input as its limit, the trailer is read where the stream
// ended, and `rec` receives the expected CRC32 (zlib frame: Adler-32).
template <int LB = INF_LBITS, u32 LCAP = INF_LTAB, int DB = INF_DBITS, u32 DCAP = INF_DTAB>
__device__ __attribute__((always_inline)) int inf_close(BitIn& b, const InfMember& m, int r, u64 P, u64 D, bool boundary,
                                                        bool last, bool after_stored, u8* lens, HuffLds* lh, u32* ltab,
                                                        HuffLds* dh, u32* dtab, u32 vflags, VerifyRec* rec,
                                                        bool zlib = false) {
    const bool verify = (vflags & ZCG_FLAG_VERIFY_GZIP_TRAILER) != 0;
    int la = R_EXHAUSTED;  // (what a look-ahead that cannot start amounts to)
    bool at_end = false;
    if (r == R_OK && P >= D && boundary) {
        b.limit = verify ? m.n_ds * 8 : inf_lookahead_limit(m.h, b.consumed, m.n_in);
        if (b.limit >= b.consumed) {
            la = inf_lookahead<LB, LCAP, DB, DCAP>(b, last, after_stored, lens, lh, ltab, dh, dtab, &at_end);
            if (la == R_INVALID) r = R_INVALID;
        }
    }
    if (r == R_INVALID) return ZCG_ERR_INVALID_DATA;
    if (r == R_EXHAUSTED || P < D) return ZCG_ERR_UNEXPECTED_EOF;
    if (!verify) return ZCG_OK;
    // the chunk decodes OK: the member's end and its trailer
    if (!boundary) return ZCG_ERR_INVALID_DATA;       // full inside a match / a stored block
    if (la == R_EXHAUSTED) return ZCG_ERR_UNEXPECTED_EOF;
    if (!at_end) return ZCG_ERR_INVALID_DATA;         // the next step would emit a byte
    const u64 tr = m.h + (b.consumed + 7) / 8;
    const u8* const tp = m.ds - m.h + tr;
    if (zlib) {  // Adler-32, big-endian; no length word
        if (tr + 4 > m.n_in) return ZCG_ERR_UNEXPECTED_EOF;
        if (threadIdx.x == 0) *rec = VerifyRec{V_CHECK, __builtin_bswap32(ld32(tp))};
        return ZCG_OK;
    }
    if (tr + 8 > m.n_in) return ZCG_ERR_UNEXPECTED_EOF;
    if (ld32(tp + 4) != (u32)D) return ZCG_ERR_INVALID_DATA;
    if (threadIdx.x == 0) *rec = VerifyRec{V_CHECK, ld32(tp)};
    return ZCG_OK;
}

// Stage entries (u16) of the parallel kernels: SE_VAL | byte is a final byte
// value; anything below is the kernel's own (pointers to earlier bytes).
constexpr u32 SE_VAL = 0xFF00u;

// Flush the resolved stage bytes [from, to) to dst by NT threads (byte-order
// transform fused): 16-byte-aligned output pieces by vector, the head and the
// tail by bytes.  Output position q sits at stage[idx(q)], and 16 entries from
// a 16-aligned q are contiguous there.  The barriers around it (the stage is
// complete; the bytes are visible to the next window reads) are the caller's.
template <u32 NT, class Idx>
__device__ __forceinline__ void stage_commit(const u16* stage, u8* dst, u64 from, u64 to, DType t, u32 tid, Idx idx) {
    const u64 a16 = (from + 15) & ~15ull, b16 = to & ~15ull;
    if (a16 < b16) {
        for (u64 p = a16 + (u64)tid * 16; p < b16; p += NT * 16) {
            const u32 i = idx(p);
            const u32x4 lo = *(const u32x4*)(stage + i);
            const u32x4 hi = *(const u32x4*)(stage + i + 8);
            // each u32 holds two 16-bit entries; keep their low bytes
            auto pk = [](u32 a, u32 b) -> u32 { return __builtin_amdgcn_perm(b, a, 0x06040200u); };
            const u32x4 v = u32x4{pk(lo.x, lo.y), pk(lo.z, lo.w), pk(hi.x, hi.y), pk(hi.z, hi.w)};
            st16(dst + p, transform16(v, t));
        }
    }
    const u64 e0 = a16 < b16 ? a16 : to;
    for (u64 q = from + tid; q < e0; q += NT) dst[swap_pos(q, t)] = (u8)stage[idx(q)];
    if (a16 < b16)
        for (u64 q = b16 + tid; q < to; q += NT) dst[swap_pos(q, t)] = (u8)stage[idx(q)];
}

// A stored block of slen bytes at stream byte in0, copied through the stage at
// most `cap` bytes at a time by NT threads: entry(P, i) = the stage index of
// the i-th byte of a piece that starts at output position P, commit(from, to)
// flushes a piece (with the kernel's barriers).  Stops at D.  Returns R_OK or
// R_EXHAUSTED; *in_end = the stream byte after the copied ones, *whole = the
// block was copied to its end.
template <u32 NT, class Entry, class Commit>
__device__ __forceinline__ int inf_stored_copy(const InfMember& m, u64 in0, u32 slen, u64& P, u64 D, u32 cap, u16* stage,
                                               u32 tid, Entry entry, Commit commit, u64* in_end, bool* whole) {
    u32 done = 0;
    while (done < slen && P < D) {
        u32 k = slen - done;
        if (k > cap) k = cap;
        if ((u64)k > D - P) k = (u32)(D - P);
        if (in0 + k > m.n_ds) return R_EXHAUSTED;
        for (u32 i = tid; i < k; i += NT) stage[entry(P, i)] = (u16)(SE_VAL | m.ds[in0 + i]);
        commit(P, P + k);
        P += k; in0 += k; done += k;
    }
    *in_end = in0;
    *whole = done == slen;
    return R_OK;
}

}  // namespace zcg
