// zcg_deflate_seg.hip — the segmented gzip coder (CompressionType::Gzip at level
// 0 and with ZCG_FLAG_GZIP_SEGMENTED; else the zlib-exact coder, zcg_deflate.hip).
//
// Reference: gzip.rs:50-56 wraps the writer in flate2's GzEncoder at the
// effective level (gzip.rs:28-39: -1 / out of [0,9] -> 6): a 10-byte header
// 1f 8b 08 00 | mtime 0 | XFL | OS 255 (XFL 2 at level >= 9, 4 at level <= 1,
// else 0), zlib raw deflate, then CRC32 and ISIZE (LE).  Encoded bytes are not
// pinned beyond the doc-spec vector; the contract is: the stream
// inflates (zlib) to exactly the serialised chunk, with those conventions.
// The block-type choice (stored / fixed / dynamic by size, fixed on a tie)
// follows zlib's _tr_flush_block, which is what reproduces the doc-spec vector.
//
// Layout (stream-ordered kernels):
//   0. match finding over whole chunks, data-parallel (<= 128 MiB per
//      sub-batch): keys (chunk, the 3 serialised bytes) sorted with the
//      positions as values (stable radix sort), chain_links (zcg_chains.h) links each
//      position to its predecessor with the same 3 bytes, df_best walks up to
//      zlib's max_chain (capped at 64) candidates within 32 KiB and keeps the
//      longest match (nearest on ties, zlib's nice_length stops the walk).
//   1. deflate_segment: one wave per 16 KiB input segment.  The segment and
//      the 32 KiB before it (deflate's window) are staged in LDS with the
//      dtype transform applied (write_data's byte order, chunk.rs:118-140).
//      Every position's longest match comes precomputed (step 0); the
//      64 lanes read 64 consecutive positions' matches and the wave walks them
//      greedily (one-step lazy evaluation at level >= 4).  Pass A runs the parse for symbol
//      frequencies; the wave builds length-limited Huffman codes (zlib's
//      bl_count overflow rule) and picks stored/fixed/dynamic; pass B re-runs
//      the same deterministic parse and emits the bits through an LDS ring
//      (wave prefix sums place 64 literal codes at once).  A non-final
//      segment ends with an empty stored block so it is byte aligned.
//      Segment k is written at its upper-bound slot of dst.
//   2. deflate_finalize: per chunk, the gzip header and segment compaction.
//   3. gzip_crc32 (zcg_deflate.hip): per chunk, the CRC32 + ISIZE trailer.
#include "zcg_chains.h"
#include "zcg_deflate.h"

namespace zcg {

constexpr u32 DF_SEG = 16384;               // input bytes per segment (one deflate block)
constexpr u32 DF_HIST = 32768;              // deflate window
constexpr u32 DF_WIN = DF_SEG + DF_HIST;
constexpr u32 DF_SLOT = DF_SEG + 128;       // output slot per segment (stored worst case + sync)
constexpr u32 DF_RING = 1024;               // output ring words
constexpr u32 DF_FLUSH = 512;

__constant__ u16 d_len_base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ u8 d_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2,
                                   2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ u16 d_dist_base[30] = {1,    2,    3,    4,    5,    7,     9,     13,    17,  25,
                                    33,   49,   65,   97,   129,  193,   257,   385,   513, 769,
                                    1025, 1537, 2049, 3073, 4097, 6145,  8193,  12289, 16385,
                                    24577};
__constant__ u8 d_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2,  3,  3,  4,  4,  5,  5,  6,
                                    6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ u8 d_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ u32 len_code(u32 len) {  // 3..258 -> 0..28 (d_len_base)
    if (len == 258) return 28;
    const u32 x = len - 3;
    if (x < 8) return x;
    const u32 k = 31 - __builtin_clz(x);  // 3..7
    return 4 * (k - 1) + ((x >> (k - 2)) & 3);
}
__device__ __forceinline__ u32 dist_code(u32 d) {  // 1..32768 -> 0..29 (d_dist_base)
    const u32 x = d - 1;
    if (x < 4) return x;
    const u32 k = 31 - __builtin_clz(x);  // 2..14
    return 2 * k + ((x >> (k - 1)) & 1);
}
__device__ __forceinline__ u32 rev_bits(u32 v, u32 n) { return n ? __builtin_bitreverse32(v) >> (32 - n) : 0u; }

struct DefLds {
    u32 lfreq[288], dfreq[32], cfreq[20];
    u32 lcode[288], dcode[32], ccode[20];  // (length << 16) | bit-reversed code
    u32 ring[DF_RING];
    // Huffman construction scratch
    u16 sorted[288];
    u16 parent[576];
    u16 depth[576];
    u32 wq[288];               // internal node weights (two-queue construction)
    u8 clens[320];             // code lengths: litlen [0,286), dist [288,318)
    u8 clcl[20];               // code-length code lengths
    u8 seq[320];               // litlen ++ dist lengths for the RLE
    u16 rle[320];              // code-length symbols: sym | extra << 8
    u32 ctl[16];
};

// Bits into the LDS ring at absolute bit position `bp` (value < 2^n, n <= 32).
__device__ __forceinline__ void ring_put(DefLds& L, u32 bp, u32 v, u32 n) {
    if (!n) return;
    const u32 w = bp >> 5, sh = bp & 31;
    atomicOr(&L.ring[w & (DF_RING - 1)], v << sh);
    if (sh + n > 32) atomicOr(&L.ring[(w + 1) & (DF_RING - 1)], v >> (32 - sh));
}

// Flush complete ring words [*fw, upto) to out (wave-cooperative).
constexpr u32 DF_OUTCAP = DF_SLOT - 4;   // bytes a segment may write after its length word
constexpr u32 CTL_ERR = 8;               // L.ctl slot: pass B inconsistency / overrun

__device__ void ring_flush(DefLds& L, u8* out, u32* fw, u32 upto) {
    const u32 lane = lane_id();
    __syncthreads();
    for (u32 w = *fw + lane; w < upto; w += 64) {
        const u32 v = L.ring[w & (DF_RING - 1)];
        if (4 * w + 4 <= DF_OUTCAP) {
            u8* o = out + 4ull * w;
            o[0] = (u8)v; o[1] = (u8)(v >> 8); o[2] = (u8)(v >> 16); o[3] = (u8)(v >> 24);
        } else {
            L.ctl[CTL_ERR] = 1;  // would overrun the slot: the segment falls back to stored
        }
        L.ring[w & (DF_RING - 1)] = 0;
    }
    *fw = upto;
    __syncthreads();
}

// Length-limited Huffman code lengths for freq[0..n) (n <= 288), wave-wide.
// Symbols with freq 0 get length 0; if fewer than 2 symbols are used, the
// first unused of symbols 0/1 gets freq 1 (zlib build_tree forces 2 codes).
__device__ void huff_lengths(DefLds& L, u32* freq, u32 n, u32 maxbits, u8* len_out) {
    const u32 lane = lane_id();
    __syncthreads();
    if (lane == 0) {
        u32 used = 0;
        for (u32 i = 0; i < n; i++) used += freq[i] != 0;
        for (u32 i = 0; used < 2 && i < 2; i++)
            if (!freq[i]) { freq[i] = 1; used++; }
    }
    __syncthreads();
    // rank sort by (freq, symbol) ascending, zero-frequency symbols excluded
    for (u32 s = lane; s < n; s += 64) {
        const u32 f = freq[s];
        if (!f) { len_out[s] = 0; continue; }
        u32 r = 0;
        for (u32 t = 0; t < n; t++) {
            const u32 g = freq[t];
            r += (g && (g < f || (g == f && t < s))) ? 1u : 0u;
        }
        L.sorted[r] = (u16)s;
    }
    __syncthreads();
    if (lane == 0) {
        u32 m = 0;
        for (u32 i = 0; i < n; i++) m += freq[i] != 0;
        // two-queue Huffman: leaves 0..m-1 (sorted), internal nodes m..2m-2
        u32* wq = L.wq;
        u32 li = 0, ii = 0, nint = 0;
        for (u32 k = 0; k + 1 < m; k++) {
            u32 pick[2];
            u32 wsum = 0;
            for (u32 j = 0; j < 2; j++) {
                const bool leaf = li < m && (ii >= nint || freq[L.sorted[li]] <= wq[ii]);
                if (leaf) { pick[j] = li; wsum += freq[L.sorted[li]]; li++; }
                else { pick[j] = m + ii; wsum += wq[ii]; ii++; }
            }
            L.parent[pick[0]] = (u16)(m + nint);
            L.parent[pick[1]] = (u16)(m + nint);
            wq[nint++] = wsum;
        }
        // depths: root = m + nint - 1
        u32 blc[16];
        for (u32 b = 0; b < 16; b++) blc[b] = 0;
        if (m == 1) {
            blc[1] = 1;
        } else {
            // zlib gen_bitlen: depths top-down from the CLAMPED parent depth;
            // every node (internal or leaf) pushed past maxbits counts as overflow
            L.depth[m + nint - 1] = 0;
            int overflow = 0;
            for (int x = (int)(m + nint) - 2; x >= 0; x--) {
                u32 d = (u32)L.depth[L.parent[x]] + 1;
                if (d > maxbits) { d = maxbits; overflow++; }
                L.depth[x] = (u16)d;
                if ((u32)x < m) blc[d]++;
            }
            while (overflow > 0) {  // zlib gen_bitlen
                u32 b = maxbits - 1;
                while (blc[b] == 0) b--;
                blc[b]--;
                blc[b + 1] += 2;
                blc[maxbits]--;
                overflow -= 2;
            }
        }
        // least frequent symbols get the longest codes
        u32 h = 0;
        for (u32 b = maxbits; b >= 1; b--)
            for (u32 c = blc[b]; c > 0; c--) len_out[L.sorted[h++]] = (u8)b;
    }
    __syncthreads();
}

// Canonical codes (bit-reversed for LSB-first output): code[s] = len << 16 | rev.
__device__ void huff_codes(const u8* len, u32 n, u32* code) {
    if (lane_id() != 0) return;
    u32 blc[16], next[16];
    for (u32 b = 0; b < 16; b++) blc[b] = 0;
    for (u32 s = 0; s < n; s++) blc[len[s]]++;
    blc[0] = 0;
    u32 c = 0;
    for (u32 b = 1; b < 16; b++) { c = (c + blc[b - 1]) << 1; next[b] = c; }
    for (u32 s = 0; s < n; s++) {
        const u32 l = len[s];
        code[s] = l ? ((l << 16) | rev_bits(next[l]++, l)) : 0u;
    }
}

// Fixed Huffman code (RFC 1951 3.2.6).
__device__ __forceinline__ u32 fixed_lcode(u32 s) {
    if (s < 144) return (8u << 16) | rev_bits(0x30 + s, 8);
    if (s < 256) return (9u << 16) | rev_bits(0x190 + (s - 144), 9);
    if (s < 280) return (7u << 16) | rev_bits(s - 256, 7);
    return (8u << 16) | rev_bits(0xC0 + (s - 280), 8);
}

struct ParseCfg {
    bool lazy;     // one-step lazy evaluation
    bool insert;   // insert positions inside matches
};

// One pass of the segment parse over window positions [h0, wend).
// EMIT=false: symbol frequencies.  EMIT=true: bits into the ring (bp, fw).
template <bool EMIT>
__device__ void parse_pass(DefLds& L, u32 h0, u32 wend, ParseCfg cfg, u32* bp, u32* fw, u8* out,
                           const u32* __restrict__ mt, const u8* __restrict__ src, u64 w0, DType t) {
    const u32 lane = lane_id();
    u32 ip = h0;
    while (ip < wend) {
        // keep the ring from wrapping: a group adds < 2 Kbit
        if (EMIT && (*bp >> 5) >= *fw + DF_FLUSH) ring_flush(L, out, fw, *bp >> 5);
        const u32 gend = (wend - ip) < 64 ? (wend - ip) : 64u;  // positions of this group
        const u32 p = ip + lane;
        const bool valid = lane < gend && p + 3 <= wend;
        // the precomputed longest match of this position (df_best), clipped to the segment
        const u32 m = valid ? mt[p] : 0u;
        u32 bl = m & 0x1FF, br = p - ((m >> 16) + 1);
        if (bl > wend - p) bl = wend - p;
        if (bl < 3 || (bl == 3 && p - br > 4096)) bl = 0;  // zlib TOO_FAR
        const unsigned long long mask = __ballot(bl >= 3);
        // The greedy (lazy) parse of the group as a chain over its positions:
        // position p steps to p + 1 (literal), p + len (match) or, when the
        // next position holds a longer match (lazy evaluation), emits a
        // literal and that match and steps to p + 1 + len'.  The chain from 0
        // is found by pointer doubling (lane k gets its k-th member in six
        // ds_bpermute rounds), and the members emit in parallel at bit
        // offsets from a wave prefix sum: the same parse, decisions and bits
        // as a serial walk (zlib deflate_slow's order).
        (void)mask;
        const u32 bl1 = (u32)__shfl((int)bl, (int)((lane + 1) & 63), 64);
        const u32 br1 = (u32)__shfl((int)br, (int)((lane + 1) & 63), 64);
        const bool ism = bl >= 3;
        const bool lz = cfg.lazy && ism && bl < 32 && lane + 1 < gend && bl1 > bl;
        const u32 nx = !ism ? lane + 1 : lz ? lane + 1 + bl1 : lane + bl;
        u32 J[6];
        J[0] = nx;
#pragma unroll
        for (u32 k = 1; k < 6; k++) {
            const u32 t = (u32)__shfl((int)J[k - 1], (int)(J[k - 1] & 63), 64);
            J[k] = J[k - 1] < 64 ? t : J[k - 1];
        }
        u32 cur = 0;  // position of member #lane
#pragma unroll
        for (u32 k = 0; k < 6; k++) {
            const u32 t = (u32)__shfl((int)J[k], (int)(cur & 63), 64);
            if ((lane >> k) & 1u) cur = cur < 64 ? t : cur;
        }
        const bool mem = cur < gend;
        const u32 nm = (u32)__popcll(__ballot(mem));  // >= 1: position 0 is a member
        const u32 lastp = (u32)__builtin_amdgcn_readlane((int)cur, (int)(nm - 1));
        const u32 pos = (u32)__builtin_amdgcn_readlane((int)nx, (int)lastp);  // first position after the group's chain
        // my member's unit: literal, match, or literal + match (lazy)
        const u32 q = cur & 63;
        const u32 qism = (u32)__shfl((int)(ism ? 1u : 0u), (int)q, 64);
        const u32 qlz = (u32)__shfl((int)(lz ? 1u : 0u), (int)q, 64);
        const u32 qbl = (u32)__shfl((int)bl, (int)q, 64), qbr = (u32)__shfl((int)br, (int)q, 64);
        const u32 qbl1 = (u32)__shfl((int)bl1, (int)q, 64), qbr1 = (u32)__shfl((int)br1, (int)q, 64);
        const bool hlit = mem && (!qism || qlz);  // a literal at q
        const bool hmat = mem && qism;            // a match at q (or q + 1 when lazy)
        const u32 mpos = ip + q + (qlz ? 1u : 0u);
        const u32 mlen = qlz ? qbl1 : qbl;
        const u32 d = mpos - (qlz ? qbr1 : qbr);
        const u32 byte = hlit ? (u32)norm_byte(src[swap_pos(w0 + ip + q, t)], t) : 0u;
        const u32 lc = hmat ? len_code(mlen) : 0u, dc = hmat ? dist_code(d) : 0u;
        if (!EMIT) {
            if (hlit) atomicAdd(&L.lfreq[byte], 1u);
            if (hmat) { atomicAdd(&L.lfreq[257 + lc], 1u); atomicAdd(&L.dfreq[dc], 1u); }
        } else {
            const u32 cw = hlit ? L.lcode[byte] : 0u;
            const u32 nb = cw >> 16;
            const u32 lcw = hmat ? L.lcode[257 + lc] : 0u, dcw = hmat ? L.dcode[dc] : 0u;
            const u32 nl = lcw >> 16, nd = dcw >> 16;
            const u32 el = hmat ? (u32)d_len_extra[lc] : 0u, ed = hmat ? (u32)d_dist_extra[dc] : 0u;
            if ((hlit && nb == 0) || (hmat && (nl == 0 || nd == 0))) L.ctl[CTL_ERR] = 1;
            const u32 nbits = nb + nl + el + nd + ed;
            u32 x = nbits;  // wave inclusive scan of the units' bit counts
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const u32 y = (u32)__shfl_up((int)x, dd, 64);
                if ((int)lane >= dd) x += y;
            }
            const u32 tot = (u32)__shfl((int)x, 63, 64);
            u32 b = *bp + x - nbits;
            if (hlit) { ring_put(L, b, cw & 0xFFFF, nb); b += nb; }
            if (hmat) {
                ring_put(L, b, lcw & 0xFFFF, nl); b += nl;
                ring_put(L, b, mlen - d_len_base[lc], el); b += el;
                ring_put(L, b, dcw & 0xFFFF, nd); b += nd;
                ring_put(L, b, d - d_dist_base[dc], ed);
            }
            *bp += tot;
        }
        ip += pos;
    }
    if (EMIT && (*bp >> 5) >= *fw + DF_FLUSH) ring_flush(L, out, fw, *bp >> 5);
}

__global__ __launch_bounds__(64) void deflate_segment(const zcg_chunk* __restrict__ chunks, u32 c0, u32 n, u64 D,
                                                      u32 nseg, u64 bound, DType t, u32 level,
                                                      const u32* __restrict__ match) {
    extern __shared__ __attribute__((aligned(16))) u8 smem_raw[];
    DefLds& L = *(DefLds*)smem_raw;
    const u32 lane = threadIdx.x;
    const u32 cl = blockIdx.x / nseg, k = blockIdx.x % nseg;
    if (cl >= n) return;
    const u32 c = c0 + cl;
    const zcg_chunk ch = chunks[c];
    if (ch.dst_cap < bound || ch.src_len < D) return;
    const u8* src = (const u8*)ch.src;
    u8* slot = (u8*)ch.dst + DF_HDR + (u64)k * DF_SLOT;
    u8* out = slot + 4;
    const u64 s0 = (u64)k * DF_SEG;
    const u32 S = (u32)((D - s0) < DF_SEG ? (D - s0) : DF_SEG);
    const u32 hist = (u32)(s0 < DF_HIST ? s0 : DF_HIST);
    const u64 w0 = s0 - hist;
    const u32 wend = hist + S;
    const bool final_seg = (k + 1 == nseg);
    for (u32 q = lane; q < 288; q += 64) L.lfreq[q] = 0;
    if (lane < 32) L.dfreq[lane] = 0;
    if (lane < 20) L.cfreq[lane] = 0;
    for (u32 q = lane; q < DF_RING; q += 64) L.ring[q] = 0;
    __syncthreads();
    u32 bp = 0, fw = 0;
    int btype = 0;  // 0 stored, 1 fixed, 2 dynamic
    u32 hlit = 257, hdist = 1, hclen = 4, nrle = 0;
    if (level > 0) {
        const ParseCfg cfg{level >= 4, level >= 4};
        parse_pass<false>(L, hist, wend, cfg, &bp, &fw, out, match + (u64)cl * D + w0, src, w0, t);
        if (lane == 0) L.lfreq[256] += 1;  // end of block
        __syncthreads();
        // ---- codes and the block type (zlib _tr_flush_block) ------------------------
        huff_lengths(L, L.lfreq, 286, 15, L.clens);
        huff_lengths(L, L.dfreq, 30, 15, L.clens + 288);
        if (lane == 0) {
            hlit = 286;
            while (hlit > 257 && L.clens[hlit - 1] == 0) hlit--;
            hdist = 30;
            while (hdist > 1 && L.clens[288 + hdist - 1] == 0) hdist--;
            // code-length sequence (litlen[0..hlit) ++ dist[0..hdist)), RLE 16/17/18
            u8* seq = L.seq;
            const u32 N = hlit + hdist;
            for (u32 i = 0; i < hlit; i++) seq[i] = L.clens[i];
            for (u32 i = 0; i < hdist; i++) seq[hlit + i] = L.clens[288 + i];
            u32 i = 0;
            nrle = 0;
            while (i < N) {
                const u32 v = seq[i];
                u32 run = 1;
                while (i + run < N && seq[i + run] == v) run++;
                if (v == 0 && run >= 3) {
                    u32 r = run;
                    while (r >= 11) { const u32 a = r < 138 ? r : 138; L.rle[nrle++] = (u16)(18 | ((a - 11) << 8)); r -= a; }
                    if (r >= 3) { L.rle[nrle++] = (u16)(17 | ((r - 3) << 8)); r = 0; }
                    while (r) { L.rle[nrle++] = 0; r--; }
                } else {
                    L.rle[nrle++] = (u16)v;
                    u32 r = run - 1;
                    while (r >= 3) { const u32 a = r < 6 ? r : 6; L.rle[nrle++] = (u16)(16 | ((a - 3) << 8)); r -= a; }
                    while (r) { L.rle[nrle++] = (u16)v; r--; }
                }
                i += run;
            }
            for (u32 j = 0; j < 20; j++) L.cfreq[j] = 0;
            for (u32 j = 0; j < nrle; j++) L.cfreq[L.rle[j] & 31]++;
            L.ctl[1] = hlit; L.ctl[2] = hdist; L.ctl[3] = nrle;
        }
        __syncthreads();
        hlit = L.ctl[1]; hdist = L.ctl[2]; nrle = L.ctl[3];
        huff_lengths(L, L.cfreq, 19, 7, L.clcl);
        huff_codes(L.clens, 286, L.lcode);
        huff_codes(L.clens + 288, 30, L.dcode);
        huff_codes(L.clcl, 19, L.ccode);
        __syncthreads();
        if (lane == 0) {
            hclen = 19;
            while (hclen > 4 && L.clcl[d_clen_order[hclen - 1]] == 0) hclen--;
            // sizes in bits (zlib: opt_len / static_len exclude the 3 header bits)
            u64 opt = 5 + 5 + 4 + 3ull * hclen, stat = 0;
            for (u32 j = 0; j < nrle; j++) {
                const u32 sym = L.rle[j] & 31;
                opt += L.clcl[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
            }
            for (u32 s = 0; s < 286; s++) {
                const u32 f = L.lfreq[s];
                if (!f) continue;
                const u32 ex = s >= 257 ? d_len_extra[s - 257] : 0;
                opt += (u64)f * (L.clens[s] + ex);
                stat += (u64)f * ((fixed_lcode(s) >> 16) + ex);
            }
            for (u32 s = 0; s < 30; s++) {
                const u32 f = L.dfreq[s];
                if (!f) continue;
                opt += (u64)f * (L.clens[288 + s] + d_dist_extra[s]);
                stat += (u64)f * (5 + d_dist_extra[s]);
            }
            u64 optb = (opt + 3 + 7) >> 3, statb = (stat + 3 + 7) >> 3;
            if (statb <= optb) optb = statb;
            int bt;
            if ((u64)S + 4 <= optb) bt = 0;
            else if (statb == optb) bt = 1;
            else bt = 2;
            L.ctl[4] = (u32)bt;
            L.ctl[5] = hclen;
        }
        __syncthreads();
        btype = (int)L.ctl[4];
        hclen = L.ctl[5];
    }
    bp = 0;
    fw = 0;
    if (btype == 0) {  // stored block (byte aligned: the segment starts at a byte)
        if (lane == 0) {
            out[0] = final_seg ? 1 : 0;
            out[1] = (u8)S; out[2] = (u8)(S >> 8);
            out[3] = (u8)~S; out[4] = (u8)(~S >> 8);
        }
        for (u32 q = lane; q < S; q += 64) out[5 + q] = norm_byte(src[swap_pos(s0 + q, t)], t);
        if (lane == 0) { const u32 len = 5 + S; slot[0] = (u8)len; slot[1] = (u8)(len >> 8); slot[2] = (u8)(len >> 16); slot[3] = (u8)(len >> 24); }
        return;
    }
    if (btype == 1) {  // fixed codes
        for (u32 s = lane; s < 288; s += 64) L.lcode[s] = fixed_lcode(s);
        if (lane < 32) L.dcode[lane] = (5u << 16) | rev_bits(lane, 5);
    }
    __syncthreads();
    if (lane == 0) {
        u32 b = 0;
        ring_put(L, b, (final_seg ? 1u : 0u) | ((u32)btype << 1), 3); b += 3;
        if (btype == 2) {
            ring_put(L, b, hlit - 257, 5); b += 5;
            ring_put(L, b, hdist - 1, 5); b += 5;
            ring_put(L, b, hclen - 4, 4); b += 4;
            for (u32 j = 0; j < hclen; j++) { ring_put(L, b, L.clcl[d_clen_order[j]], 3); b += 3; }
            for (u32 j = 0; j < nrle; j++) {
                const u32 sym = L.rle[j] & 31, ex = L.rle[j] >> 8;
                const u32 cw = L.ccode[sym];
                ring_put(L, b, cw & 0xFFFF, cw >> 16); b += cw >> 16;
                const u32 eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                ring_put(L, b, ex, eb); b += eb;
            }
        }
        L.ctl[0] = b;
    }
    __syncthreads();
    bp = L.ctl[0];
    // the header may exceed a flush unit only in theory (< 400 bytes); flush if needed
    if ((bp >> 5) >= fw + DF_FLUSH) ring_flush(L, out, &fw, bp >> 5);
    if (lane == 0) L.ctl[CTL_ERR] = 0;
    __syncthreads();
    const ParseCfg cfg{level >= 4, level >= 4};
    parse_pass<true>(L, hist, wend, cfg, &bp, &fw, out, match + (u64)cl * D + w0, src, w0, t);
    if (lane == 0) {
        u32 b = bp;
        const u32 cw = L.lcode[256];
        ring_put(L, b, cw & 0xFFFF, cw >> 16); b += cw >> 16;  // end of block
        if (!final_seg) { b += 3; b = (b + 7) & ~7u; b += 32; }  // empty stored block (sync)
        L.ctl[0] = b;
    }
    __syncthreads();
    bp = L.ctl[0];
    const u32 nbytes = (bp + 7) >> 3;
    // empty stored block after a non-final segment: LEN = 0 (zero bits), NLEN = 0xFFFF
    if (!final_seg && lane == 0) ring_put(L, bp - 16, 0xFFFFu, 16);
    __syncthreads();
    ring_flush(L, out, &fw, (bp + 31) >> 5);
    if (L.ctl[CTL_ERR]) {  // inconsistent or oversized: store the segment instead
        if (lane == 0) {
            out[0] = final_seg ? 1 : 0;
            out[1] = (u8)S; out[2] = (u8)(S >> 8);
            out[3] = (u8)~S; out[4] = (u8)(~S >> 8);
        }
        for (u32 q = lane; q < S; q += 64) out[5 + q] = norm_byte(src[swap_pos(s0 + q, t)], t);
        if (lane == 0) { const u32 len = 5 + S; slot[0] = (u8)len; slot[1] = (u8)(len >> 8); slot[2] = (u8)(len >> 16); slot[3] = (u8)(len >> 24); }
        return;
    }
    if (lane == 0) { slot[0] = (u8)nbytes; slot[1] = (u8)(nbytes >> 8); slot[2] = (u8)(nbytes >> 16); slot[3] = (u8)(nbytes >> 24); }
}

__global__ __launch_bounds__(256) void deflate_finalize(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                        u32 nseg, u64 bound, u32 xfl, u32 zhdr,
                                                        u64* __restrict__ out_len, i32* __restrict__ status) {
    const u32 c = blockIdx.x, tid = threadIdx.x;
    if (c >= n) return;
    const zcg_chunk ch = chunks[c];
    if (ch.src_len < D) { if (tid == 0) { status[c] = ZCG_ERR_INVALID_DATA; out_len[c] = 0; } return; }
    if (ch.dst_cap < bound) { if (tid == 0) { status[c] = ZCG_ERR_OUTPUT_TOO_SMALL; out_len[c] = 0; } return; }
    u8* dst = (u8*)ch.dst;
    if (tid == 0) df_put_header(dst, xfl, zhdr);
    __shared__ u32 s_sz;
    u64 pos = df_header_bytes(zhdr);  // (<= DF_HDR, where the first slot starts: the copies below move down)
    if (nseg == 0) {  // empty input: one final fixed block holding only end-of-block
        if (tid == 0) { dst[pos] = 0x03; dst[pos + 1] = 0x00; }
        pos += 2;
    }
    for (u32 k = 0; k < nseg; k++) {
        const u64 tmp = DF_HDR + (u64)k * DF_SLOT;
        __syncthreads();
        if (tid == 0) s_sz = ld32(dst + tmp);
        __syncthreads();
        const u64 total = s_sz;
        const u64 from = tmp + 4;
        for (u64 q = 0; q < total; q += 256 * 16) {  // dst <= src: all reads of a tile before its writes
            const u64 i = q + (u64)tid * 16;
            u32x4 v = {0u, 0u, 0u, 0u};
            u32 nb = 0;
            if (i < total) {
                nb = (total - i) < 16 ? (u32)(total - i) : 16u;
                if (nb == 16) v = ld16(dst + from + i);
                else for (u32 j = 0; j < nb; j++) ((u8*)&v)[j] = dst[from + i + j];
            }
            __syncthreads();
            if (nb == 16) st16(dst + pos + i, v);
            else for (u32 j = 0; j < nb; j++) dst[pos + i + j] = ((u8*)&v)[j];
            __syncthreads();
        }
        pos += total;
    }
    if (tid == 0) {
        out_len[c] = pos + df_trailer_bytes(zhdr);  // + CRC32 + ISIZE, or the Adler-32 (kernel 3)
        status[c] = ZCG_OK;
    }
}

namespace {

constexpr u64 DF_SUB_BYTES = 128ull << 20;  // input bytes per match-finder sub-batch
constexpr u64 DF_SUPER_BYTES = 1ull << 30;  // input bytes per segment launch

struct DfWs {
    SubBatch b;  // (m <= 256: chunk id + 24 key bits fit 32)
    ChainWs c;
    u64 off_match, total;
};

DfWs df_ws(u64 D, u32 n) {
    DfWs y{};
    y.b = sub_batch_plan(D, n, DF_SUB_BYTES, DF_SUPER_BYTES, 256);
    WsCarve ws;
    y.c = carve_chain_ws(ws, y.b.tot, true);
    y.off_match = ws.take(4 * (u64)y.b.sm * D);
    y.total = ws.total();
    return y;
}

__global__ void df_keys(const zcg_chunk* __restrict__ chunks, u32 c0, u64 D, u64 tot, DType t,
                        u32* __restrict__ keys, u32* __restrict__ vals) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tot) return;
    const u32 cl = (u32)(g / D);
    const u64 p = g - (u64)cl * D;
    const zcg_chunk ch = chunks[c0 + cl];
    const u8* src = (const u8*)ch.src;
    u32 v = 0;
    if (p + 3 <= D && ch.src_len >= D) v = ser1(src, p, t) | (ser1(src, p + 1, t) << 8) | (ser1(src, p + 2, t) << 16);
    keys[g] = (cl << 24) | v;
    vals[g] = (u32)g;
}

// match[g] = len | (dist - 1) << 16 of the longest match at g (len 0: none)
__global__ void df_best(const zcg_chunk* __restrict__ chunks, u32 c0, u64 D, u64 tot, DType t, u32 depth,
                        u32 nice, const u32* __restrict__ prev, u32* __restrict__ match) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tot) return;
    const u32 cl = (u32)(g / D);
    const u64 p = g - (u64)cl * D;
    u32 best = 0, bd = 0;
    if (p + 3 <= D && chunks[c0 + cl].src_len >= D) {  // a short src is INVALID_DATA (deflate_finalize)
        const u8* src = (const u8*)chunks[c0 + cl].src;
        const u64 cbase = (u64)cl * D;
        const u32 mx = (D - p) < 258 ? (u32)(D - p) : 258u;
        // bytes p+3..p+6 are compared with every candidate: load them once;
        // the next chain link is loaded before this candidate's compare
        const u32 pw = mx >= 7 ? ser4(src, p + 3, t) : 0u;
        u32 q = prev[g];
        for (u32 dep = 0; dep < depth && q != 0xFFFFFFFFu; dep++) {
            const u64 qp = q - cbase;
            if (p - qp > DF_HIST) break;
            const u32 qn = prev[q];
            u32 k = 3;  // the 3 key bytes are equal
            bool diff = false;
            if (mx >= 7) {
                const u32 x = pw ^ ser4(src, qp + 3, t);
                if (x) { k += (u32)__builtin_ctz(x) >> 3; diff = true; }
                else k = 7;
            }
            while (!diff && k + 4 <= mx) {
                const u32 x = ser4(src, p + k, t) ^ ser4(src, qp + k, t);
                if (x) { k += (u32)__builtin_ctz(x) >> 3; diff = true; break; }
                k += 4;
            }
            if (!diff)
                while (k < mx && ser1(src, p + k, t) == ser1(src, qp + k, t)) k++;
            if (k > best && !(k == 3 && p - qp > 4096)) { best = k; bd = (u32)(p - qp); }
            if (best >= nice) break;
            q = qn;
        }
    }
    match[g] = best ? (best | ((bd - 1) << 16)) : 0u;
}

}  // namespace

uint64_t deflate_seg_ws_bytes(u64 D, u32 n) { return df_ws(D, n).total; }

hipError_t launch_deflate_seg(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, u32 level,
                              uint64_t* d_out_len, int32_t* d_status, void* ws, uint64_t ws_bytes, hipStream_t s) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    const u32 xfl = level >= 9 ? 2u : (level <= 1 ? 4u : 0u);
    const u32 nseg = (u32)((D + DF_SEG - 1) / DF_SEG);
    const u32 zhdr = zlib_header_word(a, level);
    const u64 bound = zcg_encode_bound(&a->compression, D);
    const DfWs y = df_ws(D, n);
    if (nseg && (ws_bytes < y.total || y.b.tot >= (1ull << 31))) return hipErrorInvalidValue;
    // zlib's configuration_table: max_chain (capped for the GPU) and nice_length
    static const u32 chain[10] = {0, 4, 8, 32, 16, 32, ZCG_DF_CHAIN6, 64, 64, 64};
    static const u32 nice[10] = {0, 8, 16, 32, 16, 32, 128, 128, 258, 258};
    u8* w = (u8*)ws;
    if (nseg) {
        if (hipError_t e = lds_attr_once((const void*)deflate_segment, (int)sizeof(DefLds)); e != hipSuccess)
            return e;
        for (u32 s0 = 0; s0 < n; s0 += y.b.sm) {
            const u32 scnt = batch_count(s0, n, y.b.sm);
            for (u32 c0 = s0; c0 < s0 + scnt && level > 0; c0 += y.b.m) {
                const u32 cnt = batch_count(c0, s0 + scnt, y.b.m);
                const u64 tot = (u64)cnt * D;
                const u32 G = (u32)((tot + 255) / 256);
                u32 *keys = (u32*)(w + y.c.ka), *vals = (u32*)(w + y.c.va), *prev = (u32*)(w + y.c.prev);
                hipLaunchKernelGGL(df_keys, dim3(G), dim3(256), 0, s, d_chunks, c0, D, tot, t, keys, vals);
                hipError_t e = sort_pairs_u32(w + y.c.cub, y.c.cub_bytes, keys, (u32*)(w + y.c.kb), vals,
                                              (u32*)(w + y.c.vb), tot, 24 + id_bits(cnt), s, &keys, &vals);
                if (e == hipSuccess) e = launch_chain_links(tot, keys, vals, prev, s);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(df_best, dim3(G), dim3(256), 0, s, d_chunks, c0, D, tot, t, chain[level],
                                   nice[level], (const u32*)prev, (u32*)(w + y.off_match) + (u64)(c0 - s0) * D);
            }
            const u64 nb = (u64)scnt * nseg;
            if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
            hipLaunchKernelGGL(deflate_segment, dim3((u32)nb), dim3(64), sizeof(DefLds), s, d_chunks, s0, scnt, D,
                               nseg, bound, t, level, (const u32*)(w + y.off_match));
        }
    }
    hipLaunchKernelGGL(deflate_finalize, dim3(n), dim3(256), 0, s, d_chunks, n, D, nseg, bound, xfl, zhdr,
                       (u64*)d_out_len, d_status);
    return launch_stream_checksum(zhdr, d_chunks, n, D, t, (const u64*)d_out_len, (const i32*)d_status, nullptr, s);
}

}  // namespace zcg
