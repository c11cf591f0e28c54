// zcg_bz2_enc.hip — GPU bzip2 encoder: write_chunk for CompressionType::Bzip2
// (src/compression/bzip.rs:36-45: bzip2-rs BzEncoder = libbz2 1.0.x
// BZ2_bzCompressInit(blockSize100k = block_size, verbosity 0, workFactor 30)).
//
// The reference pins no bzip2 encoder bytes (its own doc-spec encode vector
// differs from libbz2, bzip.rs:83-84), so parity is: the stream is a valid
// single bzip2 stream ("BZh" + level, blocks, end-of-stream record, combined
// CRC) that libbz2 — the reference's decoder — decodes to exactly the
// serialised chunk, with every block inside libbz2's size limits for that
// level.  The stages follow libbz2's published encoder (compress.c,
// blocksort.c, huffman.c); the work is laid out for the GPU:
//
//   1. bze_rle1 (one wave per chunk): RLE1 (runs of 4..255 equal bytes ->
//      4 bytes + count), run bookkeeping by wave ballots, 64 input bytes per
//      step; block cuts at piece boundaries with at most 100000*L-19 bytes per
//      block (libbz2's nblockMAX); the block CRC (MSB-first CRC32 of the
//      original bytes) as 64 lane segments combined in GF(2).
//   2. bze_layout / bze_compact: all blocks of the sub-batch are laid out back
//      to back in one text of T bytes.
//   3. Burrows-Wheeler sort of every block's cyclic rotations at once: prefix
//      doubling over the whole text (hipCUB radix sorts of (rank[i],
//      rank[i+h]) pairs, ranks = SA positions of group heads).  Only positions
//      in unresolved groups are re-sorted each round (Larsson-Sadakane), and a
//      block drops out once h reaches its length (its remaining ties are equal
//      rotations: any order of them decodes to the same text).
//   4. bze_block (one 256-thread workgroup per block): BWT last column and
//      origPtr; move-to-front + RUNA/RUNB zero-run coding (wave 0: MTF list in
//      one VGPR per lane, one ballot per run of equal L bytes); then libbz2's
//      table selection (nGroups by nMTF, initial partition, 4 refinement
//      iterations over 50-symbol groups, hbMakeCodeLengths with maxLen 17) with
//      the groups spread over the workgroup; selector MTF; the block's bit
//      stream written at per-thread bit offsets (block scan).
//   5. bze_assemble (one workgroup per chunk): "BZh"+L, the blocks'
//      bit streams concatenated at bit granularity, 0x177245385090 + combined
//      CRC, zero padding to a byte; written straight into the chunk's dst.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "zcg_common.h"
#include "zcg_encode_plan.h"

namespace zcg {
namespace {

constexpr u32 BZE_T = 256;            // threads of the per-block / per-chunk workgroups
constexpr u32 BZE_GSIZE = 50;         // BZ_G_SIZE
constexpr u32 BZE_MAXSYM = 258;       // BZ_MAX_ALPHA_SIZE
constexpr u32 BZE_MAXSEL = 18002;     // BZ_MAX_SELECTORS
constexpr u32 BZE_MAXLEN = 17;        // libbz2 1.0.x code length limit for encoding
constexpr u64 BZE_SUB_BYTES = 128ull << 20;  // input bytes per sub-batch (workspace bound)

constexpr u32 BZE_CRC_POLY = 0x04C11DB7u;
struct BzeCrcTable {
    u32 t[256];
    constexpr BzeCrcTable() : t() {
        for (u32 i = 0; i < 256; i++) {
            u32 c = i << 24;
            for (int k = 0; k < 8; k++) c = (c << 1) ^ ((c & 0x80000000u) ? BZE_CRC_POLY : 0u);
            t[i] = c;
        }
    }
};
static __constant__ BzeCrcTable g_bze_crc = BzeCrcTable();

__device__ inline u32 bze_mulmod(u32 a, u32 b) {
    u32 r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80000000u) ? BZE_CRC_POLY : 0u);
        if ((a >> i) & 1) r ^= b;
    }
    return r;
}
__device__ inline u32 bze_xpow8(u64 n) {
    u32 r = 1, p = 0x100;  // x^8
    while (n) {
        if (n & 1) r = bze_mulmod(p, r);
        p = bze_mulmod(p, p);
        n >>= 1;
    }
    return r;
}

// ---- layout of one sub-batch's workspace ------------------------------------
struct BzeChunkInfo {
    u32 rle_len;   // RLE1 bytes of the chunk
    u32 nblk;      // blocks of the chunk
    u32 text_off;  // offset of the chunk's RLE1 bytes in the compacted text
    u32 blk0;      // global id of the chunk's first block
};
struct BzeLocalBlk {
    u32 start, len, crc;     // start/len in the chunk's RLE1 bytes
    u32 in_start, in_end;    // the block's original bytes [in_start, in_end)
    u32 pad[3];
};
struct BzeBlk {
    u32 start, len, crc, chunk;  // start/len in the text
    u32 orig, nbits, sym_off, pad;
    u64 out_off, out_cap;        // bit-stream scratch (bytes)
    u64 bit_off;                 // bit offset in the chunk's stream (bze_assemble)
    u64 pad2;
};
struct BzeCounters {
    u32 T, NB, maxlen, nsel;
    u64 out_total;
};

struct BzeLayout {
    u32 m;        // chunks per sub-batch
    u64 D, R;     // chunk bytes, RLE1 slot bytes
    u32 L;        // level 1..9
    u32 bmax;     // max RLE1 bytes per block
    u32 maxb;     // max blocks per chunk
    u64 tmax;     // max text bytes
    u64 nbmax;    // max blocks
    u64 outmax;   // bit-stream scratch bytes
    u64 cub_bytes;
    u64 off_rle, off_cinfo, off_lblk, off_blk, off_cnt, off_text, off_blkof, off_rank, off_sa,
        off_ka, off_kb, off_va, off_vb, off_u, off_sa_scan, off_sb_scan, off_flags, off_out, off_cub,
        total;
};

__host__ __device__ inline u64 al256(u64 x) { return (x + 255) & ~255ull; }

u64 cub_temp_bytes(u64 tmax);

BzeLayout make_layout(u64 D, u32 L, u32 n) {
    BzeLayout y{};
    y.D = D;
    y.L = L;
    u64 m = D ? BZE_SUB_BYTES / D : n;
    if (m < 1) m = 1;
    if (m > n) m = n;
    if (m > 4096) m = 4096;
    y.m = (u32)m;
    y.R = al256(D + D / 4 + 64);
    y.bmax = 100000u * L - 19u;
    y.maxb = (u32)(y.R / (y.bmax - 4) + 2);
    y.tmax = y.R * y.m;
    y.nbmax = (u64)y.maxb * y.m;
    y.outmax = y.tmax * 17 / 8 + y.nbmax * (24576 + 512);
    y.cub_bytes = cub_temp_bytes(y.tmax);
    WsCarve ws;
    y.off_rle = ws.take(y.R * y.m);
    y.off_cinfo = ws.take(sizeof(BzeChunkInfo) * y.m);
    y.off_lblk = ws.take(sizeof(BzeLocalBlk) * y.nbmax);
    y.off_blk = ws.take(sizeof(BzeBlk) * y.nbmax);
    y.off_cnt = ws.take(sizeof(BzeCounters));
    y.off_text = ws.take(y.tmax + 16);
    y.off_blkof = ws.take(4 * y.tmax);
    y.off_rank = ws.take(4 * y.tmax);
    y.off_sa = ws.take(4 * y.tmax);
    y.off_ka = ws.take(8 * y.tmax);
    y.off_kb = ws.take(8 * y.tmax);
    y.off_va = ws.take(4 * y.tmax);
    y.off_vb = ws.take(4 * y.tmax);
    y.off_u = ws.take(4 * y.tmax);
    y.off_sa_scan = ws.take(4 * y.tmax);
    y.off_sb_scan = ws.take(4 * y.tmax);
    y.off_flags = ws.take(y.tmax);
    y.off_out = ws.take(y.outmax);
    y.off_cub = ws.take(y.cub_bytes);
    y.total = ws.total();
    return y;
}

struct MaxU32 {
    __device__ __forceinline__ u32 operator()(u32 a, u32 b) const { return a > b ? a : b; }
};

u64 cub_temp_bytes(u64 tmax) {
    size_t b1 = 0, b2 = 0, b3 = 0;
    hipcub::DoubleBuffer<u64> k(nullptr, nullptr);
    hipcub::DoubleBuffer<u32> v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k, v, (int)tmax, 0, 62);
    size_t b4 = 0;
    hipcub::DoubleBuffer<u32> k32(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b4, k32, v, (int)tmax, 0, 32);
    b1 = b1 > b4 ? b1 : b4;
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b2, (u32*)nullptr, (u32*)nullptr, MaxU32(), (int)tmax);
    (void)hipcub::DeviceSelect::Flagged(nullptr, b3, (u32*)nullptr, (u8*)nullptr, (u32*)nullptr,
                                        (u32*)nullptr, (int)tmax);
    size_t b = b1 > b2 ? b1 : b2;
    b = b > b3 ? b : b3;
    return al256(b + 256);
}

// ---- wave helpers --------------------------------------------------------------
__device__ __forceinline__ u64 lanemask_lt() {
    const u32 l = lane_id();
    return l ? (~0ull >> (64 - l)) : 0ull;
}
__device__ __forceinline__ u64 wave_max_u64(u64 x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 y = __shfl_xor(x, d);
        x = y > x ? y : x;
    }
    return x;
}

// ---- 1. RLE1 + block cuts + block CRCs (one wave per chunk) ---------------------
// libbz2 ADD_CHAR_TO_BLOCK / flush_RL: a run of length l is cut into pieces of
// at most 255; a piece of k >= 4 bytes is written as 4 bytes + (k - 4), a
// shorter piece verbatim.  Per input byte with run index k and piece index
// q = k % 255: it emits itself if q < 4, and the count byte q - 3 if it ends a
// piece (q == 254, next byte differs, or end of input) with q >= 3.  Blocks are
// cut only between pieces, so "4 bytes + count" never straddles two blocks.
__global__ __launch_bounds__(64) void bze_rle1(const zcg_chunk* __restrict__ chunks, u32 c0, u32 cnt,
                                               u64 D0, DType t, BzeLayout y, u8* __restrict__ ws) {
    const u32 ci = blockIdx.x;
    if (ci >= cnt) return;
    const int lane = lane_id();
    const zcg_chunk ch = chunks[c0 + ci];
    const u64 D = ch.src_len >= D0 ? D0 : 0;  // a short src reads nothing (INVALID_DATA in bze_assemble)
    const gu8* src = (const gu8*)ch.src;
    gu8* out = (gu8*)(ws + y.off_rle + (u64)ci * y.R);
    BzeLocalBlk* lb = (BzeLocalBlk*)(ws + y.off_lblk) + (u64)ci * y.maxb;
    BzeChunkInfo* info = (BzeChunkInfo*)(ws + y.off_cinfo) + ci;
    const u32 bmax = y.bmax;
    auto byte_at = [&](u64 p) -> u32 { return norm_byte(src[swap_pos(p, t)], t); };

    u32 run_sym = 0x100;   // symbol of the run that the previous byte belongs to (none)
    u32 carry_k = 0;       // run index of the previous byte
    u32 out_pos = 0;       // RLE1 bytes emitted
    u32 bs = 0;            // current block start (RLE1 bytes)
    u32 lastb = 0;         // last piece boundary seen (RLE1 position)
    u32 lastb_in = 0;      // its input position
    u32 in_bs = 0;         // input position of the current block's first byte
    u32 nb = 0;            // blocks closed
    const u32 maxb = y.maxb;

    for (u64 w = 0; w < D; w += 64) {
        const u64 p = w + lane;
        const bool valid = p < D;
        const u32 b = valid ? byte_at(p) : 0x200u;
        const u32 nx = (w + 64 < D) ? byte_at(w + 64) : 0x300u;  // look-ahead byte (scalar)
        u32 prev = __shfl_up(b, 1);
        if (lane == 0) prev = run_sym;
        const bool st = valid && b != prev;
        const u64 S = __ballot(st);
        // run index of this byte
        const u64 upto = S & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
        u32 k;
        if (upto) k = (u32)lane - (63u - (u32)__builtin_clzll(upto));
        else k = carry_k + 1 + (u32)lane;
        const u32 q = k % 255u;
        const bool next_differs = (lane == 63) ? (nx != b) : (((S >> (lane + 1)) & 1ull) != 0 || p + 1 >= D);
        const bool piece_end = valid && (q == 254u || next_differs);
        const u32 e1 = (valid && q < 4u) ? 1u : 0u;
        const u32 e2 = (piece_end && q >= 3u) ? 1u : 0u;
        const u64 m1 = __ballot(e1 != 0), m2 = __ballot(e2 != 0);
        const u64 lt = lanemask_lt();
        const u32 excl = (u32)(__popcll(m1 & lt) + __popcll(m2 & lt));
        const u32 total = (u32)(__popcll(m1) + __popcll(m2));
        const u32 opos = out_pos + excl;
        const bool bnd = valid && q == 0u;  // a piece starts here
        if (out_pos + total > bs + bmax) {
            // close the block at the last piece boundary <= bs + bmax
            u64 cand = (bnd && opos <= bs + bmax && opos > bs) ? (((u64)opos << 32) | (u32)p) : 0ull;
            cand = wave_max_u64(cand);
            u32 cut = (u32)(cand >> 32), cut_i = (u32)cand;
            if (cand == 0ull) { cut = lastb; cut_i = lastb_in; }
            cut = __builtin_amdgcn_readfirstlane(cut);
            cut_i = __builtin_amdgcn_readfirstlane(cut_i);
            if (nb < maxb && lane == 0) {
                lb[nb].start = bs;
                lb[nb].len = cut - bs;
                lb[nb].in_start = in_bs;
                lb[nb].in_end = cut_i;
            }
            nb++;
            bs = cut;
            in_bs = cut_i;
        }
        const u64 B = __ballot(bnd);
        if (B) {
            const int hl = 63 - __builtin_clzll(B);
            lastb = __builtin_amdgcn_readlane(opos, hl);
            lastb_in = __builtin_amdgcn_readlane((u32)p, hl);
        }
        if (e1) out[opos] = (u8)b;
        if (e2) out[opos + e1] = (u8)(q - 3u);
        run_sym = __builtin_amdgcn_readlane(b, 63);
        carry_k = __builtin_amdgcn_readlane(k, 63);
        out_pos += total;
    }
    if (out_pos > bs) {
        if (nb < maxb && lane == 0) {
            lb[nb].start = bs;
            lb[nb].len = out_pos - bs;
            lb[nb].in_start = in_bs;
            lb[nb].in_end = (u32)D;
        }
        nb++;
    }
    __threadfence_block();
    // block CRCs over the original (serialised) bytes, MSB-first CRC32
    for (u32 bi = 0; bi < nb && bi < maxb; bi++) {
        const u64 a = __builtin_amdgcn_readfirstlane(lb[bi].in_start);
        const u64 e = __builtin_amdgcn_readfirstlane(lb[bi].in_end);
        const u64 len = e - a;
        const u64 seg = (len + 63) / 64;
        const u64 s0 = a + (u64)lane * seg;
        const u64 s1 = (s0 + seg < e) ? s0 + seg : e;
        u32 c = 0xFFFFFFFFu;
        for (u64 q2 = s0; q2 < s1; q2++) c = (c << 8) ^ g_bze_crc.t[((c >> 24) ^ byte_at(q2)) & 0xFF];
        c = ~c;
        const u64 my_len = s1 > s0 ? s1 - s0 : 0;
        const u32 xs = bze_xpow8(seg);
        u32 tot = 0;
        for (int l = 0; l < 64; l++) {
            const u32 cl = __shfl(c, l);
            const u64 ll = __shfl(my_len, l);
            if (ll == 0) continue;
            const u32 sh = (ll == seg) ? xs : bze_xpow8(ll);
            tot = bze_mulmod(sh, tot) ^ cl;
        }
        if (lane == 0) lb[bi].crc = tot;
    }
    if (lane == 0) {
        info->rle_len = out_pos;
        info->nblk = nb <= maxb ? nb : 0xFFFFFFFFu;  // overflow: reported by the layout pass
    }
}

// ---- 2. layout of the text and the global block table (one thread) ----------------
__global__ void bze_layout(u32 cnt, BzeLayout y, u8* __restrict__ ws) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    BzeChunkInfo* info = (BzeChunkInfo*)(ws + y.off_cinfo);
    const BzeLocalBlk* lb = (const BzeLocalBlk*)(ws + y.off_lblk);
    BzeBlk* gb = (BzeBlk*)(ws + y.off_blk);
    BzeCounters* cn = (BzeCounters*)(ws + y.off_cnt);
    u32 T = 0, NB = 0, maxlen = 0;
    u64 out = 0;
    for (u32 c = 0; c < cnt; c++) {
        info[c].text_off = T;
        info[c].blk0 = NB;
        const u32 nb = info[c].nblk == 0xFFFFFFFFu ? 0u : info[c].nblk;
        for (u32 k = 0; k < nb; k++) {
            const BzeLocalBlk l = lb[(u64)c * y.maxb + k];
            BzeBlk g;
            g.start = T + l.start;
            g.len = l.len;
            g.crc = l.crc;
            g.chunk = c;
            g.orig = 0;
            g.nbits = 0;
            g.sym_off = g.start + NB + k;  // room for the EOB symbol of every block (nMTF <= len + 1)
            g.pad = 0;
            g.out_off = out;
            g.out_cap = ((u64)l.len * 17 / 8 + 24576 + 256) & ~15ull;
            out += g.out_cap;
            gb[NB + k] = g;
            maxlen = l.len > maxlen ? l.len : maxlen;
        }
        NB += nb;
        T += info[c].rle_len;
    }
    cn->T = T;
    cn->NB = NB;
    cn->maxlen = maxlen;
    cn->nsel = 0;
    cn->out_total = out;
}

// ---- 3. compact the RLE1 slots into one text, block id per position ----------------
__global__ __launch_bounds__(BZE_T) void bze_compact(u32 cnt, BzeLayout y, u8* __restrict__ ws) {
    const u32 c = blockIdx.x;
    if (c >= cnt) return;
    const BzeChunkInfo info = ((const BzeChunkInfo*)(ws + y.off_cinfo))[c];
    const BzeBlk* gb = (const BzeBlk*)(ws + y.off_blk);
    const u8* rle = ws + y.off_rle + (u64)c * y.R;
    u8* text = ws + y.off_text;
    u32* blkof = (u32*)(ws + y.off_blkof);
    const u32 nb = info.nblk == 0xFFFFFFFFu ? 0u : info.nblk;
    for (u32 k = 0; k < nb; k++) {
        const BzeBlk g = gb[info.blk0 + k];
        for (u32 i = threadIdx.x; i < g.len; i += BZE_T) {
            text[g.start + i] = rle[g.start - info.text_off + i];
            blkof[g.start + i] = info.blk0 + k;
        }
    }
}

// ---- 4. prefix-doubling rotation sort -------------------------------------------------
// The first sort's 32-bit key: the block index above the rotation's first
// dpre bytes (dpre = 3 while the sub-batch has <= 256 blocks, fewer bytes
// for more blocks), so one 4-pass radix sort of (u32, u32) pairs orders all
// blocks' rotations by their prefixes.
__global__ void bze_init_keys(u32 T, const u8* __restrict__ text, const u32* __restrict__ blkof,
                              const BzeBlk* __restrict__ gb, u32 dpre, u32* __restrict__ keys,
                              u32* __restrict__ vals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const u32 b = blkof[i];
    const u32 s = gb[b].start, n = gb[b].len;
    u32 loc = i - s;
    u32 v = 0;
    for (u32 d = 0; d < dpre; d++) {
        v = (v << 8) | text[s + loc];
        loc = (loc + 1 == n) ? 0u : loc + 1;
    }
    keys[i] = (b << (8 * dpre)) | v;
    vals[i] = i;
}

// head positions of equal-key runs (scanned with max -> first index of the run)
template <typename K>
__global__ void bze_heads(u32 n, const K* __restrict__ keys, u32 shift, u32* __restrict__ out) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool h = (j == 0) || ((keys[j] >> shift) != (keys[j - 1] >> shift));
    out[j] = h ? j : 0u;
}

// first sort: SA, ranks, and the unresolved positions
__global__ void bze_rank0(u32 T, const u32* __restrict__ keys, const u32* __restrict__ vals,
                          const u32* __restrict__ headpos, const u32* __restrict__ blkof,
                          const BzeBlk* __restrict__ gb, u32 dpre, u32* __restrict__ rank, u32* __restrict__ sa,
                          u8* __restrict__ flags) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    const u32 i = vals[p];
    rank[i] = headpos[p];
    sa[p] = i;
    const bool head = (p == 0) || keys[p] != keys[p - 1];
    const bool nhead = (p + 1 == T) || keys[p + 1] != keys[p];
    // the keys lead with the block index, so SA position p lies in the same
    // block as text position i: blkof[p] is a coalesced read, blkof[i] a gather
    const u32 len = gb[blkof[p]].len;
    flags[p] = (!(head && nhead) && dpre < len) ? 1 : 0;
}

__global__ void bze_keys(u32 n, u32 h, u32 rb, const u32* __restrict__ U, const u32* __restrict__ rank,
                         const u32* __restrict__ blkof, const BzeBlk* __restrict__ gb,
                         u64* __restrict__ keys, u32* __restrict__ vals) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 i = U[j];
    const u32 ri = rank[i];
    const u32 b = blkof[ri];  // the group head's SA position is in i's block (U is in SA order: ascending reads)
    const u32 s = gb[b].start, len = gb[b].len;
    u32 nx = i + h;  // h < len for every kept position
    if (nx >= s + len) nx -= len;
    keys[j] = ((u64)ri << rb) | rank[nx];
    vals[j] = i;
}

// SA position of every re-sorted entry, and the head position of its new group
__global__ void bze_sapos(u32 n, u32 rb, const u64* __restrict__ keys, const u32* __restrict__ vals,
                          const u32* __restrict__ firstj, u32* __restrict__ sa, u32* __restrict__ out) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u64 k = keys[j];
    const u32 sp = (u32)(k >> rb) + (j - firstj[j]);
    sa[sp] = vals[j];
    const bool sub = (j == 0) || k != keys[j - 1];
    out[j] = sub ? sp : 0u;
}

__global__ void bze_update(u32 n, u32 h2, u32 rb, const u64* __restrict__ keys, const u32* __restrict__ vals,
                           const u32* __restrict__ newrank, const u32* __restrict__ blkof,
                           const BzeBlk* __restrict__ gb, u32* __restrict__ rank, u8* __restrict__ flags) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 i = vals[j];
    rank[i] = newrank[j];
    const u64 k = keys[j];
    const bool head = (j == 0) || k != keys[j - 1];
    const bool nhead = (j + 1 == n) || keys[j + 1] != k;
    const u32 len = gb[blkof[(u32)(k >> rb)]].len;  // (the old group head: same block, ascending)
    flags[j] = (!(head && nhead) && h2 < len) ? 1 : 0;
}


// ---- 4b. small groups sorted in LDS --------------------------------------------------
// After the first (4-byte) sort, a workgroup takes the groups whose heads lie
// in its tile of BZE_LC SA positions (a group may run past the tile; one
// larger than BZE_LN stays for the global rounds) and refines them in LDS:
// 8 more bytes of each unresolved rotation per round (cyclic within its
// block), a bitonic sort by (tie run, bytes) — or, once every tie run is
// short, an insertion sort of each run by its head thread — and new tie
// runs, for up to BZE_LROUNDS rounds.  Resolved positions get their final SA slot and rank;
// rotations still tied afterwards keep their run head as rank and stay
// flagged for the global prefix-doubling rounds (whose ranks only need to be
// at least 4-byte accurate, which refined ranks are).  A tie that reaches
// the block length is an equal rotation: any order decodes the same.
constexpr u32 BZE_LC = 1024;
constexpr u32 BZE_LN = 2 * BZE_LC;
constexpr u32 BZE_LROUNDS = 4;  // (prefix + 32 bytes; deeper ties go to the global rounds; 6/8/12 rounds:
                                // 221/218/214 GB per 512-chunk encode against 227, 1-5 % slower)
constexpr u32 BZE_ISORT = 64;   // tie runs up to this long are insertion-sorted by one thread

__device__ __forceinline__ u64 bze_key8(const u8* __restrict__ text, u32 s, u32 len, u32 loc) {
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        v = (v << 8) | text[s + loc];
        loc = (loc + 1 == len) ? 0u : loc + 1;
    }
    return v;
}

__global__ __launch_bounds__(BZE_T) void bze_lds_sort(u32 T, const u8* __restrict__ text,
                                                      const u32* __restrict__ blkof, const BzeBlk* __restrict__ gb,
                                                      const u32* __restrict__ headpos, u32 dpre,
                                                      u32* __restrict__ sa, u32* __restrict__ rank,
                                                      u8* __restrict__ flags) {
    __shared__ u64 K[BZE_LN];
    __shared__ u32 R[BZE_LN];
    __shared__ u32 P[BZE_LN];
    __shared__ u32 part[BZE_T];
    __shared__ u32 s_a, s_last, s_b, s_tied, s_maxrun;
    const u32 tid = threadIdx.x;
    const u32 t0 = blockIdx.x * BZE_LC;
    const u32 t1 = (T - t0) < BZE_LC ? T : t0 + BZE_LC;
    if (tid == 0) { s_a = 0xFFFFFFFFu; s_last = 0; s_b = 0xFFFFFFFFu; }
    __syncthreads();
    for (u32 p = t0 + tid; p < t1; p += BZE_T)
        if (headpos[p] == p) { atomicMin(&s_a, p); atomicMax(&s_last, p); }
    __syncthreads();
    const u32 a = s_a;
    if (a == 0xFFFFFFFFu) return;  // inside a group that started before the tile
    {
        const u32 lim = (T - a) < BZE_LN ? T : a + BZE_LN;  // b may be at most a + BZE_LN
        for (u32 p = t1 + tid; p <= lim; p += BZE_T)
            if (p == T || headpos[p] == p) atomicMin(&s_b, p);
    }
    __syncthreads();
    const u32 b = s_b != 0xFFFFFFFFu ? s_b : s_last;  // else the last group is too large: leave it
    const u32 n = b - a;
    if (n < 2) return;
    u32 N = 2;
    while (N < n) N <<= 1;
    for (u32 k = tid; k < N; k += BZE_T) {
        if (k < n) {
            const u32 p = a + k, pos = sa[p];
            P[k] = pos;
            if (flags[p]) {
                const u32 bi = blkof[p], st = gb[bi].start, len = gb[bi].len;  // (SA and text ranges of a block coincide)
                R[k] = headpos[p] - a;
                K[k] = bze_key8(text, st, len, (pos - st + dpre) % len);
            } else {
                R[k] = k;
                K[k] = 0;
            }
        } else {
            R[k] = 0xFFFFFFFFu;
            K[k] = ~0ull;
            P[k] = 0;
        }
    }
    __syncthreads();
    u32 depth = dpre;
    // the longest group (capped) picks the first round's sort too
    if (tid == 0) s_maxrun = 0;
    __syncthreads();
    for (u32 k = tid; k < n; k += BZE_T) {
        if (R[k] != k || k + 1 >= n || R[k + 1] != k) continue;
        u32 e = k + 1;
        while (e < n && R[e] == k && e - k <= BZE_ISORT) e++;
        atomicMax(&s_maxrun, e - k);
    }
    __syncthreads();
    for (u32 round = 0; round < BZE_LROUNDS; round++) {
        if (s_maxrun <= BZE_ISORT) {
            // every tie run is short: its head thread insertion-sorts it by K
            for (u32 k = tid; k < n; k += BZE_T) {
                if (R[k] != k || k + 1 >= n || R[k + 1] != k) continue;
                u32 e = k + 1;
                while (e < n && R[e] == k) e++;
                for (u32 i = k + 1; i < e; i++) {
                    const u64 kv = K[i];
                    const u32 pv = P[i];
                    u32 j = i;
                    while (j > k && K[j - 1] > kv) { K[j] = K[j - 1]; P[j] = P[j - 1]; j--; }
                    K[j] = kv;
                    P[j] = pv;
                }
            }
            __syncthreads();
        } else
        // bitonic sort by (R, K)
        for (u32 kk = 2; kk <= N; kk <<= 1)
            for (u32 j = kk >> 1; j > 0; j >>= 1) {
                for (u32 i = tid; i < N; i += BZE_T) {
                    const u32 x = i ^ j;
                    if (x > i) {
                        const bool up = (i & kk) == 0;
                        const bool gt = R[i] > R[x] || (R[i] == R[x] && K[i] > K[x]);
                        const bool lt = R[i] < R[x] || (R[i] == R[x] && K[i] < K[x]);
                        if (up ? gt : lt) {
                            const u32 r = R[i]; R[i] = R[x]; R[x] = r;
                            const u64 q = K[i]; K[i] = K[x]; K[x] = q;
                            const u32 w = P[i]; P[i] = P[x]; P[x] = w;
                        }
                    }
                }
                __syncthreads();
            }
        // tie runs: head index by a block max-scan over 16 elements per thread
        const u32 per = (N + BZE_T - 1) / BZE_T;
        const u32 k0 = tid * per;
        u32 m = 0;
        for (u32 q = 0; q < per; q++) {
            const u32 k = k0 + q;
            if (k < n && (k == 0 || R[k] != R[k - 1] || K[k] != K[k - 1])) m = k;
        }
        part[tid] = m;
        __syncthreads();
        u32 carry = 0;
        for (u32 t = 0; t < tid; t++) carry = part[t] > carry ? part[t] : carry;
        __syncthreads();
        if (tid == 0) s_tied = 0;
        __syncthreads();
        // new run id = run head index; tied = the run has >= 2 members and
        // its rotations are not yet compared over their whole length
        // (run heads and tie bits packed in one register per 16 elements)
        u32 hd = carry, tiebits = 0;
        u32 hdq[16];
#pragma unroll
        for (u32 q = 0; q < 16; q++) {
            const u32 k = k0 + q;
            if (q < per && k < n) {
                if (k == 0 || R[k] != R[k - 1] || K[k] != K[k - 1]) hd = k;
                const bool next_same = k + 1 < n && R[k + 1] == R[k] && K[k + 1] == K[k];
                if ((hd != k || next_same) && depth + 8 < gb[blkof[a + k]].len) tiebits |= 1u << q;
            }
            hdq[q] = hd;
        }
        __syncthreads();
#pragma unroll
        for (u32 q = 0; q < 16; q++) {
            const u32 k = k0 + q;
            if (q >= per || k >= n) continue;
            const u32 heads_q = hdq[q];
            if ((tiebits >> q) & 1u) {
                const u32 pos = P[k], bi = blkof[a + k], st = gb[bi].start, len = gb[bi].len;
                R[k] = heads_q;
                K[k] = bze_key8(text, st, len, (pos - st + depth + 8) % len);
                s_tied = 1;
            } else {
                R[k] = k;
                K[k] = 0;
            }
        }
        __syncthreads();
        depth += 8;
        if (!s_tied) break;
        // the longest tie run (capped) picks the next round's sort
        if (tid == 0) s_maxrun = 0;
        __syncthreads();
        for (u32 k = tid; k < n; k += BZE_T) {
            if (R[k] != k || k + 1 >= n || R[k + 1] != k) continue;
            u32 e = k + 1;
            while (e < n && R[e] == k && e - k <= BZE_ISORT) e++;
            atomicMax(&s_maxrun, e - k);
        }
        __syncthreads();
    }
    // write back: SA order, ranks (run heads for ties), flags
    for (u32 k = tid; k < n; k += BZE_T) {
        const u32 p = a + k, pos = P[k];
        const bool was = flags[p] != 0;  // (flagged groups keep their SA ranges)
        sa[p] = pos;
        if (was) {
            const bool t = R[k] != k || (k + 1 < n && R[k + 1] == k);
            rank[pos] = a + R[k];
            flags[p] = t ? 1 : 0;
        }
    }
}

// ---- 5. per-block: BWT column, MTF/RLE2, Huffman tables, bit stream -------------------
struct BzeBlkShared {
    u32 inuse[8];
    u32 orig;
    u32 ninuse, nmtf, ngroups, nsel, alpha;
    u32 hdr_bits;
    u32 tot_bits;
    u8 seqmap[256];
    u32 freq[BZE_MAXSYM];
    u8 len[6][BZE_MAXSYM + 2];
    u64 packed[BZE_MAXSYM];
    u32 rfreq[6][BZE_MAXSYM];
    u32 code[6][BZE_MAXSYM];
    i32 heap[6][BZE_MAXSYM + 4];
    i32 weight[6][2 * BZE_MAXSYM + 4];
    i32 parent[6][2 * BZE_MAXSYM + 4];
    u8 sel[BZE_MAXSEL + 2];
    u32 scan[BZE_T];
    u32 wsum[4];
};

// libbz2 huffman.c BZ2_hbMakeCodeLengths (restated): weights carry the depth
// in the low 8 bits; lengths over maxLen -> halve the frequencies and retry.
// This function follows libbz2's statement by statement (its heap order
// decides the code lengths, and so the bytes), so it carries libbz2's notice:
//   bzip2/libbzip2 version 1.0.8 of 13 July 2019, Copyright (C) 1996-2019
//   Julian Seward <jseward@acm.org>.  Redistribution and use in source and
//   binary forms, with or without modification, are permitted provided that
//   the following conditions are met: 1. Redistributions of source code must
//   retain the above copyright notice, this list of conditions and the
//   following disclaimer.  2. The origin of this software must not be
//   misrepresented; you must not claim that you wrote the original software.
//   If you use this software in a product, an acknowledgment in the product
//   documentation would be appreciated but is not required.  3. Altered
//   source versions must be plainly marked as such, and must not be
//   misrepresented as being the original software.  4. The name of the author
//   may not be used to endorse or promote products derived from this software
//   without specific prior written permission.  THIS SOFTWARE IS PROVIDED BY
//   THE AUTHOR "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT
//   NOT LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR
//   A PARTICULAR PURPOSE ARE DISCLAIMED.  IN NO EVENT SHALL THE AUTHOR BE
//   LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR
//   CONSEQUENTIAL DAMAGES ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE.
// (Altered: a device restatement on LDS arrays, not libbz2's source.)
__device__ void bze_make_lengths(u8* len, const u32* freq, i32 alpha, i32 maxlen, i32* heap, i32* weight,
                                 i32* parent) {
    for (i32 i = 0; i < alpha; i++) weight[i + 1] = (freq[i] == 0 ? 1 : (i32)freq[i]) << 8;
    while (true) {
        i32 nNodes = alpha, nHeap = 0;
        heap[0] = 0;
        weight[0] = 0;
        parent[0] = -2;
        for (i32 i = 1; i <= alpha; i++) {
            parent[i] = -1;
            nHeap++;
            heap[nHeap] = i;
            i32 zz = nHeap, tmp = heap[zz];
            while (weight[tmp] < weight[heap[zz >> 1]]) { heap[zz] = heap[zz >> 1]; zz >>= 1; }
            heap[zz] = tmp;
        }
        auto downheap = [&](i32 z) {
            i32 zz = z, tmp = heap[zz];
            while (true) {
                i32 yy = zz << 1;
                if (yy > nHeap) break;
                if (yy < nHeap && weight[heap[yy + 1]] < weight[heap[yy]]) yy++;
                if (weight[tmp] < weight[heap[yy]]) break;
                heap[zz] = heap[yy];
                zz = yy;
            }
            heap[zz] = tmp;
        };
        while (nHeap > 1) {
            const i32 n1 = heap[1];
            heap[1] = heap[nHeap];
            nHeap--;
            downheap(1);
            const i32 n2 = heap[1];
            heap[1] = heap[nHeap];
            nHeap--;
            downheap(1);
            nNodes++;
            parent[n1] = parent[n2] = nNodes;
            const i32 w1 = weight[n1], w2 = weight[n2];
            const i32 d1 = w1 & 0xff, d2 = w2 & 0xff;
            weight[nNodes] = ((w1 & (i32)0xffffff00) + (w2 & (i32)0xffffff00)) | (1 + (d1 > d2 ? d1 : d2));
            parent[nNodes] = -1;
            nHeap++;
            heap[nHeap] = nNodes;
            i32 zz = nHeap, tmp = heap[zz];
            while (weight[tmp] < weight[heap[zz >> 1]]) { heap[zz] = heap[zz >> 1]; zz >>= 1; }
            heap[zz] = tmp;
        }
        bool too_long = false;
        for (i32 i = 1; i <= alpha; i++) {
            i32 j = 0, k = i;
            while (parent[k] >= 0) { k = parent[k]; j++; }
            len[i - 1] = (u8)j;
            if (j > maxlen) too_long = true;
        }
        if (!too_long) break;
        for (i32 i = 1; i <= alpha; i++) {
            i32 j = weight[i] >> 8;
            j = 1 + (j / 2);
            weight[i] = j << 8;
        }
    }
}

// MSB-first bit writer into zeroed 32-bit words (word MSB = first bit)
struct BitW {
    u32* words;
    u64 pos;  // bit position
    u64 acc;  // pending bits, left-aligned in the low `n` bits
    u32 n;
    __device__ void init(u32* w, u64 p) {
        words = w;
        pos = p;
        acc = 0;
        n = 0;
    }
    __device__ __forceinline__ void put(u32 nb, u32 v) {
        acc = (acc << nb) | (v & ((1u << nb) - 1u));
        n += nb;
        u32 room = 32 - (u32)(pos & 31);
        while (n >= room) {
            const u32 bits = (u32)(acc >> (n - room)) & (room == 32 ? 0xFFFFFFFFu : ((1u << room) - 1u));
            atomicOr(&words[pos >> 5], bits);
            pos += room;
            n -= room;
            room = 32;
        }
    }
    __device__ void flush() {
        if (n) {
            const u32 room = 32 - (u32)(pos & 31);
            const u32 v = (u32)(acc & ((1ull << n) - 1ull)) << (room - n);
            atomicOr(&words[pos >> 5], v);
            pos += n;
            n = 0;
        }
    }
};

__device__ u32 bze_block_scan(u32 x, u32* tmp, u32* total) {
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    u32 incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 yv = __shfl_up(incl, d);
        if (lane >= (u32)d) incl += yv;
    }
    if (lane == 63) tmp[w] = incl;
    __syncthreads();
    u32 base = 0;
    for (u32 k = 0; k < w; k++) base += tmp[k];
    *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    __syncthreads();
    return base + incl - x;
}

__global__ __launch_bounds__(BZE_T) void bze_block(u32 NB, BzeLayout y, u8* __restrict__ ws) {
    const u32 b = blockIdx.x;
    if (b >= NB) return;
    __shared__ BzeBlkShared sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    BzeBlk* gbp = (BzeBlk*)(ws + y.off_blk) + b;
    const BzeBlk g = *gbp;
    const u8* text = ws + y.off_text;
    const u32* sa = (const u32*)(ws + y.off_sa);
    u8* Lb = ws + y.off_ka;                 // BWT last column (keys buffer, free after the sort)
    u16* mtfv = (u16*)(ws + y.off_kb);      // MTF/RLE2 symbols
    const u32 s = g.start, n = g.len;
    u8* L = Lb + s;
    u16* sym = mtfv + g.sym_off;

    if (tid < 8) sh.inuse[tid] = 0;
    for (u32 k = tid; k < BZE_MAXSYM; k += BZE_T) sh.freq[k] = 0;
    __syncthreads();
    // ---- BWT last column, origPtr, symbols in use ----
    for (u32 p = tid; p < n; p += BZE_T) {
        const u32 i = sa[s + p];
        const u32 loc = i - s;
        const u32 c = text[loc == 0 ? s + n - 1 : i - 1];
        L[p] = (u8)c;
        if (loc == 0) sh.orig = p;
        atomicOr(&sh.inuse[c >> 5], 1u << (c & 31));
    }
    __syncthreads();
    if (tid == 0) {
        u32 k = 0;
        for (u32 c = 0; c < 256; c++)
            if ((sh.inuse[c >> 5] >> (c & 31)) & 1) sh.seqmap[c] = (u8)k++;
        sh.ninuse = k;
        sh.alpha = k + 2;
    }
    __syncthreads();
    // ---- MTF + RUNA/RUNB (wave 0, libbz2 generateMTFValues) ----
    if (wave == 0) {
        u32 listw = (4u * lane) | ((4u * lane + 1) << 8) | ((4u * lane + 2) << 16) | ((4u * lane + 3) << 24);
        u32 wr = 0;       // symbols written
        u32 obuf = 0;     // pending symbols, one per lane
        u32 zp = 0;       // pending zero MTF values
        u32 prev_start = 0xFFFFFFFFu;
        u32 last = 0x100;  // seq of the previous L byte
        const u32 eob = sh.ninuse + 1;
        auto put = [&](u32 v) {
            if (lane == (wr & 63)) obuf = v;
            if ((wr & 63) == 63) sym[(wr & ~63u) + lane] = (u16)obuf;
            wr++;
        };
        auto flush_zeros = [&]() {
            if (zp > 0) {
                zp--;
                while (true) {
                    put((zp & 1) ? 1u : 0u);  // RUNB : RUNA
                    if (zp < 2) break;
                    zp = (zp - 2) / 2;
                }
                zp = 0;
            }
        };
        for (u32 w0 = 0; w0 < n; w0 += 64) {
            const u32 p = w0 + lane;
            const bool valid = p < n;
            const u32 sq = valid ? (u32)sh.seqmap[L[p]] : 0x200u;
            u32 pv = __shfl_up(sq, 1);
            if (lane == 0) pv = last;
            u64 S = __ballot(valid && sq != pv);
            while (S) {
                const u32 l = (u32)__builtin_ctzll(S);
                S &= S - 1;
                const u32 a = w0 + l;
                const u32 v = __builtin_amdgcn_readlane(sq, l);
                if (prev_start != 0xFFFFFFFFu) zp += a - prev_start - 1;
                prev_start = a;
                // position of v in the list
                const u32 x = listw ^ (v * 0x01010101u);
                const u32 z = (x - 0x01010101u) & ~x & 0x80808080u;
                const u64 mm = __ballot(z != 0);
                const u32 wn = (u32)__builtin_ctzll(mm);
                const u32 zw = __builtin_amdgcn_readlane(z, wn);
                const u32 bi = (u32)__builtin_ctz(zw) >> 3;
                const u32 pos = 4 * wn + bi;
                if (pos == 0) {
                    zp++;
                } else {
                    flush_zeros();
                    put(pos + 1);
                    const u32 pw = __shfl_up(listw, 1);
                    const u32 shw = (listw << 8) | (lane == 0 ? v : (pw >> 24));
                    const u32 keep = (u32)(0xFFFFFFFFull << (8 * bi + 8));
                    if ((u32)lane < wn) listw = shw;
                    else if ((u32)lane == wn) listw = (shw & ~keep) | (listw & keep);
                }
            }
            last = __builtin_amdgcn_readlane(sq, 63);
        }
        if (prev_start != 0xFFFFFFFFu) zp += n - prev_start - 1;
        flush_zeros();
        put(eob);
        if ((u32)lane < (wr & 63)) sym[(wr & ~63u) + lane] = (u16)obuf;
        if (lane == 0) sh.nmtf = wr;
    }
    __syncthreads();
    const u32 nmtf = sh.nmtf, alpha = sh.alpha;
    for (u32 k = tid; k < nmtf; k += BZE_T) atomicAdd(&sh.freq[sym[k]], 1u);
    __syncthreads();
    // ---- initial tables (libbz2 sendMTFValues) ----
    if (tid == 0) {
        const u32 ng = nmtf < 200 ? 2 : nmtf < 600 ? 3 : nmtf < 1200 ? 4 : nmtf < 2400 ? 5 : 6;
        sh.ngroups = ng;
        i32 nPart = (i32)ng, remF = (i32)nmtf, gs = 0;
        while (nPart > 0) {
            const i32 tFreq = remF / nPart;
            i32 ge = gs - 1, aFreq = 0;
            while (aFreq < tFreq && ge < (i32)alpha - 1) {
                ge++;
                aFreq += (i32)sh.freq[ge];
            }
            if (ge > gs && nPart != (i32)ng && nPart != 1 && (((i32)ng - nPart) % 2 == 1)) {
                aFreq -= (i32)sh.freq[ge];
                ge--;
            }
            for (i32 v = 0; v < (i32)alpha; v++) sh.len[nPart - 1][v] = (v >= gs && v <= ge) ? 0 : 15;
            nPart--;
            gs = ge + 1;
            remF -= aFreq;
        }
        sh.nsel = (nmtf + BZE_GSIZE - 1) / BZE_GSIZE;
    }
    __syncthreads();
    const u32 ng = sh.ngroups, nsel = sh.nsel;
    // groups [g0, g1) of this thread
    const u32 g0 = (u32)((u64)nsel * tid / BZE_T), g1 = (u32)((u64)nsel * (tid + 1) / BZE_T);
    for (int it = 0; it < 4; it++) {
        for (u32 v = tid; v < alpha; v += BZE_T) {
            u64 pk = 0;
            for (u32 tt = 0; tt < ng; tt++) pk |= (u64)sh.len[tt][v] << (10 * tt);
            sh.packed[v] = pk;
        }
        for (u32 k = tid; k < 6 * BZE_MAXSYM; k += BZE_T) (&sh.rfreq[0][0])[k] = 0;
        __syncthreads();
        for (u32 gi = g0; gi < g1; gi++) {
            const u32 a0 = gi * BZE_GSIZE;
            const u32 a1 = a0 + BZE_GSIZE < nmtf ? a0 + BZE_GSIZE : nmtf;
            u64 cost = 0;
            for (u32 k = a0; k < a1; k++) cost += sh.packed[sym[k]];
            u32 bt = 0, bc = 0xFFFFFFFFu;
            for (u32 tt = 0; tt < ng; tt++) {
                const u32 c = (u32)(cost >> (10 * tt)) & 1023u;
                if (c < bc) { bc = c; bt = tt; }
            }
            sh.sel[gi] = (u8)bt;
            for (u32 k = a0; k < a1; k++) atomicAdd(&sh.rfreq[bt][sym[k]], 1u);
        }
        __syncthreads();
        if (tid < ng)
            bze_make_lengths(sh.len[tid], sh.rfreq[tid], (i32)alpha, (i32)BZE_MAXLEN, sh.heap[tid],
                             sh.weight[tid], sh.parent[tid]);
        __syncthreads();
    }
    // ---- canonical codes (hbAssignCodes) ----
    if (tid < ng) {
        u32 minl = 32, maxl = 0;
        for (u32 v = 0; v < alpha; v++) {
            const u32 l = sh.len[tid][v];
            minl = l < minl ? l : minl;
            maxl = l > maxl ? l : maxl;
        }
        u32 vec = 0;
        for (u32 l = minl; l <= maxl; l++) {
            for (u32 v = 0; v < alpha; v++)
                if (sh.len[tid][v] == l) sh.code[tid][v] = vec++;
            vec <<= 1;
        }
    }
    // ---- data bits per thread ----
    u32 my_bits = 0;
    for (u32 gi = g0; gi < g1; gi++) {
        const u32 a0 = gi * BZE_GSIZE;
        const u32 a1 = a0 + BZE_GSIZE < nmtf ? a0 + BZE_GSIZE : nmtf;
        const u32 tt = sh.sel[gi];
        for (u32 k = a0; k < a1; k++) my_bits += sh.len[tt][sym[k]];
    }
    u32 data_total;
    const u32 my_off = bze_block_scan(my_bits, sh.wsum, &data_total);
    // ---- header (thread 0): size first, the selectors keep their group ids ----
    if (tid == 0) {
        u32 nused16 = 0;
        for (u32 i = 0; i < 16; i++) {
            bool any = false;
            for (u32 j = 0; j < 16; j++) any |= (sh.inuse[(i * 16 + j) >> 5] >> ((i * 16 + j) & 31)) & 1;
            nused16 += any;
        }
        u32 hb = 48 + 32 + 1 + 24 + 16 + 16 * nused16 + 3 + 15;
        u32 pos = 0x543210u;  // selector MTF list, 4 bits per entry
        for (u32 i = 0; i < nsel; i++) {
            const u32 v = sh.sel[i];
            u32 j = 0;
            while (((pos >> (4 * j)) & 15u) != v) j++;
            const u32 below = pos & ((1u << (4 * j)) - 1u);
            const u32 above = pos & ~((1u << (4 * j + 4)) - 1u);
            pos = above | (below << 4) | v;
            hb += j + 1;
        }
        for (u32 tt = 0; tt < ng; tt++) {
            i32 curr = sh.len[tt][0];
            hb += 5;
            for (u32 v = 0; v < alpha; v++) {
                const i32 l = sh.len[tt][v];
                hb += 1 + 2 * (u32)(l > curr ? l - curr : curr - l);
                curr = l;
            }
        }
        sh.hdr_bits = hb;
        sh.tot_bits = hb + data_total;
    }
    __syncthreads();
    const u64 need = ((u64)sh.tot_bits + 31) / 32 * 4 + 8;
    u32* outw = (u32*)(ws + y.off_out + g.out_off);
    if (need > g.out_cap) {  // cannot happen with the bound in bze_layout; keep the stream valid-or-nothing
        if (tid == 0) gbp->nbits = 0xFFFFFFFFu;
        return;
    }
    for (u64 k = tid; k < need / 4; k += BZE_T) outw[k] = 0;
    __syncthreads();
    if (tid == 0) {
        BitW bw;
        bw.init(outw, 0);
        bw.put(24, 0x314159u);
        bw.put(24, 0x265359u);
        bw.put(16, g.crc >> 16);
        bw.put(16, g.crc & 0xFFFFu);
        bw.put(1, 0);
        bw.put(24, sh.orig);
        u32 used16 = 0;
        for (u32 i = 0; i < 16; i++) {
            bool any = false;
            for (u32 j = 0; j < 16; j++) any |= (sh.inuse[(i * 16 + j) >> 5] >> ((i * 16 + j) & 31)) & 1;
            used16 |= (any ? 1u : 0u) << i;
            bw.put(1, any ? 1u : 0u);
        }
        for (u32 i = 0; i < 16; i++) {
            if (!((used16 >> i) & 1)) continue;
            for (u32 j = 0; j < 16; j++) bw.put(1, (sh.inuse[(i * 16 + j) >> 5] >> ((i * 16 + j) & 31)) & 1);
        }
        bw.put(3, ng);
        bw.put(15, nsel);
        u32 pos = 0x543210u;
        for (u32 i = 0; i < nsel; i++) {
            const u32 v = sh.sel[i];
            u32 j = 0;
            while (((pos >> (4 * j)) & 15u) != v) j++;
            // move entry j to the front
            const u32 below = pos & ((1u << (4 * j)) - 1u);
            const u32 above = pos & ~((1u << (4 * j + 4)) - 1u);
            pos = above | (below << 4) | v;
            for (u32 k = 0; k < j; k++) bw.put(1, 1);
            bw.put(1, 0);
        }
        for (u32 tt = 0; tt < ng; tt++) {
            i32 curr = sh.len[tt][0];
            bw.put(5, (u32)curr);
            for (u32 v = 0; v < alpha; v++) {
                const i32 l = sh.len[tt][v];
                while (curr < l) { bw.put(2, 2); curr++; }
                while (curr > l) { bw.put(2, 3); curr--; }
                bw.put(1, 0);
            }
        }
        bw.flush();
    }
    {
        BitW bw;
        bw.init(outw, (u64)sh.hdr_bits + my_off);
        for (u32 gi = g0; gi < g1; gi++) {
            const u32 a0 = gi * BZE_GSIZE;
            const u32 a1 = a0 + BZE_GSIZE < nmtf ? a0 + BZE_GSIZE : nmtf;
            const u32 tt = sh.sel[gi];
            for (u32 k = a0; k < a1; k++) {
                const u32 v = sym[k];
                bw.put(sh.len[tt][v], sh.code[tt][v]);
            }
        }
        bw.flush();
    }
    if (tid == 0) {
        gbp->orig = sh.orig;
        gbp->nbits = sh.tot_bits;
    }
}

// ---- 6. per chunk: stream header, blocks at bit offsets, stream footer -----------------
__device__ __forceinline__ u32 bits_from(const u32* w, u64 q, u32 cnt) {
    // cnt (1..32) bits starting at bit q of an MSB-first word stream, right-aligned
    const u64 wi = q >> 5;
    const u64 two = ((u64)w[wi] << 32) | w[wi + 1];
    return (u32)((two << (q & 31)) >> (64 - cnt));
}

__global__ __launch_bounds__(BZE_T) void bze_assemble(const zcg_chunk* __restrict__ chunks, u32 c0, u32 cnt,
                                                      BzeLayout y, u8* __restrict__ ws,
                                                      u64* __restrict__ out_len, i32* __restrict__ status) {
    const u32 c = blockIdx.x;
    if (c >= cnt) return;
    const u32 tid = threadIdx.x;
    const BzeChunkInfo info = ((const BzeChunkInfo*)(ws + y.off_cinfo))[c];
    BzeBlk* gb = (BzeBlk*)(ws + y.off_blk);
    const zcg_chunk ch = chunks[c0 + c];
    __shared__ u32 hdr[4], ftr[4];
    __shared__ u32 bad_s;
    __shared__ u64 total_s, ftr_s;
    const u32 nb = info.nblk == 0xFFFFFFFFu ? 0u : info.nblk;
    if (tid == 0) {
        u32 bad = info.nblk == 0xFFFFFFFFu ? 1u : 0u;
        hdr[0] = 0x425A6830u + y.L;  // "BZh" + level
        hdr[1] = hdr[2] = hdr[3] = 0;
        u64 p = 32;
        u32 comb = 0;
        for (u32 k = 0; k < nb; k++) {
            BzeBlk* g = gb + info.blk0 + k;
            const u32 nbits = g->nbits;
            if (nbits == 0xFFFFFFFFu) bad = 1;
            g->bit_off = p;
            p += nbits;
            comb = ((comb << 1) | (comb >> 31)) ^ g->crc;
        }
        ftr[0] = 0x17724538u;
        ftr[1] = (0x5090u << 16) | (comb >> 16);
        ftr[2] = (comb & 0xFFFFu) << 16;
        ftr[3] = 0;
        ftr_s = p;
        p += 80;
        total_s = (p + 7) / 8;
        bad_s = bad;
    }
    __threadfence_block();
    __syncthreads();
    const u64 total = total_s, F = ftr_s;
    if (ch.src_len < y.D) {  // fewer serialised bytes than the chunk holds (chunk.rs:309-318)
        if (tid == 0) { out_len[c0 + c] = 0; status[c0 + c] = ZCG_ERR_INVALID_DATA; }
        return;
    }
    if (bad_s) {
        if (tid == 0) { out_len[c0 + c] = 0; status[c0 + c] = ZCG_ERR_RUNTIME; }
        return;
    }
    if (total > ch.dst_cap) {
        if (tid == 0) { out_len[c0 + c] = total; status[c0 + c] = ZCG_ERR_OUTPUT_TOO_SMALL; }
        return;
    }
    gu8* dst = (gu8*)ch.dst;
    const BzeBlk* cb = gb + info.blk0;
    const u64 nwords = (total + 3) / 4;
    for (u64 wd = tid; wd < nwords; wd += BZE_T) {
        u64 pos = wd * 32;
        const u64 pend = pos + 32;
        // first block whose end is past pos (binary search over the chunk's blocks)
        u32 lo = 0, hi = nb;
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (cb[mid].bit_off + cb[mid].nbits <= pos) lo = mid + 1; else hi = mid;
        }
        u32 k = lo;
        u32 val = 0, got = 0;
        while (pos < pend) {
            u64 ss, se;
            const u32* src;
            if (pos < 32) { ss = 0; se = 32; src = hdr; }
            else if (pos >= F) { ss = F; se = F + 80; src = ftr; }
            else {
                while (k < nb && cb[k].bit_off + cb[k].nbits <= pos) k++;
                ss = cb[k].bit_off;
                se = ss + cb[k].nbits;
                src = (const u32*)(ws + y.off_out + cb[k].out_off);
            }
            if (pos >= se) break;  // past the footer: zero padding
            const u64 avail = se - pos;
            const u32 take = (u32)(avail < (u64)(32 - got) ? avail : (u64)(32 - got));
            const u32 bits = bits_from(src, pos - ss, take);
            val = (take == 32) ? bits : ((val << take) | bits);
            got += take;
            pos += take;
        }
        if (got < 32) val <<= (32 - got);
        const u64 o = wd * 4;
        for (u32 q = 0; q < 4 && o + q < total; q++) dst[o + q] = (u8)(val >> (24 - 8 * q));
    }
    if (tid == 0) {
        out_len[c0 + c] = total;
        status[c0 + c] = ZCG_OK;
    }
}

}  // namespace

uint64_t bzip2_encode_ws_bytes(const zcg_array* a, uint32_t n) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    const i32 L = a->compression.bzip2_block_size;
    if (L < 1 || L > 9 || n == 0) return 0;
    return make_layout(D, (u32)L, n).total;
}

hipError_t launch_bzip2_encode(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, uint64_t* d_out_len,
                               int32_t* d_status, void* ws, uint64_t ws_bytes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    const i32 L = a->compression.bzip2_block_size;
    if (L < 1 || L > 9) return hipErrorInvalidValue;
    const BzeLayout y = make_layout(D, (u32)L, n);
    if (ws_bytes < y.total || y.tmax >= (1ull << 31)) return hipErrorInvalidValue;
    u8* w = (u8*)ws;
    hipError_t e;
    BzeCounters hc;
    for (u32 c0 = 0; c0 < n; c0 += y.m) {
        const u32 cnt = (n - c0) < y.m ? (n - c0) : y.m;
        hipLaunchKernelGGL(bze_rle1, dim3(cnt), dim3(64), 0, s, d_chunks, c0, cnt, D, t, y, w);
        hipLaunchKernelGGL(bze_layout, dim3(1), dim3(64), 0, s, cnt, y, w);
        hipLaunchKernelGGL(bze_compact, dim3(cnt), dim3(BZE_T), 0, s, cnt, y, w);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&hc, w + y.off_cnt, sizeof(hc), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        const u32 T = hc.T, NB = hc.NB;
        u8* text = w + y.off_text;
        u32* blkof = (u32*)(w + y.off_blkof);
        const BzeBlk* gb = (const BzeBlk*)(w + y.off_blk);
        u32* rank = (u32*)(w + y.off_rank);
        u32* sa = (u32*)(w + y.off_sa);
        u64* ka = (u64*)(w + y.off_ka);
        u64* kb = (u64*)(w + y.off_kb);
        u32* va = (u32*)(w + y.off_va);
        u32* vb = (u32*)(w + y.off_vb);
        u32* U = (u32*)(w + y.off_u);
        u32* sA = (u32*)(w + y.off_sa_scan);
        u32* sB = (u32*)(w + y.off_sb_scan);
        u8* flags = w + y.off_flags;
        void* cub = w + y.off_cub;
        u32* d_nsel = (u32*)(w + y.off_cnt) + 3;
        if (T > 0) {
            const u32 TB = 256;
            u32 nbits_blk = 0;
            while ((1u << nbits_blk) < NB) nbits_blk++;
            u32 rb = 1;
            while ((1ull << rb) < T) rb++;
            if (nbits_blk > 24) return hipErrorInvalidValue;
            const u32 dpre = (32 - nbits_blk) / 8 < 3 ? (32 - nbits_blk) / 8 : 3u;
            hipLaunchKernelGGL(bze_init_keys, dim3((T + TB - 1) / TB), dim3(TB), 0, s, T, text, blkof, gb, dpre,
                               (u32*)ka, va);
            size_t cb = y.cub_bytes;
            hipcub::DoubleBuffer<u32> dk((u32*)ka, (u32*)kb);
            hipcub::DoubleBuffer<u32> dv(va, vb);
            if ((e = hipcub::DeviceRadixSort::SortPairs(cub, cb, dk, dv, (int)T, 0, (int)(8 * dpre + nbits_blk), s)) !=
                hipSuccess)
                return e;
            hipLaunchKernelGGL(bze_heads<u32>, dim3((T + TB - 1) / TB), dim3(TB), 0, s, T, dk.Current(), 0u, sA);
            cb = y.cub_bytes;
            if ((e = hipcub::DeviceScan::InclusiveScan(cub, cb, sA, sB, MaxU32(), (int)T, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(bze_rank0, dim3((T + TB - 1) / TB), dim3(TB), 0, s, T, dk.Current(), dv.Current(), sB,
                               blkof, gb, dpre, rank, sa, flags);
            hipLaunchKernelGGL(bze_lds_sort, dim3((T + BZE_LC - 1) / BZE_LC), dim3(BZE_T), 0, s, T, text, blkof, gb, sB,
                               dpre, sa, rank, flags);
            cb = y.cub_bytes;
            if ((e = hipcub::DeviceSelect::Flagged(cub, cb, sa, flags, U, d_nsel, (int)T, s)) != hipSuccess)
                return e;
            u32 cntU = 0;
            if ((e = hipMemcpyAsync(&cntU, d_nsel, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            for (u32 h = dpre; cntU > 0; h *= 2) {
                const u32 G = (cntU + TB - 1) / TB;
                hipLaunchKernelGGL(bze_keys, dim3(G), dim3(TB), 0, s, cntU, h, rb, U, rank, blkof, gb, ka, va);
                hipcub::DoubleBuffer<u64> k2(ka, kb);
                hipcub::DoubleBuffer<u32> v2(va, vb);
                cb = y.cub_bytes;
                if ((e = hipcub::DeviceRadixSort::SortPairs(cub, cb, k2, v2, (int)cntU, 0, (int)(2 * rb), s)) !=
                    hipSuccess)
                    return e;
                hipLaunchKernelGGL(bze_heads<u64>, dim3(G), dim3(TB), 0, s, cntU, k2.Current(), rb, sA);
                cb = y.cub_bytes;
                if ((e = hipcub::DeviceScan::InclusiveScan(cub, cb, sA, sB, MaxU32(), (int)cntU, s)) != hipSuccess)
                    return e;
                hipLaunchKernelGGL(bze_sapos, dim3(G), dim3(TB), 0, s, cntU, rb, k2.Current(), v2.Current(), sB, sa,
                                   sA);
                cb = y.cub_bytes;
                if ((e = hipcub::DeviceScan::InclusiveScan(cub, cb, sA, sB, MaxU32(), (int)cntU, s)) != hipSuccess)
                    return e;
                const u32 h2 = (h >= 0x80000000u) ? 0xFFFFFFFFu : 2 * h;
                hipLaunchKernelGGL(bze_update, dim3(G), dim3(TB), 0, s, cntU, h2, rb, k2.Current(), v2.Current(), sB,
                                   blkof, gb, rank, flags);
                cb = y.cub_bytes;
                if ((e = hipcub::DeviceSelect::Flagged(cub, cb, v2.Current(), flags, U, d_nsel, (int)cntU, s)) !=
                    hipSuccess)
                    return e;
                if ((e = hipMemcpyAsync(&cntU, d_nsel, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
                if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
                if (h >= 0x80000000u) break;
            }
            hipLaunchKernelGGL(bze_block, dim3(NB), dim3(BZE_T), 0, s, NB, y, w);
        }
        hipLaunchKernelGGL(bze_assemble, dim3(cnt), dim3(BZE_T), 0, s, d_chunks, c0, cnt, y, w, d_out_len, d_status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace zcg
