// zcg_deflate.hip — gzip encoder (write_chunk for CompressionType::Gzip): the
// dispatcher, the zlib-exact coder and the CRC32 kernel.  gzip.rs:50-56 writes
// flate2's GzEncoder at the effective level: a 10-byte header (XFL 2 at level
// >= 9, 4 at level <= 1), zlib raw deflate, then CRC32 and ISIZE.
//   * launch_deflate: levels 1-9 take the zlib-exact coder; level 0 and
//     ZCG_FLAG_GZIP_SEGMENTED the segmented coder (zcg_deflate_seg.hip), whose
//     streams only inflate to the chunk.
//   * The zlib-exact coder (dz_*).  zcg_zlib_core.h restates zlib's deflate_slow
//     (levels 4-9) and deflate_fast (1-3) as (1) a per-position match search,
//     (2) a short sequential parse and (3) per-block trees.  (1) runs over every
//     position: dz_keys, the shared sort (zcg_chains.h), dz_best; (2) one wave
//     per chunk, wave-uniform: dz_parse / dz_parse_fast; (3) one wave per block:
//     dz_plan, then dz_offsets / dz_emit / dz_final place the blocks' bits at
//     their prefix-summed offsets.  The bytes are zlib's (tests/test_hostcore.py
//     pins the core on the CPU, tests/test_gpu_encode.py the kernels).
//   * gzip_crc32: per chunk, 64 lanes CRC their slices, lane 0 combines them
//     with a precomputed GF(2) shift operator; both coders' trailers.
//   * The zlib codec (ZCG_CODEC_ZLIB) is the same two coders inside RFC 1950's
//     container: a 2-byte header, and zlib_adler32 in gzip_crc32's place.  At
//     levels 1-9 the bytes are zlib.compress(data, level)'s.
#include "zcg_chains.h"
#include "zcg_deflate.h"
#include "zcg_zlib_core.h"
#include "zcg_adler.h"

namespace zcg {

// GF(2) operator (32 columns) applied to a CRC: M * v.
__device__ __forceinline__ u32 gf2_times(const u32* M, u32 v) {
    u32 s = 0;
    for (u32 i = 0; v; i++, v >>= 1)
        if (v & 1) s ^= M[i];
    return s;
}

struct CrcShift { u32 m[32]; };

// 64 lanes per chunk: lane l CRCs slice l (the remainder goes to slice 0), then
// lane 0 folds them with the operator that advances a register over Lsl bytes.
// With crc_out set, only the CRC of each chunk's input is stored there (for
// the trailer dz_final writes; status and out_len are not read).
__global__ __launch_bounds__(64) void gzip_crc32(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                 u64 Lsl, CrcShift op, const u64* __restrict__ out_len,
                                                 const i32* __restrict__ status, DType t, u32* __restrict__ crc_out) {
    const u32 c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    if (crc_out ? chunks[c].src_len < D : status[c] != ZCG_OK) return;
    const u8* src = (const u8*)chunks[c].src;
    const u64 rem = D - 64 * Lsl;  // slice 0 length = Lsl + rem
    const u64 a = lane == 0 ? 0 : rem + lane * Lsl;
    const u64 b = rem + (lane + 1) * Lsl;
    // raw CRC registers: slice 0 starts from 0xFFFFFFFF, the others from 0, so
    // R(A||B) = shift_len(B)(R(A)) ^ R0(B) folds them (zlib crc32_combine)
    u32 crc = lane == 0 ? 0xFFFFFFFFu : 0u;
    u64 p = a;
    for (; p < b && (p & 15); p++) crc = g_crc32_table[(crc ^ norm_byte(src[swap_pos(p, t)], t)) & 0xFF] ^ (crc >> 8);
    for (; p + 16 <= b; p += 16) {
        const u32x4 v = transform16(ld16(src + p), t);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            u32 x = w[j];
#pragma unroll
            for (u32 q = 0; q < 4; q++) { crc = g_crc32_table[(crc ^ x) & 0xFF] ^ (crc >> 8); x >>= 8; }
        }
    }
    for (; p < b; p++) crc = g_crc32_table[(crc ^ norm_byte(src[swap_pos(p, t)], t)) & 0xFF] ^ (crc >> 8);
    __shared__ u32 s_crc[64];
    s_crc[lane] = crc;
    __syncthreads();
    if (lane != 0) return;
    u32 r = s_crc[0];
    for (u32 l = 1; l < 64; l++) r = gf2_times(op.m, r) ^ s_crc[l];
    r ^= 0xFFFFFFFFu;
    if (crc_out) {
        crc_out[c] = r;
        return;
    }
    u8* o = (u8*)chunks[c].dst + out_len[c] - 8;
    o[0] = (u8)r; o[1] = (u8)(r >> 8); o[2] = (u8)(r >> 16); o[3] = (u8)(r >> 24);
    const u32 isz = (u32)D;
    o[4] = (u8)isz; o[5] = (u8)(isz >> 8); o[6] = (u8)(isz >> 16); o[7] = (u8)(isz >> 24);
}

// Host: operator that advances a raw CRC register over `len` zero bytes
// (zlib crc32_combine's gf2 matrix powers).
static void gf2_square(u32* sq, const u32* m) {
    for (int i = 0; i < 32; i++) {
        u32 v = m[i], s = 0;
        for (int j = 0; v; j++, v >>= 1)
            if (v & 1) s ^= m[j];
        sq[i] = s;
    }
}
static void crc_shift_op(u64 len, u32* out) {
    u32 odd[32], even[32], res[32];
    odd[0] = 0xEDB88320u;  // one zero bit
    for (int i = 1; i < 32; i++) odd[i] = 1u << (i - 1);
    gf2_square(even, odd);  // 2 bits
    gf2_square(odd, even);  // 4 bits
    for (int i = 0; i < 32; i++) res[i] = 1u << i;  // identity
    // res = op^(8*len): square up through bits of len (each step: 8 bits * 2^k)
    u32 cur[32];
    gf2_square(cur, odd);  // 8 bits = one byte
    while (len) {
        if (len & 1) {
            u32 t[32];
            for (int i = 0; i < 32; i++) {
                u32 v = res[i], s = 0;
                for (int j = 0; v; j++, v >>= 1)
                    if (v & 1) s ^= cur[j];
                t[i] = s;
            }
            for (int i = 0; i < 32; i++) res[i] = t[i];
        }
        len >>= 1;
        if (len) {
            u32 t[32];
            gf2_square(t, cur);
            for (int i = 0; i < 32; i++) cur[i] = t[i];
        }
    }
    for (int i = 0; i < 32; i++) out[i] = res[i];
}

hipError_t launch_gzip_crc32(const zcg_chunk* d_chunks, u32 n, u64 D, DType t, const u64* d_out_len,
                             const i32* d_status, u32* crc_out, hipStream_t s) {
    const u64 Lsl = D / 64;
    CrcShift op;
    crc_shift_op(Lsl, op.m);
    hipLaunchKernelGGL(gzip_crc32, dim3(n), dim3(64), 0, s, d_chunks, n, D, Lsl, op, d_out_len, d_status, t, crc_out);
    return hipGetLastError();
}

// The zlib codec's trailer: gzip_crc32's two modes with Adler-32 (zcg_adler.h)
// of the serialised input.  One workgroup per chunk; thread i takes the 16
// bytes at i * 16 of every 4 KiB tile (coalesced), a short last tile is padded
// with zero pieces; the lanes' partials add.  sum_out set: the value only (the
// slot dz_final reads); else 4 big-endian bytes at the end of the stream.
constexpr u32 ZA_NT = 256;
static_assert((1ull << 31) / (ZA_NT * 16) <= ADLER_LANE_MAX_PIECES,
              "a lane's pieces of the largest chunk (D < 2^31) stay inside the deferred-modulo bound");
__global__ __launch_bounds__(ZA_NT) void zlib_adler32(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                      const u64* __restrict__ out_len, const i32* __restrict__ status,
                                                      DType t, u32* __restrict__ sum_out) {
    const u32 c = blockIdx.x, tid = threadIdx.x;
    if (c >= n) return;
    if (sum_out ? chunks[c].src_len < D : status[c] != ZCG_OK) return;
    const u8* src = (const u8*)chunks[c].src;
    constexpr u64 TILE = ZA_NT * 16;
    const u64 ntile = (D + TILE - 1) / TILE;
    AdlerLane al = adler_lane_open();
    for (u64 k = 0; k < ntile; k++) {
        const u64 p = k * TILE + tid * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (p + 16 <= D) {
            v = transform16(ld16(src + p), t);
        } else if (p < D) {  // the piece the chunk ends in (whole elements: D % es == 0)
            u32 w[4] = {0u, 0u, 0u, 0u};
            for (u64 q = p; q < D; q++) w[(q - p) >> 2] |= ser1(src, q, t) << (8 * ((q - p) & 3));
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        adler_lane_piece(al, v.x, v.y, v.z, v.w);
    }
    u32 v = 0;
    if (ntile) v = adler_lane_close(al, (i64)D - (i64)((ntile - 1) * TILE + tid * 16) - 16, (u32)TILE);
    v = adler_wave_sum(v);
    __shared__ u32 s_part[ZA_NT / 64];
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
    if (tid != 0) return;
    u32 r = 0;
    for (u32 i = 0; i < ZA_NT / 64; i++) r = adler_add(r, s_part[i]);
    r = adler_finish(r, D);
    if (sum_out) {
        sum_out[c] = r;
        return;
    }
    u8* o = (u8*)chunks[c].dst + out_len[c] - 4;
    o[0] = (u8)(r >> 24); o[1] = (u8)(r >> 16); o[2] = (u8)(r >> 8); o[3] = (u8)r;
}

hipError_t launch_zlib_adler32(const zcg_chunk* d_chunks, u32 n, u64 D, DType t, const u64* d_out_len,
                               const i32* d_status, u32* sum_out, hipStream_t s) {
    hipLaunchKernelGGL(zlib_adler32, dim3(n), dim3(ZA_NT), 0, s, d_chunks, n, D, d_out_len, d_status, t, sum_out);
    return hipGetLastError();
}

// The container of a deflate stream: zhdr == 0 the gzip member (10-byte header
// with XFL, CRC32 + ISIZE), else the zlib stream whose two header bytes are
// zhdr (big-endian) and whose trailer is the Adler-32.  zlib 1.2.11's
// deflate(): CMF 0x78, FLG's level bits from the level, FCHECK makes it a
// multiple of 31.
u32 zlib_header_word(const zcg_array* a, u32 level) {
    if (a->compression.codec != ZCG_CODEC_ZLIB) return 0u;
    return level <= 1 ? 0x7801u : level <= 5 ? 0x785Eu : level == 6 ? 0x789Cu : 0x78DAu;
}
hipError_t launch_stream_checksum(u32 zhdr, const zcg_chunk* d_chunks, u32 n, u64 D, DType t, const u64* d_out_len,
                                  const i32* d_status, u32* sum_out, hipStream_t s) {
    return zhdr ? launch_zlib_adler32(d_chunks, n, D, t, d_out_len, d_status, sum_out, s)
                : launch_gzip_crc32(d_chunks, n, D, t, d_out_len, d_status, sum_out, s);
}

// ---- the zlib-exact coder ----
namespace {

constexpr u64 DZ_SUPER_BYTES = 512ull << 20;  // input bytes per super-batch (match results kept for all)
#ifndef ZDZ_SUB_MIB
#define ZDZ_SUB_MIB 128  // (256: 125.7 vs 125.6-126.0 ms per C5 call; 512: 130.4)
#endif
constexpr u64 DZ_SUB_BYTES = (u64)ZDZ_SUB_MIB << 20;  // input bytes per match-search sub-batch (zlib-exact coder)
constexpr u32 DZ_TAILCAP = 2048;               // symbols a segment's parse may run past its end before syncing
constexpr u32 DZ_HDRW = 96;                 // header bit-string words per block (<= 14 + 57 + 316 * 14 bits)

struct DzBlock {     // one flushed block (zz::BlockRec) + its plan
    u32 s0, s1, b0, b1;
    u32 in_win, last, type, hbits;
    u32 dbits, pad;
    u64 bitoff;      // bit offset in the chunk's deflate stream
    u32 lcode[zz::L_CODES];  // code | len << 16 (dynamic)
    u32 dcode[zz::D_CODES];
    u32 hdr[DZ_HDRW];        // the block-type bits and (dynamic) send_all_trees, LSB first
};

struct DzChunk {
    u32 nblocks, status;
    u64 bytes;       // deflate stream bytes
    u64 fsym, fpos;  // the final symbol stream and its positions (u32 offsets from the workspace base)
    u32 nsym, nloop;
};

struct DzWs {
    SubBatch b;  // (m <= 65536: chunk id + 16 key bits fit 32)
    u32 nbmax;
    ChainWs c;  // (no links: dz_best searches the sorted run)
    u64 outcap, off_m2, off_sym, off_pos, off_bm, off_tail, off_ch, off_blk, off_out, off_crc, total;
};

DzWs dz_ws(u64 D, u32 n) {
    DzWs y{};
    y.b = sub_batch_plan(D, n, DZ_SUB_BYTES, DZ_SUPER_BYTES, 65536);
    const u64 sb = y.b.sm;
    y.nbmax = (u32)((D + zz::BLOCK_SYMS - 1) / zz::BLOCK_SYMS + 1);
    y.outcap = (D + D / 8 + 4096 + 255) & ~255ull;
    WsCarve ws;
    y.c = carve_chain_ws(ws, y.b.tot, false);
    y.off_m2 = ws.take(8 * sb * D + 4096);   // match results; then the final symbols + positions
    y.off_sym = ws.take(4 * sb * D + 4096);  // per-segment symbols (pass 1)
    y.off_pos = ws.take(4 * sb * D + 4096);  // their positions
    y.off_bm = ws.take(4 * sb * (D / 32 + 2));
    y.off_tail = ws.take(8ull * 64 * DZ_TAILCAP * sb);
    y.off_ch = ws.take(sizeof(DzChunk) * sb);
    y.off_blk = ws.take(sizeof(DzBlock) * sb * y.nbmax);
    y.off_out = ws.take(y.outcap * sb);
    y.off_crc = ws.take(4ull * sb);  // the super-batch's input CRC32s or Adler-32s (dz_final writes the trailers)
    y.total = ws.total();
    return y;
}

// keys: chunk id << 16 | zlib's 15-bit hash of the serialised bytes p..p+2
// (positions past D-3 are never inserted: a group of their own).  (Hash-only
// keys sort in two radix passes instead of three and a stable sort still
// leaves each (hash, chunk) chain contiguous, but the chunks' runs then
// interleave: dz_best lost locality, 24.4 vs 23.2 ms per 128 C5 chunks, more
// than the pass saved.)
__global__ void dz_keys(const zcg_chunk* __restrict__ chunks, u32 c0, u64 D, u64 tot, DType t,
                        u32* __restrict__ keys, u32* __restrict__ vals) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tot) return;
    const u32 cl = (u32)(g / D);
    const u64 p = g - (u64)cl * D;
    const zcg_chunk ch = chunks[c0 + cl];
    u32 h = 0x8000u;
    if (p + 3 <= D && ch.src_len >= D) {
        const u8* src = (const u8*)ch.src;
        h = zz::hash3(ser1(src, p, t), ser1(src, p + 1, t), ser1(src, p + 2, t));
    }
    keys[g] = (cl << 16) | h;
    vals[g] = (u32)g;
}

// zz::search (zcg_zlib_core.h, the host reference) for native-order bytes and
// p + 32 <= D, over the sorted run: the chain of p = entry j is entries j-1,
// j-2, ... while the key is kj.  p's first 32 bytes stay in registers; the
// candidates come 4 at a time (their keys and positions by two 16-byte loads,
// then their first 16 bytes by four loads in flight together), and are then
// compared in chain order, so a thread waits two memory latencies per four
// candidates instead of one or two per candidate.  Same candidates, order,
// ties (the first candidate reaching a longer match), NIL and window rules,
// nice cut and reduced-budget snapshot as zz::search; its scan_end test only
// skips candidates that cannot beat `best`, so leaving it out changes no result.
__device__ zz::Match2 dz_search_run(u32 p, u32 D, const zz::Config& cfg, const u8* src, const u32* __restrict__ keys,
                                    const u32* __restrict__ vals, u64 j, u32 kj, u32 cbase) {
    zz::Match2 r{0u, 0u};
    const gu8* g = (const gu8*)src;
    typedef __attribute__((address_space(1))) u32x4 gu32x4_a4 __attribute__((aligned(4)));
    auto b4 = [&](u32 i) -> u32 { return *(const gu32_ua*)(g + i); };
    auto pre16 = [](u32x4 A, u32x4 B) -> u32 {
        const u32 x0 = A.x ^ B.x, x1 = A.y ^ B.y, x2 = A.z ^ B.z, x3 = A.w ^ B.w;
        if (x0) return (u32)__builtin_ctz(x0) >> 3;
        if (x1) return 4 + ((u32)__builtin_ctz(x1) >> 3);
        if (x2) return 8 + ((u32)__builtin_ctz(x2) >> 3);
        if (x3) return 12 + ((u32)__builtin_ctz(x3) >> 3);
        return 16u;
    };
    const u32 look = D - p;
    const u32 mx = look < zz::MAX_MATCH ? look : zz::MAX_MATCH;  // >= 32
    const u32 nice = cfg.nice < look ? cfg.nice : look;
    const u32 lim = p > zz::MAX_DIST ? p - zz::MAX_DIST : 0u;
    const u32 nred = cfg.chain >> 2;
    const u32x4 P0 = *(const gu32x4_ua*)(g + p), P1 = *(const gu32x4_ua*)(g + p + 16);
    u32 best = 0, bstart = 0, k = 0;
    bool red_done = false;
    // entries jj-4 .. jj-1 per block (jj >= 4 here: a shorter rest reads the
    // entries before the array start from index 0 and marks them invalid)
    for (u64 jj = j; k < cfg.chain; jj -= 4) {
        const u64 b = jj >= 4 ? jj - 4 : 0;
        const u32x4 K = *(const gu32x4_a4*)(keys + b), V = *(const gu32x4_a4*)(vals + b);
        // candidate i (chain order) = entry jj-1-i = component 3-i of the block (when jj >= 4)
        u32 cc[4];
        bool ok[4];
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            const u64 e = jj - 1 - i;  // (wraps when jj <= i: invalid)
            const u32 lane4 = (u32)(e - b);
            const u32 kv = lane4 == 0 ? K.x : lane4 == 1 ? K.y : lane4 == 2 ? K.z : K.w;
            const u32 vv = lane4 == 0 ? V.x : lane4 == 1 ? V.y : lane4 == 2 ? V.z : V.w;
            ok[i] = jj > i && kv == kj;
            cc[i] = vv - cbase;
        }
        u32x4 C[4];
#pragma unroll
        for (u32 i = 0; i < 4; i++) C[i] = *(const gu32x4_ua*)(g + (ok[i] && cc[i] < p ? cc[i] : p));
        bool stop = false;
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            const u32 c = cc[i];
            if (k == 0) {
                // hash_head != NIL && strstart - hash_head <= MAX_DIST; the
                // window-relative head at the slid window's base reads as NIL
                if (!ok[i] || c == zz::slides_at(p, D) * zz::WSIZE || p - c > zz::MAX_DIST) return r;
            } else if (!ok[i] || c <= lim) {
                stop = true;
                break;
            }
            u32 len = pre16(P0, C[i]);
            if (len == 16) {
                const u32x4 C1 = *(const gu32x4_ua*)(g + c + 16);
                len += pre16(P1, C1);
                if (len == 32) {
                    while (len + 4 <= mx) {
                        const u32 x = b4(p + len) ^ b4(c + len);
                        if (x) {
                            len += (u32)__builtin_ctz(x) >> 3;
                            goto done;
                        }
                        len += 4;
                    }
                    while (len < mx && g[p + len] == g[c + len]) len++;
                }
            }
        done:
            if (len > best) {
                best = len;
                bstart = c;
                if (best >= nice) {
                    stop = true;
                    break;
                }
            }
            if (k + 1 == nred) {
                r.red = best ? (best | ((p - bstart) << 9)) : 0u;
                red_done = true;
            }
            if (++k == cfg.chain) {
                stop = true;
                break;
            }
        }
        if (stop) break;
    }
    r.full = best ? (best | ((p - bstart) << 9)) : 0u;
    if (!red_done) r.red = r.full;
    return r;
}

// zz::search at every position of the sub-batch: m2[g] = {full, red}, one
// thread per position in the ORDER OF THE SORTED KEYS.  The stable sort of
// (chunk, hash) with ascending positions lays every hash chain out
// contiguously: position vals[j]'s chain is vals[j-1], vals[j-2], ... while
// the key stays the same -- exactly zlib's prev[] walk -- so a candidate is a
// coalesced load at a known index instead of a dependent load of prev[c] at
// a random address, and neighbouring threads walk overlapping candidate
// lists (their byte loads hit the same lines).  The result is scattered back
// to m2[vals[j]].
// (An LDS-staged variant of the prev[] walk -- each workgroup's 40 KB search
// window of bytes and u16 chain links in LDS -- measured slower: 48.9 vs
// 45.2 ms per 128 C5 chunks.)
__global__ void dz_best(const zcg_chunk* __restrict__ chunks, u32 c0, u64 D, u64 tot, DType t, zz::Config cfg,
                        const u32* __restrict__ keys, const u32* __restrict__ vals, uint2* __restrict__ m2) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= tot) return;
    const u32 kj = keys[j];
    const u32 g = vals[j];
    const u32 cl = (u32)(g / D);
    const u32 p = (u32)(g - (u64)cl * D);
    zz::Match2 r{0u, 0u};
    const zcg_chunk ch = chunks[c0 + cl];
    if (ch.src_len >= D && (kj & 0x8000u) == 0) {
        const u8* src = (const u8*)ch.src;
        const u32 cbase = (u32)((u64)cl * D);
        auto b1 = [&](u32 i) -> u32 { return ser1(src, i, t); };
        auto b4 = [&](u32 i) -> u32 { return ser4(src, i, t); };
        // zz::search asks for the chain in order (the head p, then each
        // candidate once): the next entry of the sorted run, NONE past it
        u64 jj = j;
        auto pv = [&](u32) -> u32 {
            if (jj == 0 || keys[jj - 1] != kj) {
                jj = 0;
                return zz::NONE;
            }
            jj--;
            return vals[jj] - cbase;
        };
        if (!t.swap && !t.isbool && (u64)p + 32 <= D) r = dz_search_run(p, (u32)D, cfg, src, keys, vals, j, kj, cbase);
        else r = zz::search(p, (u32)D, cfg, b4, b1, pv);
    }
    m2[g] = make_uint2(r.full, r.red);
}

// The lazy parse of one chunk, SEGMENT-PARALLEL: lane k parses positions
// [k seg, (k+1) seg) from a canonical state (zz::PState: prev_len 2, not
// pending -- the state after any match), marking the positions of its
// canonical loop tops in a bitmap (pass 1).  Then each lane continues its
// parse past its segment until it reaches a canonical loop top that a later
// segment's parse also reached (pass 2): from there the two agree, so the
// true parse is lane 0's path, its tail, the next segment's path from the
// sync symbol, and so on (stitched into one stream).  A tail that does not
// sync within DZ_TAILCAP symbols sends the chunk to a serial parse.  The
// stitched stream and block records equal deflate_slow's
// (tests/hostcore/zlib_ref.cpp zz_host_deflate_seg restates this exactly).
// The match results come from dz_best (every position searched first:
// searching on demand at the loop tops the parses visit, ~40 % of the
// positions, measured 5 347 vs 217 ms per C5 call -- each lane's searches
// are a serial chain of dependent loads).
__global__ __launch_bounds__(64) void dz_parse(const zcg_chunk* __restrict__ chunks, u32 c0, u32 nc, u64 D, DType t,
                                              zz::Config cfg, u32* __restrict__ wbase, u64 off_m2, u64 off_sym,
                                              u64 off_pos, u64 off_bm, u64 off_tail, DzChunk* __restrict__ cst,
                                              DzBlock* __restrict__ blks, u32 nbmax, u32 cb) {
    const u32 cl = blockIdx.x;  // chunk of this launch (chunks[c0 + cl]; its records at cb + cl)
    if (cl >= nc) return;
    const u32 c = cb + cl;
    const u32 lane = threadIdx.x;
    const zcg_chunk ch = chunks[c0 + cl];
    DzChunk* cs = cst + c;
    if (ch.src_len < D) {
        if (lane == 0) { cs->nblocks = 0; cs->status = ZCG_ERR_INVALID_DATA; }
        return;
    }
    const u8* src = (const u8*)ch.src;
    const u32 D32 = (u32)D;
    const uint2* mc = (const uint2*)(wbase + off_m2) + (u64)c * D;  // match results (8 B / position)
    u32* fsy = wbase + off_m2 + (u64)c * 2 * D;                      // final stream (reuses them)
    u32* fps = fsy + D;
    u32* psy = wbase + off_sym + (u64)c * D;                         // pass-1 symbols / positions
    u32* pps = wbase + off_pos + (u64)c * D;
    u32* bm = wbase + off_bm + (u64)c * (D / 32 + 2);
    u32* tsy = wbase + off_tail + (u64)c * 2 * 64 * DZ_TAILCAP + (u64)lane * 2 * DZ_TAILCAP;
    u32* tps = tsy + DZ_TAILCAP;
    const u32 seg = D32 ? (((D32 + 63) / 64 + 31) & ~31u) : 32u;
    const u32 nseg = D32 ? (D32 + seg - 1) / seg : 1u;
    const bool act = lane < nseg;
    const u32 S0 = lane * seg, S1 = (lane + 1 == nseg) ? D32 : (lane + 1) * seg;
    auto b4 = [&](u32 i) -> u32 { return ser4(src, i, t); };
    auto byte = [&](u32 i) -> u32 { return ser1(src, i, t); };
    auto get = [&](u32 p) -> zz::Match2 {
        const uint2 v = mc[p];
        return zz::Match2{v.x, v.y};
    };
    // ---- pass 1 ----
    zz::PState st = zz::fresh_state(S0);
    u32 n1 = 0, fin1 = 0;
    if (act) {
        for (u32 w = S0 / 32; w < (S1 + 31) / 32; w++) bm[w] = 0;
        u32 cwi = S0 / 32, cwv = 0;
        auto em = [&](u32 sym, u32 at) {
            psy[S0 + n1] = sym;
            pps[S0 + n1] = at;
            n1++;
        };
        while (st.p < S1) {
            if (zz::canonical(st)) {
                const u32 wi = st.p >> 5;
                if (wi != cwi) {
                    if (cwv) bm[cwi] = cwv;
                    cwi = wi;
                    cwv = 0;
                }
                cwv |= 1u << (st.p & 31);
            }
            zz::step(st, D32, cfg, get, byte, em);
        }
        if (cwv) bm[cwi] = cwv;
        if (lane + 1 == nseg && st.avail) {  // Z_FINISH: the pending literal
            em(byte(st.p - 1), st.p - 1);
            st.avail = 0;
            fin1 = 1;
        }
    }
    __syncthreads();  // every segment's bitmap is in place
    // ---- pass 2 ----
    u32 nt = 0, syncq = 0xFFFFFFFFu, tfin = 0, ovf = 0;
    if (act && lane + 1 < nseg) {
        auto em = [&](u32 sym, u32 at) {
            tsy[nt] = sym;
            tps[nt] = at;
            nt++;
        };
        while (true) {
            if (st.p >= D32) {
                if (st.avail) {
                    em(byte(st.p - 1), st.p - 1);
                    tfin = 1;
                }
                break;
            }
            if (st.p >= S1 && zz::canonical(st) && ((bm[st.p >> 5] >> (st.p & 31)) & 1u)) {
                syncq = st.p;
                break;
            }
            if (nt + 1 >= DZ_TAILCAP) {
                ovf = 1;
                break;
            }
            zz::step(st, D32, cfg, get, byte, em);
        }
    }
    __syncthreads();  // tails written
    const bool any_ovf = __ballot(ovf != 0) != 0;
    u32 nsym = 0, finlit = 0;
    u64 fsel_sy = (u64)(fsy - wbase), fsel_ps = (u64)(fps - wbase);
    if (!any_ovf) {
        // ---- stitch (wave-uniform chain walk, cooperative copies) ----
        // (8 pieces per lane in flight: a copy waits one load latency per 512 symbols)
        auto copy = [&](const u32* ssy, const u32* sps, u32 n) {
            u32 i = lane;
            for (; i + 7 * 64 < n; i += 8 * 64) {
                u32 a[8], b[8];
#pragma unroll
                for (u32 k = 0; k < 8; k++) {
                    a[k] = ssy[i + 64 * k];
                    b[k] = sps[i + 64 * k];
                }
#pragma unroll
                for (u32 k = 0; k < 8; k++) {
                    fsy[nsym + i + 64 * k] = a[k];
                    fps[nsym + i + 64 * k] = b[k];
                }
            }
            for (; i < n; i += 64) {
                fsy[nsym + i] = ssy[i];
                fps[nsym + i] = sps[i];
            }
            nsym += n;
        };
        u32 cur = 0, idx = 0;
        while (true) {
            const u32 cS0 = cur * seg;
            const u32 cn1 = (u32)__builtin_amdgcn_readlane((int)n1, (int)cur);
            copy(psy + cS0 + idx, pps + cS0 + idx, cn1 - idx);
            if (cur + 1 == nseg) {
                finlit = (u32)__builtin_amdgcn_readlane((int)fin1, (int)cur);
                break;
            }
            const u32 cnt = (u32)__builtin_amdgcn_readlane((int)nt, (int)cur);
            const u32* csy = wbase + off_tail + (u64)c * 2 * 64 * DZ_TAILCAP + (u64)cur * 2 * DZ_TAILCAP;
            copy(csy, csy + DZ_TAILCAP, cnt);
            const u32 q = (u32)__builtin_amdgcn_readlane((int)syncq, (int)cur);
            if (q == 0xFFFFFFFFu) {
                finlit = (u32)__builtin_amdgcn_readlane((int)tfin, (int)cur);
                break;
            }
            const u32 nx = q / seg;
            const u32 xS0 = nx * seg;
            const u32 xn1 = (u32)__builtin_amdgcn_readlane((int)n1, (int)nx);
            // the first symbol of segment nx at or after q (there is one: q is
            // one of its canonical loop tops)
            u32 j = 0;
            for (u32 j0 = 0; j0 < xn1; j0 += 64) {
                const u32 jj = j0 + lane;
                const u64 m = __ballot(jj < xn1 && pps[xS0 + jj] >= q);
                if (m) {
                    j = j0 + (u32)__builtin_ctzll(m);
                    break;
                }
                j = xn1;
            }
            cur = nx;
            idx = j;
        }
    } else {
        // ---- a tail did not sync: the serial parse into the pass-1 arrays ----
        __syncthreads();
        fsel_sy = (u64)(psy - wbase);
        fsel_ps = (u64)(pps - wbase);
        zz::PState s2 = zz::fresh_state(0);
        u32 k = 0;
        auto em = [&](u32 sym, u32 at) {
            if (lane == 0) {
                psy[k] = sym;
                pps[k] = at;
            }
            k++;
        };
        auto gu = [&](u32 p) -> zz::Match2 {
            const zz::Match2 v = get(p);
            return zz::Match2{(u32)__builtin_amdgcn_readfirstlane(v.full), (u32)__builtin_amdgcn_readfirstlane(v.red)};
        };
        auto bu = [&](u32 i) -> u32 { return (u32)__builtin_amdgcn_readfirstlane(ser1(src, i, t)); };
        while (s2.p < D32) zz::step(s2, D32, cfg, gu, bu, em);
        if (s2.avail) {
            em(bu(s2.p - 1), s2.p - 1);
            finlit = 1;
        }
        nsym = k;
    }
    __syncthreads();  // the final stream is in place
    const u32* Fs = wbase + fsel_sy;
    const u32* Fp = wbase + fsel_ps;
    const u32 nloop = nsym - finlit;
    const u32 nb = zz::num_blocks(nloop);
    auto P = [&](u32 i) -> u32 { return Fp[i]; };
    auto Y = [&](u32 i) -> u32 { return Fs[i]; };
    for (u32 k = lane; k < nb && k < nbmax; k += 64) {
        const zz::BlockRec r = zz::block_rec(k, nsym, nloop, D32, P, Y);
        DzBlock* o = blks + (u64)c * nbmax + k;
        o->s0 = r.s0; o->s1 = r.s1; o->b0 = r.b0; o->b1 = r.b1; o->in_win = r.in_win; o->last = r.last;
    }
    if (lane == 0) {
        cs->fsym = fsel_sy;
        cs->fpos = fsel_ps;
        cs->nsym = nsym;
        cs->nloop = nloop;
        cs->nblocks = nb <= nbmax ? nb : 0u;
        cs->status = nb <= nbmax ? ZCG_OK : ZCG_ERR_INVALID_DATA;
    }
}

// deflate_fast (levels 1-3): zlib's greedy parse builds its hash chains as
// it goes (positions inside a match longer than max_insert_length are never
// inserted), so the parse is serial per chunk: one wave per chunk runs
// zz::parse_fast's rules with zlib's head[] / prev[] as window-relative u16
// Pos in LDS (64 KiB each, slid like slide_hash), the next 512 input bytes
// in two registers per lane, and each chain candidate's match length from
// one 4-byte compare per lane (a ballot finds the first difference).
// Symbols leave 64 at a time in the same final-stream layout as dz_parse;
// block records come from zz::block_rec(..., fast = true), so the plan /
// emit kernels are shared.  tests/hostcore/zlib_ref.cpp (zz::parse_fast on
// the CPU) and the GPU output are compared with zlib byte for byte.
constexpr u32 DZF_LDS = 2 * 32768 * 2;  // head[] + prev[], u16 each
// RING: the last 32 KiB of input (positions (p + 262 - 32768, p + 262],
// which covers every candidate within MAX_DIST and its 258 bytes) also live
// in LDS, so a chain candidate's compare is two LDS reads per side instead
// of a global-memory round trip; 160 KiB, the whole CU's LDS
constexpr u32 DZF_RING = 32768;
constexpr u32 DZF_LDS_RING = DZF_LDS + DZF_RING;
__device__ __forceinline__ u32 dzf_ld4(const u8* src, u32 x, u32 D, const DType& t) {  // bytes past D read 0
    if (x + 4 <= D) return ser4(src, x, t);
    u32 v = 0;
    for (u32 k = 0; k < 4; k++)
        if (x + k < D) v |= ser1(src, x + k, t) << (8 * k);
    return v;
}
__global__ __launch_bounds__(64) void dz_parse_fast(const zcg_chunk* __restrict__ chunks, u32 c0, u32 nc, u64 D,
                                                   DType t, zz::Config cfg, u32* __restrict__ wbase, u64 off_m2,
                                                   DzChunk* __restrict__ cst, DzBlock* __restrict__ blks, u32 nbmax) {
    extern __shared__ __attribute__((aligned(16))) u8 smem_raw[];
    u16* hd = (u16*)smem_raw;
    u16* pv = hd + 32768;
    u8* ring = smem_raw + DZF_LDS;  // byte q at ring[q & (DZF_RING - 1)]
    const u32 c = blockIdx.x;
    if (c >= nc) return;
    const u32 lane = threadIdx.x;
    const zcg_chunk ch = chunks[c0 + c];
    DzChunk* cs = cst + c;
    if (ch.src_len < D) {
        if (lane == 0) { cs->nblocks = 0; cs->status = ZCG_ERR_INVALID_DATA; }
        return;
    }
    const u8* src = (const u8*)ch.src;
    const u32 D32 = (u32)D;
    u32* fsy = wbase + off_m2 + (u64)c * 2 * D;  // final stream: symbols, then positions
    u32* fps = fsy + D;
    for (u32 i = lane; i < 32768; i += 64) ((u32*)smem_raw)[i] = 0u;  // both tables NIL
    __syncthreads();
    auto rd = [&](const u16* a, u32 i) -> u32 { return (u32)__builtin_amdgcn_readfirstlane((u32)a[i]); };
    // input window: lane l holds bytes [wb + 4 l, +4) (w0) and [wb + 256 + 4 l, +4) (w1)
    u32 wb = 0;
    u32 w0 = dzf_ld4(src, 4 * lane, D32, t), w1 = dzf_ld4(src, 256 + 4 * lane, D32, t);
    auto wbyte = [&](u32 q) -> u32 {  // q in [wb, wb + 512)
        const u32 o = q - wb, wi = o >> 2;
        const u32 v = (u32)__builtin_amdgcn_readlane((int)(wi < 64 ? w0 : w1), (int)(wi & 63));
        return (v >> (8 * (o & 3))) & 0xFFu;
    };
    u32 base = 0, nsym = 0, rs = 0, rp = 0;
    auto emit = [&](u32 sym, u32 at) {
        const u32 k = nsym & 63;
        if (lane == k) { rs = sym; rp = at; }
        nsym++;
        if (k == 63) {
            fsy[nsym - 64 + lane] = rs;
            fps[nsym - 64 + lane] = rp;
        }
    };
    auto insert = [&](u32 q) -> u32 {  // INSERT_STRING: the previous head (relative, 0 = NIL)
        const u32 h = zz::hash3(wbyte(q), wbyte(q + 1), wbyte(q + 2));
        const u32 hh = rd(hd, h);
        if (lane == 0) {
            pv[(q - base) & zz::WMASK] = (u16)hh;
            hd[h] = (u16)(q - base);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        return hh;
    };
    // bytes [rf, F) into the ring from the register window, 64 per round
    u32 rf = 0;
    auto ring_fill = [&](u32 F) {
        for (u32 q0 = rf; q0 < F; q0 += 64) {
            const u32 q = q0 + lane;
            const u32 o = q - wb, wi = o >> 2;
            const u32 a0 = __shfl(w0, (int)(wi & 63)), a1 = __shfl(w1, (int)(wi & 63));
            const u32 v = ((wi < 64 ? a0 : a1) >> (8 * (o & 3))) & 0xFFu;
            if (q < F) ring[q & (DZF_RING - 1)] = (u8)v;
        }
        rf = F;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto ring4 = [&](u32 x) -> u32 {  // ring bytes x..x+3 (LE)
        const u32 a = x & ~3u, sh = 8 * (x & 3);
        const u32 lo = *(const u32*)(ring + (a & (DZF_RING - 1)));
        const u32 hi = *(const u32*)(ring + ((a + 4) & (DZF_RING - 1)));
        return sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
    };
    u32 p = 0;
    while (p < D32) {
        if (p - wb >= 250) {  // keep [p, p + 262) in the window (wb <= p always)
            wb = p & ~3u;
            w0 = dzf_ld4(src, wb + 4 * lane, D32, t);
            w1 = dzf_ld4(src, wb + 256 + 4 * lane, D32, t);
        }
        {
            const u32 F = p + 262 < D32 ? p + 262 : D32;
            if (F > rf) ring_fill(F);
        }
        {  // fill_window at the loop top: one slide when due
            const u32 wend = (D32 - base) > 2 * zz::WSIZE ? base + 2 * zz::WSIZE : D32;
            if (wend - p < zz::MIN_LOOKAHEAD && p - base >= zz::WSIZE + zz::MAX_DIST) {
                for (u32 i = lane; i < 32768; i += 64) {
                    const u32 x = ((u32*)smem_raw)[i];
                    const u32 lo = x & 0xFFFFu, hi = x >> 16;
                    ((u32*)smem_raw)[i] = (lo >= zz::WSIZE ? lo - zz::WSIZE : 0u) |
                                          ((hi >= zz::WSIZE ? hi - zz::WSIZE : 0u) << 16);
                }
                __syncthreads();
                base += zz::WSIZE;
            }
        }
        u32 ml = 0, md = 0;
        if (D32 - p >= zz::MIN_MATCH) {
            const u32 hh = insert(p);
            if (hh != 0 && (p - base) - hh <= zz::MAX_DIST) {
                // longest_match (zz::search's rules) over the chain from hh
                const u32 look = D32 - p;
                const u32 mx = look < zz::MAX_MATCH ? look : zz::MAX_MATCH;
                const u32 nice = cfg.nice < look ? cfg.nice : look;
                const u32 lim = p > zz::MAX_DIST ? p - zz::MAX_DIST : 0u;
                // my 4 bytes of p.. (lane l: p + 4 l ..) from the window
                const u32 pw = ring4(p + 4 * lane);
                u32 best = 0, bstart = 0, cand = hh + base;
                for (u32 k = 0; k < cfg.chain; k++) {
                    if (k > 0) {
                        const u32 r = rd(pv, (cand - base) & zz::WMASK);
                        if (r == 0) break;
                        cand = r + base;
                        if (cand <= lim) break;
                    }
                    const u32 cw = 4 * lane < mx ? ring4(cand + 4 * lane) : pw;
                    const u64 m = __ballot(pw != cw);
                    u32 len;
                    if (m) {
                        const u32 j = (u32)__builtin_ctzll(m);
                        const u32 x = (u32)__builtin_amdgcn_readlane((int)(pw ^ cw), (int)j);
                        len = 4 * j + ((u32)__builtin_ctz(x) >> 3);
                    } else {
                        len = 256;
                        while (len < mx && wbyte(p + len) == (u32)__builtin_amdgcn_readfirstlane((u32)ring[(cand + len) & (DZF_RING - 1)]))
                            len++;
                    }
                    if (len > mx) len = mx;
                    if (len > best) {
                        best = len;
                        bstart = cand;
                        if (best >= nice) break;
                    }
                }
                if (best >= zz::MIN_MATCH) {
                    ml = best;
                    md = p - bstart;
                }
            }
        }
        if (ml) {
            emit(0x80000000u | ((ml - zz::MIN_MATCH) << 16) | (md - 1), p);
            if (ml <= cfg.lazy && D32 - (p + ml) >= zz::MIN_MATCH)
                for (u32 q = p + 1; q < p + ml; q++) insert(q);
            p += ml;
        } else {
            emit(wbyte(p), p);
            p++;
        }
    }
    if (nsym & 63) {
        const u32 b0 = nsym & ~63u;
        if (lane < (nsym & 63)) {
            fsy[b0 + lane] = rs;
            fps[b0 + lane] = rp;
        }
    }
    __syncthreads();  // the final stream is in place
    const u32 nb = zz::num_blocks(nsym);
    auto P = [&](u32 i) -> u32 { return fps[i]; };
    auto Y = [&](u32 i) -> u32 { return fsy[i]; };
    for (u32 k = lane; k < nb && k < nbmax; k += 64) {
        const zz::BlockRec r = zz::block_rec(k, nsym, nsym, D32, P, Y, true);
        DzBlock* o = blks + (u64)c * nbmax + k;
        o->s0 = r.s0; o->s1 = r.s1; o->b0 = r.b0; o->b1 = r.b1; o->in_win = r.in_win; o->last = r.last;
    }
    if (lane == 0) {
        cs->fsym = (u64)(fsy - wbase);
        cs->fpos = (u64)(fps - wbase);
        cs->nsym = nsym;
        cs->nloop = nsym;
        cs->nblocks = nb <= nbmax ? nb : 0u;
        cs->status = nb <= nbmax ? ZCG_OK : ZCG_ERR_INVALID_DATA;
    }
}

struct DzPlanLds {
    zz::BlockWork bw;
    u32 lf[zz::L_CODES], df[zz::D_CODES];
    u32 hbits;
};

// One wave per block: histogram, zlib's trees and block-type decision, the
// header bit-string and the block's exact bit count.
__global__ __launch_bounds__(64) void dz_plan(u32 nc, DzChunk* __restrict__ cst, DzBlock* __restrict__ blks,
                                             u32 nbmax, const u32* __restrict__ wbase, u64 D) {
    __shared__ DzPlanLds L;
    const u32 c = blockIdx.x / nbmax, k = blockIdx.x % nbmax;
    if (c >= nc) return;
    const DzChunk cs = cst[c];
    if (cs.status != ZCG_OK || k >= cs.nblocks) return;
    DzBlock* B = blks + (u64)c * nbmax + k;
    const u32* sy = wbase + cs.fsym;
    const u32 lane = threadIdx.x;
    const u32 s0 = B->s0, s1 = B->s1;
    for (u32 i = lane; i < (u32)zz::L_CODES; i += 64) L.lf[i] = 0;
    if (lane < (u32)zz::D_CODES) L.df[lane] = 0;
    __syncthreads();
    for (u32 i = s0 + lane; i < s1; i += 64) {
        const u32 s = sy[i];
        if (!(s & 0x80000000u)) {
            atomicAdd(&L.lf[s & 0xFF], 1u);
        } else {
            atomicAdd(&L.lf[zz::len_code(((s >> 16) & 0xFF) + 3) + zz::LITERALS + 1], 1u);
            atomicAdd(&L.df[zz::dist_code((s & 0xFFFF) + 1)], 1u);
        }
    }
    __syncthreads();
    if (lane == 0) L.lf[zz::END_BLOCK] = 1;
    __syncthreads();
    for (u32 i = lane; i < (u32)zz::HEAP_SIZE; i += 64) L.bw.lt.freq[i] = i < (u32)zz::L_CODES ? L.lf[i] : 0u;
    for (u32 i = lane; i < (u32)(2 * zz::D_CODES + 1); i += 64) L.bw.dt.freq[i] = i < (u32)zz::D_CODES ? L.df[i] : 0u;
    for (u32 i = lane; i < DZ_HDRW; i += 64) B->hdr[i] = 0;
    __syncthreads();
    if (lane == 0) {
        const zz::BlockPlan pl = zz::plan_block(L.bw, B->b1 - B->b0, B->in_win != 0);
        u32 hb = 0;
        u32 acc = 0;  // header bit-string, LSB first, flushed word by word
        auto put = [&](u32 v, u32 n) {
            if (!n) return;
            v &= n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1);
            const u32 sh = hb & 31;
            acc |= v << sh;
            if (sh + n >= 32) {
                B->hdr[hb >> 5] = acc;
                acc = sh ? (v >> (32 - sh)) : 0u;
            }
            hb += n;
        };
        zz::send_header(L.bw, pl, B->last != 0, put);
        if (hb & 31) B->hdr[hb >> 5] = acc;
        B->type = pl.type;
        B->hbits = hb;
        L.hbits = hb;
        u64 db = 0;
        if (pl.type == zz::BT_DYN) {
            for (int i = 0; i < zz::L_CODES; i++) {
                const u32 x = i > zz::END_BLOCK ? zz::extra_lbits(i - 257) : 0u;
                db += (u64)L.lf[i] * (L.bw.lt.len[i] + x);
            }
            for (int i = 0; i < zz::D_CODES; i++) db += (u64)L.df[i] * (L.bw.dt.len[i] + zz::extra_dbits(i));
        } else if (pl.type == zz::BT_STATIC) {
            for (int i = 0; i < zz::L_CODES; i++) {
                const u32 x = i > zz::END_BLOCK ? zz::extra_lbits(i - 257) : 0u;
                db += (u64)L.lf[i] * (zz::static_llen(i) + x);
            }
            for (int i = 0; i < zz::D_CODES; i++) db += (u64)L.df[i] * (5 + zz::extra_dbits(i));
        }
        B->dbits = (u32)db;
    }
    __syncthreads();
    for (u32 i = lane; i < (u32)zz::L_CODES; i += 64) B->lcode[i] = L.bw.lt.code[i] | ((u32)L.bw.lt.len[i] << 16);
    if (lane < (u32)zz::D_CODES) B->dcode[lane] = L.bw.dt.code[lane] | ((u32)L.bw.dt.len[lane] << 16);
}

// Per chunk: block bit offsets (a stored block pads to a byte after its 3
// header bits), the stream length, and the boundary words cleared (blocks
// OR their first and last words in; every other word has one writer).
__global__ void dz_offsets(u32 nc, DzChunk* __restrict__ cst, DzBlock* __restrict__ blks, u32 nbmax, u8* out,
                           u64 outcap) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    DzChunk* cs = cst + c;
    if (cs->status != ZCG_OK) return;
    u32* ow = (u32*)(out + (u64)c * outcap);
    u64 acc = 0;
    for (u32 k = 0; k < cs->nblocks; k++) {
        DzBlock* B = blks + (u64)c * nbmax + k;
        B->bitoff = acc;
        ow[acc >> 5] = 0;
        if (B->type == zz::BT_STORED) {
            acc += 3;
            acc = (acc + 7) & ~7ull;
            acc += 32 + 8ull * (B->b1 - B->b0);
        } else {
            acc += (u64)B->hbits + B->dbits;
        }
        if (acc) ow[(acc - 1) >> 5] = 0;
    }
    ow[acc >> 5] = 0;
    cs->bytes = (acc + 7) >> 3;
    if (cs->bytes + 64 > outcap) cs->status = ZCG_ERR_OUTPUT_TOO_SMALL;
}

// One wave per block: its bits at its offset.  Symbols 64 at a time: each
// lane its symbol's bit count, a wave scan places them, and the bits are
// OR-ed into an LDS ring of words flushed in order (the block's first and
// last words with global atomics, the rest with plain stores).
struct DzEmitLds {
    u32 lc[zz::L_CODES], dc[zz::D_CODES];
    u32 ring[1024];
};

__global__ __launch_bounds__(64) void dz_emit(const zcg_chunk* __restrict__ chunks, u32 c0, u32 nc, u64 D, DType t,
                                             const DzChunk* __restrict__ cst, const DzBlock* __restrict__ blks,
                                             u32 nbmax, const u32* __restrict__ wbase, u8* out, u64 outcap) {
    __shared__ DzEmitLds L;
    const u32 c = blockIdx.x / nbmax, k = blockIdx.x % nbmax;
    if (c >= nc) return;
    const DzChunk cs = cst[c];
    if (cs.status != ZCG_OK || k >= cs.nblocks) return;
    const DzBlock* B = blks + (u64)c * nbmax + k;
    const u32 lane = threadIdx.x;
    const u32* sy = wbase + cs.fsym;
    u32* ow = (u32*)(out + (u64)c * outcap);
    const u64 b0 = B->bitoff;
    const u32 type = B->type;
    const bool stat = type == zz::BT_STATIC;
    for (u32 i = lane; i < (u32)zz::L_CODES; i += 64) L.lc[i] = B->lcode[i];
    if (lane < (u32)zz::D_CODES) L.dc[lane] = B->dcode[lane];
    for (u32 i = lane; i < 1024; i += 64) L.ring[i] = 0;
    __syncthreads();
    // bit position relative to the aligned word holding bit b0
    const u64 w0 = b0 >> 5;
    u32 pos = (u32)(b0 & 31);  // next bit, relative to 32 * w0
    u32 fw = 0;                // ring words flushed (relative to w0)
    u64 bend = 0;              // the block's end bit, relative to 32 * w0
    {
        u64 len = (u64)B->hbits + B->dbits;
        if (type == zz::BT_STORED) len = 0;  // (computed below)
        bend = pos + len;
    }
    auto put_lane = [&](u32 at, u32 v, u32 n) {  // at: relative bit; n <= 32
        if (!n) return;
        v &= n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1);
        const u32 w = at >> 5, sh = at & 31;
        atomicOr(&L.ring[w & 1023], v << sh);
        if (sh + n > 32) atomicOr(&L.ring[(w + 1) & 1023], v >> (32 - sh));
    };
    auto flush_to = [&](u32 upto, bool fin) {  // words [fw, upto) are complete (fin: and the partial last one)
        __syncthreads();
        const u32 lastw = fin ? (u32)((bend + 31) >> 5) : upto;
        for (u32 w = fw + lane; w < lastw; w += 64) {
            const u32 v = L.ring[w & 1023];
            const bool edge = (w == 0) || (fin && w == lastw - 1);
            if (edge) atomicOr(&ow[w0 + w], v);
            else ow[w0 + w] = v;
            L.ring[w & 1023] = 0;
        }
        fw = lastw;
        __syncthreads();
    };
    // header bit-string
    {
        const u32 hb = B->hbits;
        for (u32 i = lane; i < (hb + 31) / 32; i += 64) {
            const u32 n = (i + 1) * 32 <= hb ? 32u : hb - i * 32;
            put_lane(pos + i * 32, B->hdr[i], n);
        }
        pos += hb;
    }
    if (type == zz::BT_STORED) {
        pos = (pos + 7) & ~7u;
        const u32 len = B->b1 - B->b0;
        if (lane == 0) {
            put_lane(pos, len & 0xFFFF, 16);
            put_lane(pos + 16, ~len & 0xFFFF, 16);
        }
        pos += 32;
        bend = pos + 8ull * len;
        const u8* src = (const u8*)chunks[c0 + c].src;
        for (u32 i0 = 0; i0 < len; i0 += 256) {
            __syncthreads();
            for (u32 i = i0 + lane; i < i0 + 256 && i < len; i += 64)
                put_lane(pos + 8 * i, ser1(src, (u64)B->b0 + i, t), 8);
            flush_to((pos + 8 * (i0 + 256 < len ? i0 + 256 : len)) >> 5, false);
        }
        flush_to(0, true);
        return;
    }
    const u32 s0 = B->s0, s1 = B->s1;
    for (u32 i0 = s0; i0 < s1; i0 += 64) {
        const u32 i = i0 + lane;
        zz::SymBits sb{{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (i < s1) {
            const u32 s = sy[i];
            if (stat) {
                sb = zz::sym_bits(s, true, nullptr, nullptr, nullptr, nullptr);
            } else if (!(s & 0x80000000u)) {
                const u32 e = L.lc[s & 0xFF];
                sb.v[0] = e & 0xFFFF;
                sb.n[0] = e >> 16;
            } else {
                const u32 lc = (s >> 16) & 0xFF, dist = (s & 0xFFFF) + 1;
                const int code = (int)zz::len_code(lc + 3);
                const u32 e = L.lc[code + zz::LITERALS + 1];
                sb.v[0] = e & 0xFFFF;
                sb.n[0] = e >> 16;
                sb.n[1] = zz::extra_lbits(code);
                sb.v[1] = lc - zz::base_length(code);
                const int dcd = (int)zz::dist_code(dist);
                const u32 f = L.dc[dcd];
                sb.v[2] = f & 0xFFFF;
                sb.n[2] = f >> 16;
                sb.n[3] = zz::extra_dbits(dcd);
                sb.v[3] = (dist - 1) - zz::base_dist(dcd);
            }
        }
        const u32 nbits = sb.n[0] + sb.n[1] + sb.n[2] + sb.n[3];
        u32 x = nbits;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = __shfl_up(x, d, 64);
            if ((int)lane >= d) x += y;
        }
        u32 at = pos + x - nbits;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // a part is <= 15 bits, so two parts always fit one 32-bit put
            put_lane(at, sb.v[j], sb.n[j]);
            at += sb.n[j];
        }
        pos += __shfl(x, 63, 64);
        if (((pos >> 5) - fw) >= 512) flush_to(pos >> 5, false);
    }
    if (lane == 0) {
        const u32 e = stat ? (zz::static_lcode(zz::END_BLOCK) | (7u << 16)) : L.lc[zz::END_BLOCK];
        put_lane(pos, e & 0xFFFF, e >> 16);
    }
    flush_to(0, true);
}

// Per chunk: the container's header (df_put_header), the stream, its trailer: CRC32/ISIZE or the
// Adler-32 (the checksum from gzip_crc32's crc_out / zlib_adler32's sum_out mode, run before).
__global__ __launch_bounds__(256) void dz_final(const zcg_chunk* __restrict__ chunks, u32 c0, u32 nc, u64 D,
                                               u64 bound, u32 xfl, u32 zhdr, const DzChunk* __restrict__ cst,
                                               const u8* out, u64 outcap, u64* __restrict__ out_len,
                                               i32* __restrict__ status, const u32* __restrict__ crc) {
    const u32 c = blockIdx.x, tid = threadIdx.x;
    if (c >= nc) return;
    const zcg_chunk ch = chunks[c0 + c];
    const DzChunk cs = cst[c];
    const u32 H = df_header_bytes(zhdr), T = df_trailer_bytes(zhdr);
    if (ch.src_len < D) { if (tid == 0) { status[c0 + c] = ZCG_ERR_INVALID_DATA; out_len[c0 + c] = 0; } return; }
    if (cs.status != ZCG_OK) { if (tid == 0) { status[c0 + c] = (i32)cs.status; out_len[c0 + c] = 0; } return; }
    if (ch.dst_cap < bound || ch.dst_cap < H + cs.bytes + T) {
        if (tid == 0) { status[c0 + c] = ZCG_ERR_OUTPUT_TOO_SMALL; out_len[c0 + c] = 0; }
        return;
    }
    u8* dst = (u8*)ch.dst;
    const u8* o = out + (u64)c * outcap;
    if (tid == 0) df_put_header(dst, xfl, zhdr);
    const u64 n = cs.bytes;
    for (u64 i = (u64)tid * 16; i < n; i += 256 * 16) {
        if (i + 16 <= n) st16(dst + H + i, *(const u32x4*)(o + i));
        else for (u64 j = i; j < n; j++) dst[H + j] = o[j];
    }
    if (tid == 0) {
        const u32 r = crc[c], isz = (u32)D;
        u8* tr = dst + H + n;
        if (zhdr) {
            const u8 t4[4] = {(u8)(r >> 24), (u8)(r >> 16), (u8)(r >> 8), (u8)r};
            for (u32 i = 0; i < 4; i++) tr[i] = t4[i];
        } else {
            const u8 t8[8] = {(u8)r, (u8)(r >> 8), (u8)(r >> 16), (u8)(r >> 24),
                              (u8)isz, (u8)(isz >> 8), (u8)(isz >> 16), (u8)(isz >> 24)};
            for (u32 i = 0; i < 8; i++) tr[i] = t8[i];
        }
        out_len[c0 + c] = H + n + T;
        status[c0 + c] = ZCG_OK;
    }
}

}  // namespace

static hipError_t launch_deflate_exact(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, u32 level,
                                       uint64_t* d_out_len, int32_t* d_status, void* ws, uint64_t ws_bytes,
                                       hipStream_t s, hipStream_t side, hipEvent_t fork, hipEvent_t join) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    const u32 xfl = level >= 9 ? 2u : (level <= 1 ? 4u : 0u);
    const u32 zhdr = zlib_header_word(a, level);
    const u64 bound = zcg_encode_bound(&a->compression, D);
    if (D >= (1ull << 31)) {  // u32 positions: every chunk UNSUPPORTED, the launch itself succeeds
        if (hipError_t e = hipMemsetD32Async((hipDeviceptr_t)d_status, ZCG_ERR_UNSUPPORTED, n, s); e != hipSuccess)
            return e;
        return hipMemsetAsync(d_out_len, 0, sizeof(uint64_t) * (size_t)n, s);
    }
    const DzWs y = dz_ws(D, n);
    if (ws_bytes < y.total || y.b.tot >= (1ull << 31)) return hipErrorInvalidValue;
    const zz::Config cfg = zz::level_config((int)level);
    u8* w = (u8*)ws;
    uint2* m2 = (uint2*)(w + y.off_m2);
    DzChunk* cst = (DzChunk*)(w + y.off_ch);
    DzBlock* blks = (DzBlock*)(w + y.off_blk);
    u8* out = w + y.off_out;
    const bool fast = level <= 3;
    // deflate_fast takes the whole CU's 160 KiB of LDS (head/prev + the input ring)
    if (fast) {
        if (hipError_t e = lds_attr_once((const void*)dz_parse_fast, (int)DZF_LDS_RING); e != hipSuccess) return e;
    }
    const bool two = side && fork && join && !fast;  // the parse of each sub-batch on the side stream
    SideFork sf{s, side, fork, join};  // (its destructor joins on every return below an open fork)
    u32* crcb = (u32*)(w + y.off_crc);
    // blocks (trees, header bits), their bit offsets, the bits, the container
    // with its CRC32 trailer: for the chunks [s0 + cb, s0 + cb + cnt) of the
    // super-batch at s0
    auto tail = [&](u32 s0, u32 cb, u32 cnt, hipStream_t ts) -> hipError_t {
        const u64 nbk = (u64)cnt * y.nbmax;
        DzChunk* cs = cst + cb;
        DzBlock* bk = blks + (u64)cb * y.nbmax;
        u8* ot = out + (u64)cb * y.outcap;
        hipLaunchKernelGGL(dz_plan, dim3((u32)nbk), dim3(64), 0, ts, cnt, cs, bk, y.nbmax, (const u32*)w, D);
        hipLaunchKernelGGL(dz_offsets, dim3((cnt + 63) / 64), dim3(64), 0, ts, cnt, cs, bk, y.nbmax, ot, y.outcap);
        hipLaunchKernelGGL(dz_emit, dim3((u32)nbk), dim3(64), 0, ts, d_chunks, s0 + cb, cnt, D, t, (const DzChunk*)cs,
                           (const DzBlock*)bk, y.nbmax, (const u32*)w, ot, y.outcap);
        hipLaunchKernelGGL(dz_final, dim3(cnt), dim3(256), 0, ts, d_chunks, s0 + cb, cnt, D, bound, xfl, zhdr,
                           (const DzChunk*)cs, (const u8*)ot, y.outcap, (u64*)d_out_len, (i32*)d_status,
                           (const u32*)crcb + cb);
        return hipGetLastError();
    };
    for (u32 s0 = 0; s0 < n; s0 += y.b.sm) {
        const u32 scnt = batch_count(s0, n, y.b.sm);
        // a parse that does not run leaves every chunk failed, so the kernels
        // after it never read an unset record
        if (hipError_t e = hipMemsetAsync(cst, 0xFF, sizeof(DzChunk) * (size_t)scnt, s); e != hipSuccess) return e;
        // the inputs' checksums: on the side stream (idle until the first parse)
        // beside the first match search, else in line.  (Sorting sub-batch
        // i + 1 on the side stream beside match search i measured slower,
        // 133.7 vs 126.0 ms per C5 call: the search takes the CUs, the sort
        // beside it ran 20 instead of 3 ms and held back the parses.)
        {
            hipStream_t cs = s;
            if (two && D > 0) {
                if (hipError_t e = sf.fork(); e != hipSuccess) return e;
                cs = side;
            }
            if (hipError_t e = launch_stream_checksum(zhdr, d_chunks + s0, scnt, D, t, nullptr, nullptr, crcb, cs);
                e != hipSuccess)
                return e;
        }
        for (u32 c0 = s0; c0 < s0 + scnt && D > 0 && !fast; c0 += y.b.m) {
            const u32 cnt = batch_count(c0, s0 + scnt, y.b.m);
            const u64 tot = (u64)cnt * D;
            const u32 G = (u32)((tot + 255) / 256);
            u32 *keys = (u32*)(w + y.c.ka), *vals = (u32*)(w + y.c.va);
            hipLaunchKernelGGL(dz_keys, dim3(G), dim3(256), 0, s, d_chunks, c0, D, tot, t, keys, vals);
            hipError_t e = sort_pairs_u32(w + y.c.cub, y.c.cub_bytes, keys, (u32*)(w + y.c.kb), vals,
                                          (u32*)(w + y.c.vb), tot, 16 + id_bits(cnt), s, &keys, &vals);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(dz_best, dim3(G), dim3(256), 0, s, d_chunks, c0, D, tot, t, cfg, (const u32*)keys,
                               (const u32*)vals, m2 + (u64)(c0 - s0) * D);
            // the sub-batch's lazy parse (one wave per chunk: a few waves per
            // CU) runs beside the next sub-batch's sort and match search
            hipStream_t ps = s;
            if (two) {
                if ((e = sf.fork()) != hipSuccess) return e;
                ps = side;
            }
            hipLaunchKernelGGL(dz_parse, dim3(cnt), dim3(64), 0, ps, d_chunks, c0, cnt, D, t, cfg, (u32*)w,
                               y.off_m2 / 4, y.off_sym / 4, y.off_pos / 4, y.off_bm / 4, y.off_tail / 4, cst, blks,
                               y.nbmax, c0 - s0);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            // and the rest of the sub-batch's encode right behind it
            if (two && (e = tail(s0, c0 - s0, cnt, side)) != hipSuccess) return e;
        }
        if (hipError_t e = sf.join(); e != hipSuccess) return e;
        if (fast) {
            hipLaunchKernelGGL(dz_parse_fast, dim3(scnt), dim3(64), DZF_LDS_RING, s, d_chunks, s0, scnt, D, t, cfg,
                               (u32*)w, y.off_m2 / 4, cst, blks, y.nbmax);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        if (!fast && D == 0) {  // (empty chunks: the parse writes their empty streams)
            hipLaunchKernelGGL(dz_parse, dim3(scnt), dim3(64), 0, s, d_chunks, s0, scnt, D, t, cfg, (u32*)w,
                               y.off_m2 / 4, y.off_sym / 4, y.off_pos / 4, y.off_bm / 4, y.off_tail / 4, cst, blks,
                               y.nbmax, 0u);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        if (!two || D == 0) {
            if (hipError_t e = tail(s0, 0, scnt, s); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// levels 1-9 reproduce zlib's bytes (1-3 deflate_fast, 4-9 deflate_slow);
// level 0 (stored) and ZCG_FLAG_GZIP_SEGMENTED take the segmented coder
static bool deflate_exact_level(const zcg_array* a) {
    const int level = zcg_effective_gzip_level(a->compression.gzip_level);
    return level >= 1 && (a->compression.flags & ZCG_FLAG_GZIP_SEGMENTED) == 0;
}

uint64_t deflate_ws_bytes(const zcg_array* a, uint32_t n) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    if (n == 0) return 0;
    if (!deflate_exact_level(a)) return deflate_seg_ws_bytes(D, n);
    return D >= (1ull << 31) ? 0 : dz_ws(D, n).total;  // (chunks of >= 2 GiB: per-chunk UNSUPPORTED)
}

const char* cfg_deflate() { return "deflate:CHAIN6=" ZCG_STR(ZCG_DF_CHAIN6) ",SUB=" ZCG_STR(ZDZ_SUB_MIB); }

hipError_t launch_deflate(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n,
                          uint64_t* d_out_len, int32_t* d_status, void* ws, uint64_t ws_bytes,
                          hipStream_t s, hipStream_t side, hipEvent_t fork, hipEvent_t join) {
    if (n == 0) return hipSuccess;
    const u32 level = (u32)zcg_effective_gzip_level(a->compression.gzip_level);
    if (deflate_exact_level(a))
        return launch_deflate_exact(a, d_chunks, n, level, d_out_len, d_status, ws, ws_bytes, s, side, fork, join);
    return launch_deflate_seg(a, d_chunks, n, level, d_out_len, d_status, ws, ws_bytes, s);
}

}  // namespace zcg
