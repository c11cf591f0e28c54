// zcg_verify.hip — opt-in checksum verification of decoded chunks
// (ZCG_FLAG_VERIFY_GZIP_TRAILER, ZCG_FLAG_VERIFY_ZLIB_TRAILER,
// ZCG_FLAG_VERIFY_LZ4_CONTENT; rules in
// include/zchunk_gpu.h).  The decoders locate the trailer and leave one
// VerifyRec per chunk; the kernels here read each decoded byte once, in stream
// order, checksum it, apply the part of the element transform the decoder was
// told to leave out, and turn a mismatch into ZCG_ERR_INVALID_DATA.
//
// crc32_verify (gzip).  A chunk is cut into at most 64 slices, one per wave,
// four waves per workgroup.  A wave reads a slice in 1 KiB tiles, lane l the
// 16 bytes at l*16 of every tile (one coalesced 16 B/lane load per tile), so a
// lane's bytes are a comb through the slice, not a run.  CRC32 is linear: a
// lane's register after "16 bytes, then 1008 bytes of zeros" is one
// slice-by-16 step with tables multiplied by x^(8*1008) mod P, so the comb
// costs the same 16 LDS lookups per 16 bytes as a contiguous run and the lanes
// need no fold until the slice ends.  Two table sets sit in LDS (32 KiB, built
// once per workgroup, workgroups loop over their work): TZ (step + skip 1008)
// for every tile but the last, T (plain slice-by-16) for the last.  The lanes
// are then 16 bytes apart, and a 6-level shuffle tree with the multipliers
// x^(128*2^k) folds them into lane 63.  A slice shorter than a whole number of
// tiles is padded with virtual zero bytes IN FRONT (zeros ahead of a message do
// not move a zero register), so every slice ends on its last lane's last byte;
// the 0xFFFFFFFF initial value and final inversion are one constant the host
// derives from D.  crc32_fold folds a chunk's slices with the same tree
// (multipliers x^(8*slice*2^k)), compares and writes the status.
// Table layout: [k][256] words, so a lookup's bank is its byte value mod 64.
// The 64 lanes' bytes are independent, i.e. 64 balls in 64 banks whatever the
// layout; replicating the tables spreads the lanes over the same number of
// banks and padding only renames them, so neither is done.
//
// adler32_verify (zlib).  The same slices, tiles and loads; Adler-32's two sums
// do not depend on how the bytes are cut up, so a lane keeps three unreduced
// sums over its comb (zcg_adler.h: the arithmetic and its deferred-modulo
// bound), takes them mod 65521 once per slice, and lanes, waves and slices fold
// by modular addition: no tables, no LDS.
//
// xxh32_verify (LZ4).  XXH32's four accumulators are serial over the whole
// content, so the parallelism is across chunks: 16 chunks per wave, 4 lanes
// (accumulators) each.  Each step the whole wave loads the next 1 KiB of every
// chunk (16 B/lane, coalesced, the next step's loads in flight during this
// step's hashing) into a padded LDS row per chunk, applies the owed byte swap
// / bool rule to the registers and stores them back, and then lane (chunk,
// accumulator) walks its chunk's row one 16-byte stripe at a time.
#include "zcg_common.h"
#include "zcg_crc.h"
#include "zcg_adler.h"

namespace zcg {

// ---- GF(2) arithmetic on the host (the per-launch multipliers) ------------------------------------
static u32 h_mulmod(u32 a, u32 b) {  // zlib's multmodp
    u32 m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ CRC32_POLY : b >> 1;
    }
    return p;
}
static u32 h_xpow8n(u64 nbytes) {  // x^(8*nbytes) mod P
    u32 r = 1u << 31, p = 1u << 23;
    while (nbytes) {
        if (nbytes & 1) r = h_mulmod(p, r);
        p = h_mulmod(p, p);
        nbytes >>= 1;
    }
    return r;
}

constexpr u32 CV_NT = 256;          // threads per workgroup (4 waves = 4 slices)
constexpr u32 CV_TILE = 1024;       // bytes a wave reads per step
constexpr u32 CV_MAX_PARTS = 64;    // slices per chunk (one wave folds them)
constexpr u32 CV_MIN_SLICE = 16384; // bytes
constexpr u32 CV_WG_PER_CU = 4;     // 32 KiB of tables each

struct CrcArgs {
    u32 slice;    // bytes per slice (a multiple of CV_TILE); the last one may be shorter
    u32 nparts;   // slices per chunk, 1..CV_MAX_PARTS
    u32 xz;       // x^(8*(CV_TILE-16))
    u32 lm[6];    // x^(8*16*2^k): lanes 2^k apart
    u32 pm[6];    // x^(8*slice*2^k): slices 2^k apart
    u32 xlast;    // x^(8*(length of the last slice))
    u32 k;        // (0xFFFFFFFF * x^(8*D)) ^ 0xFFFFFFFF: initial value and final inversion
};

__device__ __forceinline__ u32 crc_step16(const u32* tab, u32x4 w) {
    return tab[15 * 256 + (w.x & 0xFF)] ^ tab[14 * 256 + ((w.x >> 8) & 0xFF)] ^ tab[13 * 256 + ((w.x >> 16) & 0xFF)] ^
           tab[12 * 256 + (w.x >> 24)] ^ tab[11 * 256 + (w.y & 0xFF)] ^ tab[10 * 256 + ((w.y >> 8) & 0xFF)] ^
           tab[9 * 256 + ((w.y >> 16) & 0xFF)] ^ tab[8 * 256 + (w.y >> 24)] ^ tab[7 * 256 + (w.z & 0xFF)] ^
           tab[6 * 256 + ((w.z >> 8) & 0xFF)] ^ tab[5 * 256 + ((w.z >> 16) & 0xFF)] ^ tab[4 * 256 + (w.z >> 24)] ^
           tab[3 * 256 + (w.w & 0xFF)] ^ tab[2 * 256 + ((w.w >> 8) & 0xFF)] ^ tab[1 * 256 + ((w.w >> 16) & 0xFF)] ^
           tab[0 * 256 + (w.w >> 24)];
}

// Fold of 64 lanes' registers that sit `2^k * unit` bytes apart (mul[k] =
// x^(8*unit*2^k)): lane 63 receives the register of the whole.
__device__ __forceinline__ u32 crc_lane_tree(u32 v, const u32* mul, u32 lane) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32 lo = (u32)__shfl_xor((int)v, 1 << k, 64);
        if ((lane >> k) & 1) v ^= gf2_mulmod<u32, CRC32_POLY>(lo, mul[k]);
    }
    return v;
}

// The 16 stream-order bytes of a tile piece at logical chunk offset p (16
// whole bytes inside the chunk); bool chunks get their normalised bytes back.
__device__ __forceinline__ u32x4 cv_load16(u8* dst, u64 p, const DType& t) {
    const u32x4 raw = ld16(dst + p);
    if (t.isbool) {
        const u32x4 nb = transform16(raw, t);
        if (nb.x != raw.x || nb.y != raw.y || nb.z != raw.z || nb.w != raw.w) st16(dst + p, nb);
        return raw;
    }
    return transform16(raw, t);  // '>' types: the swap is its own inverse
}

__global__ __launch_bounds__(CV_NT) void crc32_verify_kernel(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                             DType t, CrcArgs a,
                                                             const VerifyRec* __restrict__ rec,
                                                             u32* __restrict__ partials) {
    __shared__ u32 tabs[2 * 16 * 256];  // T, then TZ
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    {
        u32 v = g_crc32_table[tid];
        tabs[tid] = v;
        __syncthreads();
        tabs[4096 + tid] = gf2_mulmod<u32, CRC32_POLY>(v, a.xz);
        for (u32 k = 1; k < 16; k++) {
            v = (v >> 8) ^ tabs[v & 0xFF];
            tabs[k * 256 + tid] = v;
            tabs[4096 + k * 256 + tid] = gf2_mulmod<u32, CRC32_POLY>(v, a.xz);
        }
        __syncthreads();
    }
    const u32 gpc = (a.nparts + 3) / 4;  // workgroup items per chunk
    const u64 items = (u64)n * gpc;
    for (u64 item = blockIdx.x; item < items; item += gridDim.x) {
        const u32 c = (u32)(item / gpc);
        const u32 part = (u32)(item % gpc) * 4 + wv;
        if (part >= a.nparts || rec[c].mode != V_CHECK) continue;  // (wave-uniform; no barrier below)
        u8* const dst = (u8*)chunks[c].dst;
        const u64 off = (u64)part * a.slice;
        const u32 L = (u32)(D - off < a.slice ? D - off : a.slice);
        const u32 pad = (CV_TILE - L % CV_TILE) % CV_TILE;  // virtual zero bytes in front
        const u32 ntile = (L + pad) / CV_TILE;
        const u32 v0 = lane * 16;  // my bytes of a tile
        // tile 0: the only one that can hold padding
        u32x4 cur = {0u, 0u, 0u, 0u};
        if (v0 >= pad) {
            cur = cv_load16(dst, off + v0 - pad, t);
        } else if (v0 + 16 > pad) {  // the piece the slice starts in
            u32 w[4] = {0u, 0u, 0u, 0u};
            for (u32 j = pad - v0; j < 16; j++) {
                const u64 q = off + v0 + j - pad;  // stream-order position
                const u64 ph = swap_pos(q, t);
                const u32 b = dst[ph];
                w[j >> 2] |= b << (8 * (j & 3));
                if (t.isbool && b > 1) dst[ph] = 1;
            }
            cur = u32x4{w[0], w[1], w[2], w[3]};
        }
        u32 crc = 0;
        const u64 base = off - pad + v0;  // (tile k piece at base + k * CV_TILE; k >= 1 is inside the slice)
        for (u32 k = 0; k < ntile; k++) {
            u32x4 nxt = {0u, 0u, 0u, 0u};
            if (k + 1 < ntile) nxt = cv_load16(dst, base + (u64)(k + 1) * CV_TILE, t);
            cur.x ^= crc;
            crc = crc_step16(tabs + (k + 1 < ntile ? 4096u : 0u), cur);
            cur = nxt;
        }
        crc = crc_lane_tree(crc, a.lm, lane);
        if (lane == 63) partials[(u64)c * CV_MAX_PARTS + part] = crc;
    }
}

__global__ __launch_bounds__(64) void crc32_fold_kernel(u32 n, CrcArgs a, const VerifyRec* __restrict__ rec,
                                                        const u32* __restrict__ partials,
                                                        i32* __restrict__ status) {
    const u32 c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    const VerifyRec rc = rec[c];
    if (rc.mode != V_CHECK) return;
    const u32* const pp = partials + (u64)c * CV_MAX_PARTS;
    // slices 0 .. nparts-2 are a.slice bytes each: the tree, ending at lane 63
    const int idx = (int)lane - (int)(64 - (a.nparts - 1));
    u32 v = idx >= 0 ? pp[idx] : 0u;
    v = crc_lane_tree(v, a.pm, lane);
    if (lane == 63) {
        const u32 crc = gf2_mulmod<u32, CRC32_POLY>(v, a.xlast) ^ pp[a.nparts - 1] ^ a.k;
        if (crc != rc.expect) status[c] = ZCG_ERR_INVALID_DATA;
    }
}

// ---- Adler-32 (zlib) ---------------------------------------------------------------------------
// crc32_verify's slices, tiles and loads; the sums are zcg_adler.h's.  A slice
// that is no whole number of tiles is padded with virtual zero pieces at its
// END (they add nothing to a sum, and the front pieces then sit 16-aligned in
// the chunk).  A wave's partial is the sum of its lanes' partials, a chunk's
// the sum of its slices': adler32_fold adds them, compares and writes the status.
static_assert(0x100000000ull / CV_MAX_PARTS / CV_TILE + 1 <= ADLER_LANE_MAX_PIECES,
              "a lane's pieces of the longest slice (D < 2^32) stay inside the deferred-modulo bound");

__global__ __launch_bounds__(CV_NT) void adler32_verify_kernel(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                               DType t, u32 slice, u32 nparts,
                                                               const VerifyRec* __restrict__ rec,
                                                               u32* __restrict__ partials) {
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u32 gpc = (nparts + 3) / 4;  // workgroup items per chunk
    const u64 items = (u64)n * gpc;
    for (u64 item = blockIdx.x; item < items; item += gridDim.x) {
        const u32 c = (u32)(item / gpc);
        const u32 part = (u32)(item % gpc) * 4 + wv;
        if (part >= nparts || rec[c].mode != V_CHECK) continue;  // (wave-uniform; no barrier below)
        u8* const dst = (u8*)chunks[c].dst;
        const u64 off = (u64)part * slice;
        const u64 end = D - off < slice ? D : off + slice;  // (of the slice, in the chunk)
        const u32 ntile = (u32)((end - off + CV_TILE - 1) / CV_TILE);
        const u64 base = off + lane * 16;  // my piece of tile k at base + k * CV_TILE
        auto piece = [&](u64 p) -> u32x4 {
            if (p + 16 <= end) return cv_load16(dst, p, t);
            u32 w[4] = {0u, 0u, 0u, 0u};
            for (u64 q = p; q < end; q++) {  // the piece the chunk ends in (only the last slice is short)
                const u64 ph = swap_pos(q, t);
                const u32 b = dst[ph];
                w[(q - p) >> 2] |= b << (8 * ((q - p) & 3));
                if (t.isbool && b > 1) dst[ph] = 1;
            }
            return u32x4{w[0], w[1], w[2], w[3]};
        };
        AdlerLane al = adler_lane_open();
        u32x4 cur = piece(base);
        for (u32 k = 0; k < ntile; k++) {
            u32x4 nxt = {0u, 0u, 0u, 0u};
            if (k + 1 < ntile) nxt = piece(base + (u64)(k + 1) * CV_TILE);
            adler_lane_piece(al, cur.x, cur.y, cur.z, cur.w);
            cur = nxt;
        }
        const i64 E = (i64)D - (i64)(base + (u64)(ntile - 1) * CV_TILE) - 16;
        const u32 v = adler_wave_sum(adler_lane_close(al, E, CV_TILE));
        if (lane == 0) partials[(u64)c * CV_MAX_PARTS + part] = v;
    }
}

__global__ __launch_bounds__(64) void adler32_fold_kernel(u32 n, u64 D, u32 nparts, const VerifyRec* __restrict__ rec,
                                                          const u32* __restrict__ partials,
                                                          i32* __restrict__ status) {
    const u32 c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    const VerifyRec rc = rec[c];
    if (rc.mode != V_CHECK) return;
    const u32 v = adler_wave_sum(lane < nparts ? partials[(u64)c * CV_MAX_PARTS + lane] : 0u);
    if (lane == 0 && adler_finish(v, D) != rc.expect) status[c] = ZCG_ERR_INVALID_DATA;
}

// ---- XXH32 -------------------------------------------------------------------------------------
constexpr u32 XV_CPW = 16;              // chunks per wave
constexpr u32 XV_PIECE = 1024;          // bytes of a chunk per step
constexpr u32 XV_ROW = XV_PIECE + 16;   // LDS row stride: the 16 rows' stripes fall in distinct banks

__global__ __launch_bounds__(64) void xxh32_verify_kernel(const zcg_chunk* __restrict__ chunks, u32 n, u64 D,
                                                          DType t, const VerifyRec* __restrict__ rec,
                                                          i32* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) u8 stage[XV_CPW * XV_ROW];
    __shared__ u8* s_dst[XV_CPW];
    const u32 lane = threadIdx.x, j = lane >> 2, acc = lane & 3;
    const u32 c = blockIdx.x * XV_CPW + j;
    VerifyRec rc{V_SKIP, 0u};
    u8* mydst = nullptr;
    if (c < n) {
        rc = rec[c];
        mydst = (u8*)chunks[c].dst;
    }
    // bit 4*jj: chunk jj of this wave is hashed
    const unsigned long long active = __ballot(rc.mode != V_SKIP) & 0x1111111111111111ull;
    if (active == 0) return;
    const bool owed = t.swap || t.isbool;
    if (acc == 0) s_dst[j] = mydst;
    __syncthreads();
    auto dst_of = [&](u32 jj) -> u8* { return s_dst[jj]; };  // (an LDS broadcast read)
    u32x4 buf[XV_CPW];
    auto fetch = [&](u64 pos) {  // whole 16-byte stripes only; a shorter last one is read at its step
        const u64 p = pos + (u64)lane * 16;
#pragma unroll
        for (u32 jj = 0; jj < XV_CPW; jj++)
            if (((active >> (4 * jj)) & 1) && p + 16 <= D) buf[jj] = ld16(dst_of(jj) + p);
    };
    u32 v = acc == 0 ? XXH_P1 + XXH_P2 : acc == 1 ? XXH_P2 : acc == 2 ? 0u : 0u - XXH_P1;
    fetch(0);
    for (u64 pos = 0; pos < D; pos += XV_PIECE) {
        const u64 p = pos + (u64)lane * 16;
#pragma unroll
        for (u32 jj = 0; jj < XV_CPW; jj++) {
            if (!((active >> (4 * jj)) & 1)) continue;
            u8* const row = stage + jj * XV_ROW;
            if (p + 16 <= D) {
                *(u32x4*)(row + lane * 16) = buf[jj];
                if (owed) st16(dst_of(jj) + p, transform16(buf[jj], t));
            }
        }
        if (p < D && p + 16 > D) {  // one lane, once: the chunks' last bytes, whole elements (D % es == 0)
            const u32 m = (u32)(D - p);
#pragma nounroll
            for (u32 jj = 0; jj < XV_CPW; jj++) {
                if (!((active >> (4 * jj)) & 1)) continue;
                u8* const d = dst_of(jj);
                u8* const row = stage + jj * XV_ROW + lane * 16;
                for (u32 i = 0; i < m; i++) row[i] = d[p + i];
                if (owed)
                    for (u32 i = 0; i < m; i++) d[swap_pos(p + i, t)] = norm_byte(row[i], t);
            }
        }
        __syncthreads();
        if (pos + XV_PIECE < D) fetch(pos + XV_PIECE);
        const u64 left = D - pos;
        const u32 ns = left >= XV_PIECE ? XV_PIECE / 16 : (u32)(left / 16);
        const u32* const mine = (const u32*)(stage + j * XV_ROW) + acc;
        for (u32 s = 0; s < ns; s++) v = rotl32(v + mine[s * 4] * XXH_P2, 13) * XXH_P1;
        if (pos + XV_PIECE < D) __syncthreads();  // (the last piece stays for the tail below)
    }
    const u32 v1 = (u32)__shfl((int)v, (int)(j * 4), 64), v2 = (u32)__shfl((int)v, (int)(j * 4 + 1), 64);
    const u32 v3 = (u32)__shfl((int)v, (int)(j * 4 + 2), 64), v4 = (u32)__shfl((int)v, (int)(j * 4 + 3), 64);
    if (acc != 0 || rc.mode != V_CHECK) return;
    u32 h = D >= 16 ? rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18) : XXH_P5;
    h += (u32)D;
    {  // the last D % 16 bytes, still in the stage row
        const u32 rem = (u32)(D & 15);
        const u64 last_pos = (D - 1) / XV_PIECE * XV_PIECE;
        const u8* q = stage + j * XV_ROW + (u32)(D - rem - last_pos);
        const u8* const end = q + rem;
        for (; q + 4 <= end; q += 4) h = rotl32(h + *(const u32*)q * XXH_P3, 17) * XXH_P4;
        for (; q < end; q++) h = rotl32(h + *q * XXH_P5, 11) * XXH_P1;
    }
    h ^= h >> 15; h *= XXH_P2; h ^= h >> 13; h *= XXH_P3; h ^= h >> 16;
    if (h != rc.expect) status[c] = ZCG_ERR_INVALID_DATA;
}

// ---- host --------------------------------------------------------------------------------------
static uint64_t verify_rec_bytes(uint32_t n) { return ((u64)n * sizeof(VerifyRec) + 255) / 256 * 256; }

uint64_t verify_ws_bytes(uint32_t n) { return verify_rec_bytes(n) + (u64)n * CV_MAX_PARTS * 4 + 256; }

// (the decoder's own workspace may end at any 4-byte multiple)
static u8* verify_base(void* varea) { return (u8*)(((uintptr_t)varea + 255) & ~(uintptr_t)255); }

hipError_t verify_reset(void* varea, uint32_t n, hipStream_t s) {
    return hipMemsetAsync(varea, 0, (size_t)n * sizeof(VerifyRec), s);
}

// The slices of a chunk of D bytes, as both checksum passes cut them.
static bool verify_slices(u64 D, u32* slice_out, u32* nparts) {
    u64 slice = (D + CV_MAX_PARTS - 1) / CV_MAX_PARTS;
    slice = (slice + CV_TILE - 1) / CV_TILE * CV_TILE;
    if (slice < CV_MIN_SLICE) slice = CV_MIN_SLICE;
    if (slice > 0xFFFFFC00ull) return false;  // (D >= 2^32 is ZCG_ERR_UNSUPPORTED in the decoders)
    *slice_out = (u32)slice;
    *nparts = (u32)((D + slice - 1) / slice);
    return true;
}

hipError_t launch_crc32_verify(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, int32_t* d_status,
                               void* varea, hipStream_t s) {
    DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    if (n == 0 || D == 0) return hipSuccess;
    CrcArgs ca;
    if (!verify_slices(D, &ca.slice, &ca.nparts)) return hipErrorInvalidValue;
    const u64 slice = ca.slice;
    ca.xz = h_xpow8n(CV_TILE - 16);
    for (int k = 0; k < 6; k++) {
        ca.lm[k] = h_xpow8n(16ull << k);
        ca.pm[k] = h_xpow8n(slice << k);
    }
    ca.xlast = h_xpow8n(D - (u64)(ca.nparts - 1) * slice);
    ca.k = h_mulmod(h_xpow8n(D), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    const VerifyRec* rec = (const VerifyRec*)varea;
    u32* partials = (u32*)(verify_base((u8*)varea + verify_rec_bytes(n)));
    const u64 items = (u64)n * ((ca.nparts + 3) / 4);
    const u64 cap = (u64)device_cu_count() * CV_WG_PER_CU;
    hipLaunchKernelGGL(crc32_verify_kernel, dim3((u32)(items < cap ? items : cap)), dim3(CV_NT), 0, s, d_chunks, n, D,
                       t, ca, rec, partials);
    hipLaunchKernelGGL(crc32_fold_kernel, dim3(n), dim3(64), 0, s, n, ca, rec, (const u32*)partials, d_status);
    return hipGetLastError();
}

// Two launches, like the CRC pass: the slices' partials, then one wave per
// chunk that adds them (no atomics, no zeroed accumulators).
hipError_t launch_adler32_verify(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, int32_t* d_status,
                                 void* varea, hipStream_t s) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    if (n == 0 || D == 0) return hipSuccess;
    u32 slice = 0, nparts = 0;
    if (D >> 32 || !verify_slices(D, &slice, &nparts)) return hipErrorInvalidValue;
    const VerifyRec* rec = (const VerifyRec*)varea;
    u32* partials = (u32*)(verify_base((u8*)varea + verify_rec_bytes(n)));
    const u64 items = (u64)n * ((nparts + 3) / 4);
    const u64 cap = (u64)device_cu_count() * 8;  // (no LDS; 8 workgroups of 4 waves fill a CU)
    hipLaunchKernelGGL(adler32_verify_kernel, dim3((u32)(items < cap ? items : cap)), dim3(CV_NT), 0, s, d_chunks, n, D,
                       t, slice, nparts, rec, partials);
    hipLaunchKernelGGL(adler32_fold_kernel, dim3(n), dim3(64), 0, s, n, D, nparts, rec, (const u32*)partials, d_status);
    return hipGetLastError();
}

hipError_t launch_xxh32_verify(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, int32_t* d_status,
                               void* varea, hipStream_t s) {
    const DType t = make_dtype(a->dtype);
    const u64 D = a->chunk_num_elements * (u64)t.es;
    if (n == 0 || D == 0) return hipSuccess;
    hipLaunchKernelGGL(xxh32_verify_kernel, dim3((n + XV_CPW - 1) / XV_CPW), dim3(64), 0, s, d_chunks, n, D, t,
                       (const VerifyRec*)varea, d_status);
    return hipGetLastError();
}

}  // namespace zcg
