// zcg_adler.h — Adler-32 (RFC 1950) as the GPU kernels compute it: the lane
// arithmetic of adler32_verify (zcg_verify.hip) and zlib_adler32
// (zcg_deflate.hip), their fold, and the deferred-modulo bound.  Compiles for
// host and device; tests/adler_host builds it with the host compiler alone.
//
// Over the D stream bytes d_0 .. d_{D-1}
//     A = 1 + sum d_i                 (mod 65521)
//     B = D + sum (D - i) * d_i       (mod 65521)
// and the checksum is B << 16 | A.  Neither sum depends on how the bytes are cut
// up, so a lane may take any 16-byte pieces and partial results add.
//
// A lane walks pieces that sit `stride` bytes apart (a comb through its slice).
// For the piece at stream position p, with s = sum d_j and w = sum (16 - j) d_j
// over its bytes j = 0..15,
//     sum (D - p - j) d_j = (D - p - 16) * s + w.
// Over a lane's pieces p_k = p_last - (n - 1 - k) * stride the first term is
//     E * S + stride * T,   E = D - p_last - 16,  S = sum s_k,  T = sum (n-1-k) s_k,
// and T is kept like Adler's own B: T += S before each piece's s joins S.  So a
// piece costs two dot-product chains and two additions, and nothing is reduced
// until the lane is done: adler_lane_close() takes the sums mod 65521.  Zero
// bytes add nothing to any sum, so a short slice is padded with virtual zero
// pieces wherever that is convenient; E may then be negative (a last piece
// that lies past D), which adler_lane_close() takes as it is.
//
// The deferred-modulo bound.  s <= 16 * 255 = 4080 and w <= 255 * (16+..+1) =
// 34680 per piece.  S is 32 bits wide, W and T are 64: after n pieces
//     S <= 4080 n,  W <= 34680 n,  T <= 4080 n (n - 1) / 2,
// so S is the register that can overflow first, at n > (2^32 - 1) / 4080 =
// 1 052 688 pieces (ADLER_LANE_MAX_PIECES, 16 843 008 bytes of 0xFF per lane);
// at that n, W < 2^36 and T < 2^52.  The kernels never get there: a verify slice
// is at most 2^32 / 64 bytes + one tile = 65 537 pieces per lane, an encoder
// chunk is below 2^31 bytes = 524 288 pieces per lane (static_asserts beside
// the kernels).  A caller that can go further closes the lane every
// ADLER_LANE_MAX_PIECES pieces and starts a new one (tests/adler_host does).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZA_INL __host__ __device__ inline
#else
#define ZA_INL inline
#endif

namespace zcg {

constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t ADLER_PIECE_MAX_S = 16u * 255u;
constexpr uint32_t ADLER_LANE_MAX_PIECES = 0xFFFFFFFFu / ADLER_PIECE_MAX_S;  // 1 052 688

// The unreduced sums of one lane.
struct AdlerLane {
    uint32_t S;
    uint64_t W, T;
};
ZA_INL AdlerLane adler_lane_open() { return AdlerLane{0u, 0ull, 0ull}; }

// sum of x's bytes times m's bytes, plus c
ZA_INL uint32_t adler_dot4(uint32_t x, uint32_t m, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(x, m, c, false);  // v_dot4_u32_u8
#else
    for (int i = 0; i < 4; i++) c += ((x >> (8 * i)) & 0xFFu) * ((m >> (8 * i)) & 0xFFu);
    return c;
#endif
}

// One 16-byte piece, its bytes in stream order in x0 (bytes 0-3, little
// endian) .. x3 (bytes 12-15).
ZA_INL void adler_lane_piece(AdlerLane& l, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    l.T += l.S;
    uint32_t s = l.S, w = 0;
    s = adler_dot4(x0, 0x01010101u, s);
    s = adler_dot4(x1, 0x01010101u, s);
    s = adler_dot4(x2, 0x01010101u, s);
    s = adler_dot4(x3, 0x01010101u, s);
    w = adler_dot4(x0, 0x0D0E0F10u, w);  // weights 16, 15, 14, 13
    w = adler_dot4(x1, 0x090A0B0Cu, w);
    w = adler_dot4(x2, 0x05060708u, w);
    w = adler_dot4(x3, 0x01020304u, w);
    l.S = s;
    l.W += w;
}

// A partial result: (sum d_i) mod 65521 in the low half, (sum (D - i) d_i) mod
// 65521 in the high half.  Partials of disjoint byte sets add (adler_add).
ZA_INL uint32_t adler_pack(uint32_t a, uint32_t b) { return a | (b << 16); }
ZA_INL uint32_t adler_add(uint32_t p, uint32_t q) {
    uint32_t a = (p & 0xFFFFu) + (q & 0xFFFFu), b = (p >> 16) + (q >> 16);
    if (a >= ADLER_MOD) a -= ADLER_MOD;
    if (b >= ADLER_MOD) b -= ADLER_MOD;
    return adler_pack(a, b);
}

// The lane's partial: E = D - (position of its last piece) - 16, its pieces
// `stride` bytes apart.
ZA_INL uint32_t adler_lane_close(const AdlerLane& l, int64_t E, uint32_t stride) {
    const uint64_t Em = (uint64_t)((E % (int64_t)ADLER_MOD + (int64_t)ADLER_MOD) % (int64_t)ADLER_MOD);
    const uint64_t Sm = l.S % ADLER_MOD;
    const uint64_t b = l.W % ADLER_MOD + Em * Sm + (uint64_t)(stride % ADLER_MOD) * (l.T % ADLER_MOD);
    return adler_pack((uint32_t)Sm, (uint32_t)(b % ADLER_MOD));
}

#if defined(__HIPCC__)
// The sum of the 64 lanes' partials, in every lane.
__device__ __forceinline__ uint32_t adler_wave_sum(uint32_t v) {
#pragma unroll
    for (int k = 0; k < 6; k++) v = adler_add(v, (uint32_t)__shfl_xor((int)v, 1 << k, 64));
    return v;
}
#endif

// The checksum of D bytes from the sum of all partials.
ZA_INL uint32_t adler_finish(uint32_t partial, uint64_t D) {
    return adler_add(partial, adler_pack(1u, (uint32_t)(D % ADLER_MOD)));
}

}  // namespace zcg
