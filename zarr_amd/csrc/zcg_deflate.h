// zcg_deflate.h — what the gzip encoder's two sources share: zcg_deflate.hip
// (dispatcher, zlib-exact coder, CRC32 kernel) and zcg_deflate_seg.hip.
#pragma once
#include "zcg_common.h"

namespace zcg {
constexpr u32 DF_HDR = 10;  // gzip member header bytes
#ifndef ZCG_DF_CHAIN6
#define ZCG_DF_CHAIN6 32  // the segmented coder's max_chain at level 6 (cfg_deflate reports it)
#endif
// gzip_crc32 (zcg_deflate.hip) over n chunks of D input bytes.  crc_out null:
// CRC32 + ISIZE into the trailer (at out_len - 8) of every chunk with status
// OK; else only the inputs' CRC32s, into crc_out[0..n).
hipError_t launch_gzip_crc32(const zcg_chunk* d_chunks, u32 n, u64 D, DType t, const u64* d_out_len,
                             const i32* d_status, u32* crc_out, hipStream_t s);
// The container both coders write around a deflate stream.  zhdr == 0: the
// gzip member (DF_HDR header bytes with XFL, CRC32 + ISIZE after the stream);
// else the zlib stream (RFC 1950): zhdr's two bytes, big-endian, in front and
// the Adler-32 after it.  zlib_header_word: 0 unless the array's codec is
// ZCG_CODEC_ZLIB.  launch_stream_checksum: launch_gzip_crc32 or its Adler-32
// counterpart (zlib_adler32; 4 big-endian bytes at out_len - 4), same modes.
u32 zlib_header_word(const zcg_array* a, u32 level);
hipError_t launch_stream_checksum(u32 zhdr, const zcg_chunk* d_chunks, u32 n, u64 D, DType t, const u64* d_out_len,
                                  const i32* d_status, u32* sum_out, hipStream_t s);
__device__ __forceinline__ u32 df_header_bytes(u32 zhdr) { return zhdr ? 2u : DF_HDR; }
__device__ __forceinline__ u32 df_trailer_bytes(u32 zhdr) { return zhdr ? 4u : 8u; }
__device__ __forceinline__ void df_put_header(u8* dst, u32 xfl, u32 zhdr) {  // (one thread)
    if (zhdr) {
        dst[0] = (u8)(zhdr >> 8);
        dst[1] = (u8)zhdr;
        return;
    }
    const u8 h[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, (u8)xfl, 255};
    for (u32 i = 0; i < 10; i++) dst[i] = h[i];
}
// the segmented coder (zcg_deflate_seg.hip): level 0 and ZCG_FLAG_GZIP_SEGMENTED
uint64_t deflate_seg_ws_bytes(u64 D, u32 n);
hipError_t launch_deflate_seg(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, u32 level,
                              uint64_t* d_out_len, int32_t* d_status, void* ws, uint64_t ws_bytes, hipStream_t s);
}  // namespace zcg
