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
// the segmented coder (zcg_deflate_seg.hip): level 0 and ZCG_FLAG_GZIP_SEGMENTED
uint64_t deflate_seg_ws_bytes(u64 D, u32 n);
hipError_t launch_deflate_seg(const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n, u32 level,
                              uint64_t* d_out_len, int32_t* d_status, void* ws, uint64_t ws_bytes, hipStream_t s);
}  // namespace zcg
