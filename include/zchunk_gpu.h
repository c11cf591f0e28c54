/*
 * zchunk_gpu.h — C ABI of the MI355X (gfx950) Zarr chunk-codec path.
 *
 * This is the drop-in boundary for the reference's chunk codec path
 * (sci-rs/zarr v0.0.1).  Every entry point below replaces one piece of the
 * reference; the file:line it replaces is cited next to it.  All arguments
 * are plain pointers and sizes; no torch / HIP C++ types appear in the
 * signatures (`stream` is an opaque hipStream_t passed as void*).
 *
 * Reference interface being replaced (paths relative to the reference root):
 *   - trait Compression { decoder(R)->Box<dyn Read>; encoder(W)->Box<dyn Write> }
 *       src/compression/mod.rs:30-34, dispatch mod.rs:72-108
 *   - enum CompressionType {Raw, Bzip2, Gzip, Lz4, Xz}  src/compression/mod.rs:40-51
 *   - DefaultChunkReader::read_chunk / read_chunk_into   src/chunk.rs:270-301
 *   - DefaultChunkWriter::write_chunk                    src/chunk.rs:306-323
 *   - ReadableDataChunk::read_data (exact-N read, byte order, bool rule)
 *                                                        src/chunk.rs:103-116,163-222
 *   - WriteableDataChunk::write_data                     src/chunk.rs:118-140,169-237
 *
 * Semantics kept from the reference (see DESIGN.md "Parity contract"):
 *   - decode produces EXACTLY num_elements*elem_size bytes (read_exact,
 *     chunk.rs:112-113): a longer stream is truncated silently, a shorter one
 *     is ZCG_ERR_UNEXPECTED_EOF (tests.rs:191-219).
 *   - big-endian dtypes are byte-swapped per element (byteorder read_*_into);
 *     single-byte types and bool ignore endianness (data_type.rs:425-432).
 *   - bool: decoded byte != 0 -> 1 (chunk.rs:175-190).
 *   - encode requires the element count to equal product(chunk_shape)
 *     (chunk.rs:309-318) -> ZCG_ERR_INVALID_DATA otherwise.
 *   - only the first gzip member / LZ4 frame / xz stream / bzip2 stream is
 *     decoded (single-stream decoders of flate2/lz4-rs/xz2/bzip2).
 *
 * Threading: one zcg_ctx per device; a ctx is not shared across host threads
 * without external locking.  Work on distinct streams is independent.
 */
#ifndef ZCHUNK_GPU_H
#define ZCHUNK_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZCG_ABI_VERSION 1

/* CompressionType variants (src/compression/mod.rs:40-51).  Numbering is
 * this ABI's own; the JSON codec ids are mapped by the host layer. */
enum zcg_codec {
    ZCG_CODEC_RAW = 0,   /* raw.rs:13-24 */
    ZCG_CODEC_BZIP2 = 1, /* bzip.rs:16-46 */
    ZCG_CODEC_GZIP = 2,  /* gzip.rs:16-57 */
    ZCG_CODEC_LZ4 = 3,   /* lz.rs:45-93 */
    ZCG_CODEC_XZ = 4,    /* xz.rs:15-43 */
    ZCG_CODEC_ZLIB = 5   /* RFC 1950 (this library's own: the reference has no such variant): a 2-byte
                            header, the gzip codec's deflate body, a big-endian Adler-32 */
};

/* Per-chunk status words; map 1:1 onto std::io::ErrorKind of the reference. */
enum zcg_status {
    ZCG_OK = 0,
    ZCG_ERR_UNEXPECTED_EOF = 1, /* io::ErrorKind::UnexpectedEof (short stream) */
    ZCG_ERR_INVALID_DATA = 2,   /* corrupt stream / wrong element count        */
    ZCG_ERR_INVALID_INPUT = 3,  /* dtype mismatch (chunk.rs:261-264), bad args */
    ZCG_ERR_UNSUPPORTED = 4,    /* e.g. LZ4 dictionary frames                  */
    ZCG_ERR_OUTPUT_TOO_SMALL = 5, /* encode: dst capacity below the stream size */
    ZCG_ABSENT = 6,             /* store: no chunk file (get() -> Ok(None), read_chunk -> None) */
    ZCG_ERR_IO = 7,             /* store: a filesystem error (open/lock/read/write)  */
    ZCG_ERR_NOT_FOUND = 8,      /* store: key outside the hierarchy (io::ErrorKind::NotFound,
                                   filesystem.rs:180-186)                        */
    ZCG_ERR_RUNTIME = 100       /* HIP runtime failure (see zcg_last_error)     */
};

/* Decode flags (zcg_compression.flags).  The reference's read_exact never
 * reaches the gzip CRC32/ISIZE trailer or the LZ4 content checksum on a
 * full-length read, so neither is verified.  LZ4
 * block checksums are verified as LZ4F does, unless this flag skips them
 * (the decoded bytes are the same; only a corrupt checksum word changes the
 * status).
 *
 * Opt-in verification (decode only; encode ignores these flags, and a flag for
 * the other codec is ignored).  Every decode entry point honours them through
 * zcg_array.compression.flags: zcg_decode_batch, zcg_read_chunk,
 * zcg_read_chunks_host, zcg_store_read_chunks[_device], zcg_multi_*.
 *   - A chunk whose status without the flag is not ZCG_OK keeps exactly that
 *     status: verification runs only on chunks that decode OK.
 *   - A chunk of D == 0 decoded bytes is OK and nothing is verified (the
 *     reference reads zero bytes).
 *   - On a mismatch the decoded bytes stay in dst, untrusted (for bool arrays
 *     not normalised either); only the status says so.  Bytes after D are
 *     never touched.
 * For a chunk that decodes OK the verdict is the first rule that applies.
 * ZCG_FLAG_VERIFY_GZIP_TRAILER (D = N*elem_size decoded bytes):
 *   1. the member must end exactly at D bytes: after the output is full the
 *      rest of the deflate stream is walked with the whole input as its limit
 *      (not flate2's 32 KiB window): the EOB of the current block, empty
 *      stored blocks, block headers and tables, up to the final block's end;
 *   2. the output filled inside a match, the next token would emit a byte, or
 *      a non-empty stored block follows -> ZCG_ERR_INVALID_DATA (the member
 *      holds more than the chunk);
 *   3. an invalid header or code on the way -> ZCG_ERR_INVALID_DATA; input
 *      that runs out before the final block's end or before 8 trailer bytes
 *      -> ZCG_ERR_UNEXPECTED_EOF;
 *   4. the trailer sits at byte h + ceil(end_bit / 8) of the member (h = gzip
 *      header bytes, end_bit = deflate bits consumed); it is never taken from
 *      src_len - 8, and bytes after it (a second member) are ignored;
 *   5. ISIZE != D mod 2^32 -> ZCG_ERR_INVALID_DATA;
 *   6. CRC32 of the D decoded bytes in stream order (before the byte swap and
 *      the bool rule) != the trailer's -> ZCG_ERR_INVALID_DATA.
 * ZCG_FLAG_VERIFY_ZLIB_TRAILER (the zlib codec; the gzip and LZ4 flags are
 * ignored on it, and it is ignored on the other codecs):
 *   rules 1-4 of ZCG_FLAG_VERIFY_GZIP_TRAILER hold verbatim with h = 2 and a
 *   trailer of 4 bytes at byte 2 + ceil(end_bit / 8) (fewer than 4 bytes there
 *   -> ZCG_ERR_UNEXPECTED_EOF); there is no length word;
 *   5. Adler-32 of the D decoded bytes in stream order (before the byte swap
 *      and the bool rule) != the trailer read big-endian -> ZCG_ERR_INVALID_DATA.
 * The zlib header without any flag, as zlib's inflate() reads it: fewer than 2
 * bytes -> ZCG_ERR_UNEXPECTED_EOF; (b0 << 8 | b1) % 31 != 0, (b0 & 15) != 8 or
 * (b0 >> 4) > 7 -> ZCG_ERR_INVALID_DATA; FDICT (b1 & 0x20) -> ZCG_ERR_UNSUPPORTED
 * (a preset dictionary).  Any declared window of 8 to 15 bits is accepted and
 * distances are not checked against it (zlib does so only under
 * INFLATE_STRICT).  The body is then read exactly as the gzip codec reads it,
 * and without the flag the trailer is never read.
 * ZCG_FLAG_VERIFY_LZ4_CONTENT:
 *   1. the frame must end exactly at D bytes: the EndMark follows the block
 *      that reaches D; a further data block (or a block that decodes past D)
 *      -> ZCG_ERR_INVALID_DATA; input that ends before the EndMark, or before
 *      the 4 checksum bytes when FLG.C is set -> ZCG_ERR_UNEXPECTED_EOF;
 *   2. a content size in the header that differs from D -> ZCG_ERR_INVALID_DATA;
 *   3. FLG.C set and XXH32 (seed 0) of the D decoded bytes in stream order !=
 *      the stored word -> ZCG_ERR_INVALID_DATA.  With FLG.C clear there is
 *      nothing to compare and the chunk stays OK;
 *   4. linked-block frames and the other serially decoded frames obey the same
 *      rules. */
#define ZCG_FLAG_VERIFY_GZIP_TRAILER 0x1u
#define ZCG_FLAG_VERIFY_LZ4_CONTENT 0x2u
#define ZCG_FLAG_SKIP_LZ4_BLOCK_CHECKSUM 0x4u
#define ZCG_FLAG_VERIFY_ZLIB_TRAILER 0x8u
/* Use the wave-serial inflate kernel instead of the parallel one (the two are
 * bit-identical; the serial one is kept as a differential reference). */
#define ZCG_FLAG_SERIAL_INFLATE 0x100u
/* Accumulate internal kernel statistics (development builds / profiling; the
 * default build compiles the inflate wave kernel's counters out, so there the
 * flag changes nothing). */
#define ZCG_FLAG_DEBUG_COUNTERS 0x200u
/* Xz decode keeps 32 KiB of history in LDS instead of 4 KiB: far matches
 * stop re-reading the output from L2/HBM, at 3 instead of 8 chunks per CU. */
#define ZCG_FLAG_XZ_RING_32K 0x400u
/* LZ4 block decoder choice (bit-identical): one wave per block (speculative
 * parse, byte-parallel resolve) or one lane per block; by default the batch
 * size picks: waves below 131 072 blocks, both side by side (on a second
 * stream) below 196 608, lanes from there. */
#define ZCG_FLAG_LZ4_WAVE_PER_BLOCK 0x800u
#define ZCG_FLAG_LZ4_LANE_PER_BLOCK 0x1000u
/* Gzip and zlib decode kernel choice (all bit-identical).  By default a batch of at
 * most 3 chunks per CU (one generation of the 256-lane kernel) runs the
 * 256-lane round kernel (fine 256-bit segments, one workgroup of 4 waves per
 * chunk: half the latency of a lone chunk), a larger one the one-wave-per-chunk
 * kernel (coarse segments, 16 chunks per CU).  These flags force one. */
#define ZCG_FLAG_INFLATE_BLOCK_PAR 0x2000u
#define ZCG_FLAG_INFLATE_WAVE 0x4000u
/* Gzip encode at levels 1-9 is byte-identical to zlib 1.2.11 / flate2
 * (gzip.rs:54-56) by default (deflate_fast for 1-3, deflate_slow for 4-9), and
 * zlib encode to zlib 1.2.11's compress2() (header 78 01 at levels 0-1, 78 5E
 * at 2-5, 78 9C at 6, 78 DA at 7-9).
 * This flag selects the faster segmented coder instead (16 KiB blocks, each
 * ended by an empty stored block; the stream inflates to the same data, but
 * its bytes differ from zlib's).  Level 0 always uses the segmented coder. */
#define ZCG_FLAG_GZIP_SEGMENTED 0x8000u
/* Test hook: the one-wave-per-chunk inflate kernel sizes its first segments
 * at 116 % instead of 108 % of the estimated block bits, which makes the
 * first round of all-literal 16 383-symbol blocks cap a list and halve the
 * segment size (the round-6 regression test of that path).  Same output. */
#define ZCG_FLAG_DEBUG_INFLATE_LONG_SEG 0x10000u

/* CompressionType + its configuration (camelCase JSON keys in the reference). */
typedef struct zcg_compression {
    int32_t codec;            /* enum zcg_codec                                 */
    int32_t gzip_level;       /* deflate level of the GZIP and ZLIB codecs:
                                 gzip.rs:16-20, -1 / out of [0,9] -> 6 (28-34)  */
    int32_t lz4_block_size;   /* lz.rs:45-50, rounded to 64K/256K/1M/4M (55-65) */
    int32_t bzip2_block_size; /* bzip.rs:16-21, 1..9                            */
    int32_t xz_preset;        /* xz.rs:15-20                                    */
    uint32_t flags;           /* ZCG_FLAG_*                                     */
} zcg_compression;

/* Effective element type (data_type.rs:417-432). */
typedef struct zcg_dtype {
    uint8_t elem_size;  /* 1, 2, 4 or 8 */
    uint8_t big_endian; /* 1 for '>' types of size > 1 */
    uint8_t is_bool;    /* 1 for "bool" */
    uint8_t reserved;
} zcg_dtype;

/* What one batch shares: the array's codec, dtype and chunk element count
 * (ArrayMetadata, lib.rs:382-402; get_chunk_num_elements lib.rs:474-480). */
typedef struct zcg_array {
    zcg_compression compression;
    zcg_dtype dtype;
    uint64_t chunk_num_elements;
} zcg_array;

/* One chunk of a batch.  All pointers are DEVICE pointers, caller-owned.
 *  decode: src = compressed stream (src_len bytes), dst = N*elem_size bytes
 *  encode: src = N*elem_size bytes of native (little-endian) elements,
 *          dst = output buffer of capacity dst_cap bytes                  */
typedef struct zcg_chunk {
    const void* src;
    uint64_t src_len;
    void* dst;
    uint64_t dst_cap;
} zcg_chunk;

typedef struct zcg_ctx zcg_ctx;

/* ---- context -------------------------------------------------------- */
int zcg_abi_version(void);
/* The kernels' tuning constants this library was built with, as
 * "kernel:K=V,...;kernel:K=V,..." (A/B builds under tools/ change them; the
 * product build uses the defaults, which tests/test_abi.py checks). */
const char* zcg_build_config(void);
zcg_ctx* zcg_create(int device);
void zcg_destroy(zcg_ctx* ctx);
const char* zcg_last_error(const zcg_ctx* ctx);
/* Effective parameters the reference would use (gzip.rs:28-34, lz.rs:55-65). */
int32_t zcg_effective_gzip_level(int32_t level);
int32_t zcg_effective_lz4_block_size(int32_t block_size);
int zcg_codec_on_gpu(int32_t codec, int encode);

/* ---- device-resident batch API (the hot path) ------------------------
 * Replaces N calls of DefaultChunk::read_chunk_into (chunk.rs:288-301) with
 * one batched, stream-ordered launch sequence.  `d_chunks` and `d_status`
 * are device arrays of n entries.  Asynchronous on `stream`; returns a
 * zcg_status for argument/launch errors only — per-chunk results land in
 * d_status.  Workspace is grown on first use of a given batch shape
 * (hipMalloc), so steady-state calls do no allocation and are capturable.
 * The workspace is kept per stream (gzip decode: ~0.9 GB at full batch,
 * zcg_workspace_bytes gives the figure); a context keeps at most 4 streams'
 * workspaces and frees the least recently used one (after a device-wide
 * synchronize) when a fifth stream arrives. */
int zcg_decode_batch(zcg_ctx* ctx, const zcg_array* array, const zcg_chunk* d_chunks,
                     uint32_t n, int32_t* d_status, void* stream);

/* Replaces N calls of DefaultChunk::write_chunk (chunk.rs:306-323).
 * d_out_len[i] receives the encoded stream length of chunk i.  LZ4 encode
 * accepts at most 4096 LZ4 blocks per chunk (256 MiB at the 64 KiB default
 * block size); beyond that it returns ZCG_ERR_UNSUPPORTED (zcg_last_error
 * says why) and launches nothing. */
int zcg_encode_batch(zcg_ctx* ctx, const zcg_array* array, const zcg_chunk* d_chunks,
                     uint32_t n, uint64_t* d_out_len, int32_t* d_status, void* stream);

/* Upper bound of an encoded chunk of `src_len` bytes for this codec. */
uint64_t zcg_encode_bound(const zcg_compression* c, uint64_t src_len);

/* Bytes of device workspace a batch of this shape needs (informational). */
uint64_t zcg_workspace_bytes(const zcg_array* array, uint32_t n, int encode);

/* ---- host-memory conveniences (one read_chunk / write_chunk) ---------
 * zcg_read_chunk == DefaultChunkReader::read_chunk body (chunk.rs:270-286)
 * on host buffers: H2D of the stream, GPU decode, D2H of the elements.
 * `dst` receives N*elem_size bytes (host-native order). */
int zcg_read_chunk(zcg_ctx* ctx, const zcg_array* array, const void* src, uint64_t src_len,
                   void* dst);
/* zcg_write_chunk == DefaultChunkWriter::write_chunk (chunk.rs:306-323):
 * `n_elements` must equal array->chunk_num_elements (else INVALID_DATA). */
int zcg_write_chunk(zcg_ctx* ctx, const zcg_array* array, const void* elems,
                    uint64_t n_elements, void* out, uint64_t out_cap, uint64_t* out_len);

/* Host-resident batch (e2e path): pinned staging, H2D, decode, D2H.
 * srcs/src_lens/dsts/status are host arrays of n entries. */
int zcg_read_chunks_host(zcg_ctx* ctx, const zcg_array* array, uint32_t n,
                         const void* const* srcs, const uint64_t* src_lens, void* const* dsts,
                         int32_t* status);

/* ---- region assembly ----------------------------
 * Replaces ZarrNdarrayReader::read_ndarray / read_ndarray_into_with_buffer
 * (ndarray.rs:153-268): decoded chunks that already sit in HBM are
 * scattered into one bounding box on the device.  Chunk order is the
 * array's memory layout (ndarray.rs:453-462: ColumnMajor -> dim 0 fastest,
 * RowMajor -> last dim fastest); the output is any strided view of
 * bbox_shape (out_strides in elements, ndarray's ArrayViewMut).  Edge chunks
 * overhang the array and are read over their full nominal extent
 * (get_chunk_bounds, ndarray.rs:434-446); chunks are the ones
 * bounded_coord_iter visits (ndarray.rs:410-432). */
#define ZCG_MAX_DIMS 8
typedef struct zcg_region {
    uint32_t ndim;         /* 1..ZCG_MAX_DIMS                                   */
    uint32_t elem_size;    /* 1, 2, 4, 8 (decoded, host-native element bytes)    */
    uint32_t chunk_order;  /* 0 = RowMajor (C), 1 = ColumnMajor (F), lib.rs Order */
    uint32_t fill_missing; /* 1: read_ndarray — every element no chunk covers gets
                              fill_value (Array::from_elem, ndarray.rs:164-171);
                              0: read_ndarray_into — such elements are untouched */
    uint64_t array_shape[ZCG_MAX_DIMS];
    uint64_t chunk_shape[ZCG_MAX_DIMS];
    uint64_t bbox_offset[ZCG_MAX_DIMS];
    uint64_t bbox_shape[ZCG_MAX_DIMS];
    int64_t out_strides[ZCG_MAX_DIMS]; /* per array dim, in elements */
    uint64_t fill_value;   /* elem_size low bytes, host order (get_effective_fill_value) */
} zcg_region;

/* The chunk grid range a region reads: grid_lo[d] .. grid_lo[d]+grid_n[d]
 * (bounded_coord_iter, ndarray.rs:410-432).  Returns the number of chunks
 * (0 when the box misses the array). */
uint64_t zcg_region_grid(const zcg_region* r, uint64_t* grid_lo, uint64_t* grid_n);

/* d_chunk_table: device array of zcg_region_grid() DEVICE pointers to the
 * decoded chunks (N*elem_size bytes each), C order over the grid range
 * (dim 0 slowest); NULL = chunk absent (read_chunk -> Ok(None)).  d_out is
 * the base of the output view.  Asynchronous on `stream`. */
int zcg_read_region(zcg_ctx* ctx, const zcg_region* r, const void* const* d_chunk_table,
                    void* d_out, void* stream);

/* The inverse scatter of ZarrNdarrayWriter::write_ndarray (ndarray.rs:276-385):
 * the box (d_in, a strided view of bbox_shape) is written into the chunk
 * slots of d_chunk_table (same grid range and order as zcg_read_region; every
 * element of the box that falls in a non-NULL chunk is written, at its
 * chunk-local position in the chunk memory order).  The caller pre-fills
 * slots of partially covered chunks with the existing chunk (or fill value)
 * and encodes the slots afterwards (zcg_encode_batch).  fill_missing is
 * ignored.  Asynchronous on `stream`. */
int zcg_write_region(zcg_ctx* ctx, const zcg_region* r, void* const* d_chunk_table,
                     const void* d_in, void* stream);

/* ---- many bounding boxes in one call ----------------------------------
 * The reference's users read many small boxes from one array (tiles, patches,
 * random crops), one read_ndarray each.  zcg_read_regions assembles n_boxes
 * boxes of one common shape in one launch: each box has its own offset and its
 * own output view, all read one shared chunk table. */
typedef struct zcg_box {
    uint64_t offset[ZCG_MAX_DIMS]; /* bbox_offset of this box, per array dim   */
    void* out;                     /* DEVICE base (element (0,..,0)) of its view */
} zcg_box;

/* Union of the boxes' zcg_region_grid ranges: the smallest grid range
 * lo[d] .. lo[d]+n[d] that holds every chunk some box visits (r->bbox_offset
 * is ignored; `offsets` is a host array of n_boxes*ndim, box-major; lo and n
 * are host arrays of ndim).  Returns the number of table entries (product of
 * n); 0, with lo = n = 0, if no box visits a chunk. */
uint64_t zcg_regions_grid(const zcg_region* r, const uint64_t* offsets, uint32_t n_boxes,
                          uint64_t* lo, uint64_t* n);

/* `r` gives ndim, elem_size, chunk_order, fill_missing, array_shape,
 * chunk_shape, bbox_shape, out_strides and fill_value for every box;
 * r->bbox_offset is ignored.  d_chunk_table covers the grid range
 * table_lo[d] .. table_lo[d]+table_n[d] (host arrays of ndim), C order with
 * dim 0 slowest, NULL = chunk absent: zcg_read_region's convention.  d_boxes
 * and d_status are DEVICE arrays of n_boxes entries.
 *  - Per-box equivalence: for every box whose status is ZCG_OK the bytes
 *    written to its view are exactly those zcg_read_region writes for a
 *    zcg_region with that bbox_offset and a table holding the same pointers
 *    over that box's own zcg_region_grid range: clipping to array_shape,
 *    overhanging edge chunks, fill versus untouched.  A chunk inside the table
 *    but outside the box's own grid range is never read.
 *  - A box whose own grid range is not inside the table's range gets
 *    ZCG_ERR_INVALID_INPUT; nothing of it is written, and the other boxes are
 *    unaffected.
 *  - A box that visits no chunk is ZCG_OK, and filled when fill_missing is set.
 *  - n_boxes == 0, or a zero extent in bbox_shape, returns ZCG_OK and launches
 *    nothing (d_status is not written).
 *  - bbox_shape[d] + chunk_shape[d] - 1 >= 2^32 returns ZCG_ERR_UNSUPPORTED
 *    (the single-box limit, for any offset).
 *  - Asynchronous on `stream`; the number of launches does not depend on
 *    n_boxes; the call allocates nothing and does not synchronize with the
 *    host.  d_boxes is read when the kernel runs, so the call can be captured
 *    in a graph and a replay sees new offsets and outputs.
 *  - Output views of different boxes that overlap are the caller's business. */
int zcg_read_regions(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                     const void* const* d_chunk_table, const zcg_box* d_boxes, uint32_t n_boxes,
                     int32_t* d_status, void* stream);

/* The inverse of zcg_read_regions, ZarrNdarrayWriter::write_ndarray's scatter
 * (ndarray.rs:276-385) for n_boxes boxes of one shape in one launch.  The
 * arguments are zcg_read_regions', except that zcg_box.out is the DEVICE base
 * of the box's INPUT view (r->out_strides: its strides per array dim, in
 * elements), which is only read, and that fill_missing and fill_value are
 * ignored.
 *  - Per-box equivalence: for every box whose status is ZCG_OK the bytes
 *    written to the chunk slots are exactly those zcg_write_region writes for
 *    a zcg_region with that bbox_offset and a table holding the same pointers
 *    over that box's own zcg_region_grid range: every element of the box that
 *    falls in a visited, non-NULL chunk is written, the overhang of edge
 *    chunks beyond array_shape included; elements in chunks the box does not
 *    visit are dropped; NULL entries are skipped.  A chunk inside the table
 *    but outside the box's own grid range is never touched.
 *  - A box whose own grid range is not inside the table's range gets
 *    ZCG_ERR_INVALID_INPUT; nothing of it is written, and the other boxes are
 *    unaffected.
 *  - A box that visits no chunk is ZCG_OK and writes nothing.
 *  - n_boxes == 0, or a zero extent in bbox_shape, returns ZCG_OK and launches
 *    nothing (d_status is not written).
 *  - bbox_shape[d] + chunk_shape[d] - 1 >= 2^32 returns ZCG_ERR_UNSUPPORTED.
 *  - Overlapping boxes: two boxes of one call may write the same chunk
 *    element.  It ends up with one of their values, whole (elements are at
 *    most 8 bytes and naturally aligned); which box wins is unspecified.
 *    Callers who need "the later box wins" split the call with
 *    zcg_regions_waves and launch the waves in order on one stream.
 *  - Asynchronous on `stream`; the number of launches does not depend on
 *    n_boxes; the call allocates nothing and does not synchronize with the
 *    host.  d_boxes is read when the kernel runs, so the call can be captured
 *    in a graph and a replay sees new offsets and inputs. */
int zcg_write_regions(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                      void* const* d_chunk_table, const zcg_box* d_boxes, uint32_t n_boxes,
                      int32_t* d_status, void* stream);

/* A greedy split of a box list into consecutive runs ("waves") of pairwise
 * disjoint boxes; host code, no GPU and no context.  `r` gives ndim,
 * bbox_shape and chunk_shape; `offsets` is a host array of n_boxes*ndim,
 * box-major; wave_of (n_boxes entries) receives each box's wave.  Box 0 is in
 * wave 0; box b opens a new wave if and only if its extent intersects the
 * extent of a box already in the current wave.  The extent is offsets[b] ..
 * offsets[b] + bbox_shape, not clipped to the array, ends saturating at
 * 2^64-1; two extents intersect when they share at least one element in every
 * dimension.  wave_of is non-decreasing; the return value is the number of
 * waves, 0 for n_boxes == 0.  With a zero extent in bbox_shape nothing
 * intersects: one wave.  zcg_write_regions calls for the waves, in order on
 * one stream, leave every shared element with the later box's value.  The
 * cost is linear in n_boxes for disjoint boxes (a box is compared only with
 * boxes that share a chunk-aligned cell with it). */
uint32_t zcg_regions_waves(const zcg_region* r, const uint64_t* offsets, uint32_t n_boxes, uint32_t* wave_of);

/* ---- many bounding boxes of differing shapes in one call ----------------
 * The reference's read_ndarray / write_ndarray (ndarray.rs:153-385) take any
 * BoundingBox per call: object or segment bounding boxes, detections, halo
 * reads whose extent depends on the position, multi-scale crops.  The _v calls
 * are zcg_read_regions / zcg_write_regions with a shape and a view per box. */
typedef struct zcg_vbox {
    uint64_t offset[ZCG_MAX_DIMS];   /* bbox_offset, per array dim                */
    uint64_t shape[ZCG_MAX_DIMS];    /* this box's bbox_shape, per array dim      */
    int64_t  strides[ZCG_MAX_DIMS];  /* its view's strides per array dim, elements */
    void*    base;                   /* DEVICE element (0,..,0) of its view       */
} zcg_vbox;

/* zcg_regions_grid and zcg_regions_waves with a shape per box: `shapes` is a
 * host array of n_boxes*ndim, box-major, as `offsets` is; r->bbox_shape is the
 * bound of the _v calls (no box is expected to exceed it) and r->bbox_offset
 * is ignored.  Host code, no GPU and no context.
 *  - zcg_regions_v_grid: the union of the boxes' own zcg_region_grid ranges;
 *    the return value and lo / n are zcg_regions_grid's.
 *  - zcg_regions_v_waves: the waves are defined exactly as zcg_regions_waves'
 *    (greedy and consecutive: box b opens a new wave if and only if its
 *    unclipped extent offsets[b] .. offsets[b] + shapes[b], ends saturating,
 *    intersects the extent of a box of the current wave); a box with a zero
 *    extent intersects nothing.  With one shape repeated the result is
 *    zcg_regions_waves'.  Boxes are hashed into cells whose extent is the
 *    smallest multiple of the chunk extent that holds r->bbox_shape (or the
 *    largest box, should one exceed it), so every box lies in at most two
 *    cells per dimension.  The cost is linear in n_boxes for disjoint boxes of
 *    similar size; it degrades towards quadratic when many small boxes share
 *    one large cell (one large box sets the cell extent for all). */
uint64_t zcg_regions_v_grid (const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                             uint32_t n_boxes, uint64_t* lo, uint64_t* n);
uint32_t zcg_regions_v_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                             uint32_t n_boxes, uint32_t* wave_of);

/* Bytes of DEVICE working memory a _v call with n_boxes boxes needs
 * (d_scratch, 8-byte aligned); monotonic in n_boxes. */
uint64_t zcg_regions_v_scratch_bytes(uint32_t n_boxes);

/* `r` gives ndim, elem_size, chunk_order, fill_missing, fill_value,
 * array_shape and chunk_shape for every box.  r->bbox_shape[d] is the LARGEST
 * EXTENT ANY BOX OF THE CALL MAY HAVE along dimension d: the host checks it
 * and sizes the launch from it without reading device memory.  r->bbox_offset
 * and r->out_strides are ignored.  The table arguments are zcg_read_regions'.
 * d_boxes (zcg_vbox) and d_status are DEVICE arrays of n_boxes entries;
 * zcg_vbox.base is the box's output view for zcg_read_regions_v and its input
 * view, which is only read, for zcg_write_regions_v (which also ignores
 * fill_missing and fill_value).
 *  - Per-box equivalence: for every box whose status is ZCG_OK the bytes
 *    written are exactly those zcg_read_region (zcg_write_region) writes for a
 *    zcg_region with that box's offset, shape and strides and a table holding
 *    the same pointers over that box's own zcg_region_grid range: clipping to
 *    array_shape, overhanging edge chunks, fill versus untouched, NULL entries.
 *    A chunk inside the table but outside the box's own grid range is never
 *    touched.
 *  - A box with shape[d] > r->bbox_shape[d] for some d gets
 *    ZCG_ERR_INVALID_INPUT; nothing of it is written, and the other boxes are
 *    unaffected.  The same holds for a box whose own grid range is not inside
 *    the table's range.
 *  - A box with a zero extent is ZCG_OK and writes nothing.  A box that visits
 *    no chunk is ZCG_OK, and filled on the read side when fill_missing is set.
 *  - Every box's status word is written, also for boxes that have no work.
 *  - r->bbox_shape[d] + chunk_shape[d] - 1 >= 2^32 returns
 *    ZCG_ERR_UNSUPPORTED; so does n_boxes x the bound's elements >= 2^62.
 *  - n_boxes == 0 returns ZCG_OK and launches nothing.
 *  - Asynchronous on `stream`: two launches (a plan kernel that checks every
 *    box and writes the status words and a prefix sum of work units into
 *    d_scratch, and the walk), whatever n_boxes and the shapes are.  The call
 *    allocates nothing and does not synchronize with the host; its only
 *    working memory is d_scratch (zcg_regions_v_scratch_bytes(n_boxes) bytes),
 *    which may be reused once the call's kernels have run.  d_boxes is read
 *    when the kernels run, so the call can be captured in a graph and a replay
 *    sees new offsets, SHAPES, strides and bases, as long as the shapes stay
 *    inside the bound.  Work follows the sum of the boxes' sizes, not
 *    n_boxes x the bound.
 *  - Overlapping boxes on the write side: zcg_write_regions' rule.  An element
 *    ends up with one of the values, whole; which box wins is unspecified.
 *    Callers who need "the later box wins" split the call with
 *    zcg_regions_v_waves and launch the waves in order on one stream (each
 *    with its own part of d_status; d_scratch may be shared).
 *  - Output views of different boxes that overlap are the caller's business. */
int zcg_read_regions_v (zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        const void* const* d_chunk_table, const zcg_vbox* d_boxes, uint32_t n_boxes,
                        void* d_scratch, int32_t* d_status, void* stream);
int zcg_write_regions_v(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        void* const* d_chunk_table, const zcg_vbox* d_boxes, uint32_t n_boxes,
                        void* d_scratch, int32_t* d_status, void* stream);

/* ---- many bounding boxes with a step per dimension in one call ------------
 * The reference's slices hard-code step 1 (to_ndarray_slice, ndarray.rs:118-127):
 * a caller who wants every k-th element (a preview, a pyramid level, a
 * subsampled crop) reads the dense box and slices it.  zcg_read_regions_s is
 * zcg_read_regions_v with a step per box and dimension: shape[d] is the number
 * of SAMPLES, sample i along d is array index offset[d] + i*step[d], and the
 * view holds the samples only.  The box's HULL is the dense box offset[d] ..
 * offset[d] + (shape[d]-1)*step[d] + 1 per dimension (empty when a shape[d] is
 * 0).  zcg_write_regions_s is the inverse: the view's samples go to those
 * array indices and nothing between them is written.  There is no negative
 * step. */
typedef struct zcg_sbox {
    uint64_t offset[ZCG_MAX_DIMS];   /* first sample, per array dim               */
    uint64_t shape[ZCG_MAX_DIMS];    /* samples per array dim                     */
    uint64_t step[ZCG_MAX_DIMS];     /* >= 1, array elements between two samples  */
    int64_t  strides[ZCG_MAX_DIMS];  /* its view's strides per array dim, elements */
    void*    base;                   /* DEVICE element (0,..,0) of its view       */
} zcg_sbox;

/* Host code, no GPU and no context.  `r` gives ndim, array_shape and
 * chunk_shape; r->bbox_offset and r->bbox_shape are ignored.
 *  - zcg_region_s_chunks, for one box (offset, shape, step: host arrays of
 *    ndim): lo / n receive the hull's zcg_region_grid range; `touched`, when
 *    not NULL, receives n[0] + n[1] + ... + n[ndim-1] bytes, dimension-major,
 *    byte j of dimension d being 1 where grid index lo[d] + j holds a sample
 *    (a sample's array index lies in that chunk's nominal bounds), else 0.
 *    The chunks a strided read TOUCHES are the product of these per-dimension
 *    sets; the return value is their number: the product over d of the touched
 *    counts, 0 when the box misses the array (lo, n and touched are still
 *    filled per dimension).  A step of 0, which the read calls refuse,
 *    returns 0 with lo = n = 0 and writes no byte of `touched`.
 *  - zcg_regions_s_grid: the union of the boxes' hulls' zcg_region_grid ranges
 *    (`offsets`, `shapes`, `steps`: host arrays of n_boxes*ndim, box-major);
 *    the return value and lo / n are zcg_regions_v_grid's.  A box with a step
 *    of 0 (which the read call refuses) adds nothing.
 *  - zcg_regions_s_scratch_bytes: bytes of DEVICE working memory a call with
 *    n_boxes boxes needs (d_scratch, 8-byte aligned); monotonic in n_boxes. */
uint64_t zcg_region_s_chunks(const zcg_region* r, const uint64_t* offset, const uint64_t* shape,
                             const uint64_t* step, uint64_t* lo, uint64_t* n, uint8_t* touched);
uint64_t zcg_regions_s_grid(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                            const uint64_t* steps, uint32_t n_boxes, uint64_t* lo, uint64_t* n);
uint64_t zcg_regions_s_scratch_bytes(uint32_t n_boxes);

/* `r` gives ndim, elem_size, chunk_order, fill_missing, fill_value,
 * array_shape and chunk_shape for every box.  r->bbox_shape[d] is the LARGEST
 * SAMPLE COUNT ANY BOX OF THE CALL MAY HAVE along dimension d: the host checks
 * it and sizes the launch from it without reading device memory.
 * r->bbox_offset and r->out_strides are ignored.  The table arguments are
 * zcg_read_regions'.  d_boxes (zcg_sbox) and d_status are DEVICE arrays of
 * n_boxes entries; zcg_sbox.base is the box's output view.
 *  - Per-box equivalence: for every box whose status is ZCG_OK, element i of
 *    its view (per dimension) receives exactly what zcg_read_region writes to
 *    element i*step of a dense view of the box's hull, for a zcg_region with
 *    the hull's offset and shape and a table holding the same pointers over
 *    the hull's own zcg_region_grid range: clipping to array_shape,
 *    overhanging edge chunks read over their nominal extent, fill versus
 *    untouched, NULL entries.  Only the sampled elements of the view are ever
 *    written.
 *  - Touched chunks: a chunk is touched when at least one sample's array index
 *    lies in its nominal bounds and the chunk is inside the hull's
 *    zcg_region_grid range (zcg_region_s_chunks).  A chunk inside the hull's
 *    range that holds no sample is never read: its table entry is never
 *    dereferenced and may hold anything.  A chunk inside the table but
 *    outside the hull's range is never touched either.
 *  - A box with shape[d] > r->bbox_shape[d] for some d, or with step[d] == 0,
 *    gets ZCG_ERR_INVALID_INPUT; a box whose hull extent plus
 *    chunk_shape[d] - 1 reaches 2^32 along some d (positions are 32-bit) gets
 *    ZCG_ERR_UNSUPPORTED; a box whose hull's grid range is not inside the
 *    table's range gets ZCG_ERR_INVALID_INPUT.  Nothing of such a box is
 *    written, and the other boxes are unaffected.
 *  - A box with a zero extent is ZCG_OK and writes nothing.  A box that visits
 *    no chunk is ZCG_OK, and filled when fill_missing is set.
 *  - Every box's status word is written, also for boxes that have no work.
 *  - r->bbox_shape[d] + chunk_shape[d] - 1 >= 2^32 returns
 *    ZCG_ERR_UNSUPPORTED; so does n_boxes x the bound's elements >= 2^62.
 *  - n_boxes == 0 returns ZCG_OK and launches nothing.
 *  - Asynchronous on `stream`: two launches (a plan kernel that checks every
 *    box and writes the status words and a prefix sum of work units into
 *    d_scratch, and the walk), whatever n_boxes, the sample counts and the
 *    steps are.  The call allocates nothing and does not synchronize with the
 *    host; its only working memory is d_scratch
 *    (zcg_regions_s_scratch_bytes(n_boxes) bytes), which may be reused once the
 *    call's kernels have run.  d_boxes is read when the kernels run, so the
 *    call can be captured in a graph and a replay sees new offsets, sample
 *    counts, STEPS, strides and bases, as long as the counts stay inside the
 *    bound.  Work follows the sum of the boxes' SAMPLES, not their hulls.
 *  - Output views of different boxes that overlap are the caller's business. */
int zcg_read_regions_s(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                       const void* const* d_chunk_table, const zcg_sbox* d_boxes, uint32_t n_boxes,
                       void* d_scratch, int32_t* d_status, void* stream);

/* The strided scatter.  The arguments are zcg_read_regions_s' (r->bbox_shape
 * bounds the SAMPLE COUNTS; d_scratch is zcg_regions_s_scratch_bytes(n_boxes)
 * bytes), with two differences: zcg_sbox.base is the box's INPUT view, which
 * is only read, and fill_missing and fill_value are ignored.
 *  - Per box: sample i of the view (per dimension) goes to array index
 *    offset + i*step.  For a box whose status is ZCG_OK every sample is written
 *    whole at its chunk-local position, in the chunk's memory order, if its
 *    array index lies in a chunk that is touched (zcg_region_s_chunks), inside
 *    the hull's zcg_region_grid range, and not NULL in the table.  The overhang
 *    of an edge chunk beyond array_shape is written; a sample beyond the hull's
 *    grid range (the hull is clipped to array_shape) is dropped.
 *  - No other byte of any slot is written: not the bytes of a u8 array between
 *    two samples at step 2, not the 8 bytes next to a written u64.  No store is
 *    wider than an element unless every byte it covers is a sample's.
 *  - A chunk that is untouched, or outside the box's hull range, is never
 *    dereferenced: its table entry may hold anything.
 *  - Equivalently: the slots end up as after zcg_read_region of the hull into
 *    a scratch array, scratch[::step] = view, and zcg_write_region of the hull,
 *    restricted to touched chunks whose entry is not NULL.
 *  - Status words are zcg_read_regions_s': a box with shape[d] >
 *    r->bbox_shape[d] or step[d] == 0 gets ZCG_ERR_INVALID_INPUT; a hull extent
 *    plus chunk_shape[d] - 1 that reaches 2^32 gets ZCG_ERR_UNSUPPORTED; a hull
 *    whose grid range is not inside the table's range gets
 *    ZCG_ERR_INVALID_INPUT.  Nothing of such a box is written, and the other
 *    boxes are unaffected.  Every box's status word is written.
 *  - A box with a zero extent, or one that visits no chunk, is ZCG_OK and
 *    writes nothing.
 *  - The call-level returns are zcg_read_regions_s': r->bbox_shape[d] +
 *    chunk_shape[d] - 1 >= 2^32 and n_boxes x the bound's elements >= 2^62
 *    return ZCG_ERR_UNSUPPORTED; n_boxes == 0 returns ZCG_OK and launches
 *    nothing.
 *  - Asynchronous on `stream`: two launches whatever the boxes (the plan, and
 *    the walk), no allocation, no synchronization with the host.  d_boxes is
 *    read when the kernels run, so a captured graph replays with new offsets,
 *    sample counts, STEPS, strides and bases inside the bound.  Work follows
 *    the sum of the boxes' SAMPLES, not their hulls.
 *  - Overlapping boxes: zcg_write_regions' rule.  A sample two boxes share ends
 *    up with one of the values, whole; which box wins is unspecified.  Callers
 *    who need "the later box wins" split the call with zcg_regions_s_waves and
 *    launch the waves in order on one stream (each with its own part of
 *    d_status; d_scratch may be shared). */
int zcg_write_regions_s(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        void* const* d_chunk_table, const zcg_sbox* d_boxes, uint32_t n_boxes,
                        void* d_scratch, int32_t* d_status, void* stream);

/* zcg_regions_v_waves for strided boxes (`shapes`: sample counts, `steps`:
 * n_boxes*ndim, box-major); host code, no GPU and no context.  Greedy and
 * consecutive, exactly as zcg_regions_v_waves: box b opens a new wave if and
 * only if it intersects a box of the current wave.
 *  - Two strided boxes intersect if and only if, in every dimension, the
 *    progressions {o1 + i*s1, i < c1} and {o2 + j*s2, j < c2} share an index.
 *    The test is exact (o2 - o1 divisible by gcd(s1, s2), and the least common
 *    index at or above max(o1, o2) not past either last sample), done as a
 *    congruence in 128-bit arithmetic without a loop over samples.  Even and
 *    odd planes of one hull therefore land in ONE wave.
 *  - If a hull end (offset + (count-1)*step + 1) of either box passes 2^64-1
 *    along some dimension, the pair is compared by the interval test of the
 *    hulls with saturated ends instead: conservative, and still ordered.
 *  - A box with a step of 0 or a zero extent intersects nothing.  The step of
 *    a dimension with a count of 1 is irrelevant.
 *  - With every step 1 the result is zcg_regions_v_waves'.
 *  - Boxes are hashed into cells by their hulls, as zcg_regions_v_waves does by
 *    their extents: the cell holds the largest hull (r->bbox_shape is not
 *    used), and the cost degrades in the same way.
 * Returns the number of waves; 0 for n_boxes == 0 or a NULL argument. */
uint32_t zcg_regions_s_waves(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                             const uint64_t* steps, uint32_t n_boxes, uint32_t* wave_of);

/* ---- many single elements by coordinate in one call ------------------------
 * numpy's a[i, j, k] with index arrays: sampled voxels, labelled points, sparse
 * annotations.  The reference reads or writes each through a 1-element
 * BoundingBox (read_ndarray, ndarray.rs:153-268; write_ndarray,
 * ndarray.rs:276-385), and that pins the semantics: A POINT IS THE BOX OF SHAPE
 * (1, ..., 1) AT ITS COORDINATE, for clipping, overhanging edge chunks, fill
 * versus untouched and NULL table entries.  Nothing of a box is built, though:
 * no record, no plan launch, no scratch; a lane of the kernel takes a point.
 *
 * `r` gives ndim, elem_size, chunk_order, fill_missing, fill_value,
 * array_shape and chunk_shape; r->bbox_offset, r->bbox_shape and
 * r->out_strides are ignored.  `coords` holds n_points*ndim coordinates,
 * point-major, as `offsets` does everywhere above.
 *
 * The chunk of a point, along dimension d, is grid index coords[d] /
 * chunk_shape[d], and the point VISITS it when the 1-element box does
 * (bounded_coord_iter, ndarray.rs:410-432; get_chunk_bounds,
 * ndarray.rs:434-446): along every dimension the coordinate is below
 * array_shape[d], or it is beyond it and no multiple of chunk_shape[d].  The
 * second case is the overhang of an edge chunk, which the box calls read and
 * write over its nominal extent as well.  Any other point visits no chunk.
 *
 * Host code, no GPU and no context:
 *  - zcg_points_grid: the smallest grid range lo[d] .. lo[d]+n[d] that holds
 *    every chunk a point visits; the return value and lo / n follow
 *    zcg_regions_grid's convention (0, with lo = n = 0, when no point visits a
 *    chunk or n_points is 0).  It is zcg_regions_v_grid on the same coordinates
 *    with every shape 1, by construction.
 *  - zcg_points_last: keep[i] (n_points bytes) = 1 if and only if no later
 *    point has the same coordinate, else 0; returns the number kept (0 for a
 *    NULL argument or ndim outside 1..ZCG_MAX_DIMS).  A sort: n log n. */
uint64_t zcg_points_grid(const zcg_region* r, const uint64_t* coords, uint64_t n_points, uint64_t* lo, uint64_t* n);
uint64_t zcg_points_last(const uint64_t* coords, uint64_t n_points, uint32_t ndim, uint8_t* keep);

/* d_coords is a DEVICE array of n_points*ndim coordinates; the values are a
 * dense DEVICE array of n_points elements of elem_size bytes, point i being
 * element i (d_out, written; d_in, only read).  The table arguments are
 * zcg_read_regions'.  d_first_outside is one DEVICE word.
 *  - zcg_read_points: point i receives the element of its chunk, at its
 *    chunk-local position in the chunk memory order, if it visits a chunk that
 *    is inside the table and not NULL; fill_value if fill_missing is set and
 *    the chunk is NULL or the point visits no chunk; nothing (d_out[i] is
 *    untouched) if fill_missing is clear.  No other byte of d_out is written.
 *  - zcg_write_points: point i's value goes to that position if the point
 *    visits a chunk that is inside the table and not NULL, the overhang of an
 *    edge chunk included; else it is dropped.  fill_missing and fill_value are
 *    ignored.  Two points of one call with the same coordinate leave the
 *    element with one of their values, whole; which one wins is unspecified
 *    (zcg_points_last tells a caller which points to drop so that the later
 *    one wins).
 *  - Points outside the table: a point that visits a chunk outside table_lo ..
 *    table_lo + table_n is neither read nor written (the box calls give such a
 *    box ZCG_ERR_INVALID_INPUT), and the other points are unaffected.  The
 *    call sets *d_first_outside to UINT64_MAX on the stream (an 8-byte
 *    device-to-device copy from a word the context owns: a captured memset
 *    node did not keep its fill pattern from one replay to the next), and
 *    the kernel lowers it to the lowest index of such a point (an atomic
 *    minimum per wave that has one).  There is no status word per point: at 1
 *    to 8 bytes of payload per point it would cost as much traffic as the
 *    data.
 *  - n_points == 0 returns ZCG_OK and launches nothing (d_first_outside is not
 *    written).
 *  - ndim outside 1..ZCG_MAX_DIMS, a bad elem_size, a chunk extent of 0 or of
 *    2^32 and above return ZCG_ERR_INVALID_INPUT, as zcg_read_regions does;
 *    so does a NULL d_coords, value array or d_first_outside.  n_points above
 *    2^60 returns ZCG_ERR_UNSUPPORTED.  A coordinate may be any uint64_t, up
 *    to 2^64-1.
 *  - Asynchronous on `stream`: one kernel launch plus that reset, whatever
 *    n_points is.  The call allocates nothing and does not synchronize with
 *    the host.  d_coords is read when the kernel runs, so the call can be
 *    captured in a graph and a replay sees new coordinates. */
int zcg_read_points(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                    const void* const* d_chunk_table, const uint64_t* d_coords, uint64_t n_points,
                    void* d_out, uint64_t* d_first_outside, void* stream);
int zcg_write_points(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                     void* const* d_chunk_table, const uint64_t* d_coords, uint64_t n_points,
                     const void* d_in, uint64_t* d_first_outside, void* stream);

/* ---- an orthogonal selection: one index list per dimension -----------------
 * numpy's a[np.ix_(rows, cols, planes)], zarr's oindex: the result is the
 * Cartesian product of the lists.  ELEMENT (i_0, .., i_{n-1}) OF THE SELECTION
 * IS THE POINT (L_0[i_0], .., L_{n-1}[i_{n-1}]) OF zcg_read_points /
 * zcg_write_points, BIT FOR BIT: the visit rule, the overhang of edge chunks,
 * fill versus untouched, NULL table entries, any uint64_t index.  What differs
 * is the cost: sum(count) divisions instead of prod(count) * ndim, and no
 * coordinate array.
 *
 * `r` gives what it gives the point calls (ndim, elem_size, chunk_order,
 * fill_missing, fill_value, array_shape, chunk_shape); its other fields are
 * ignored.  The table arguments are zcg_read_regions'.
 *
 * zcg_osel is a HOST struct.  index[d] is a DEVICE array of count[d] array
 * indices along dimension d, in any order, with or without duplicates; the
 * counts are host-known and size the launch.  Element (i_0, .., i_{n-1}) is at
 * base + sum(i_d * strides[d]) elements of the DEVICE view (any strides,
 * negative ones included).
 *
 * Host code, no GPU and no context:
 *  - zcg_ortho_chunks mirrors zcg_region_s_chunks.  lists[d] is a HOST array of
 *    count[d] indices.  lo / n receive the smallest grid range that holds every
 *    visited chunk, per dimension; if some dimension has no visiting index
 *    (an empty list included) all of them are 0 and so is the return value.
 *    touched (may be NULL) is dimension-major, n[0] + .. + n[ndim-1] bytes:
 *    1 where grid index lo[d] + j holds a visiting index of list d.  Returns
 *    the number of touched chunks, the product of the per-dimension touched
 *    counts (saturating).  lo and n equal zcg_points_grid's on the expanded
 *    product.
 *  - zcg_ortho_scratch_bytes: the device working memory of one call (a record
 *    per list entry); a multiple of 256, non-decreasing in every count.
 *
 * The device calls:
 *  - zcg_read_ortho writes exactly the elements of the view that
 *    zcg_read_points would write for the expanded product: the chunk's element,
 *    or fill_value with fill_missing set where the chunk is NULL or the point
 *    visits none; with fill_missing clear such an element is untouched.  No
 *    other byte of the view is written.
 *  - zcg_write_ortho stores whole elements only, into chunks that are visited,
 *    inside the table and not NULL.  With duplicate indices in a list one value
 *    wins whole, which one is unspecified: drop the earlier duplicates per list
 *    with zcg_points_last(list, count, 1, keep).  The view is only read.
 *  - d_outside is a DEVICE array of ndim words.  The table is a product range,
 *    so a chunk index outside it is a property of one list entry: word d ends
 *    up as the lowest position in list d whose index visits (along d: it is
 *    below array_shape[d] or no multiple of chunk_shape[d]) a grid index
 *    outside table_lo[d] .. table_lo[d] + table_n[d], UINT64_MAX if there is
 *    none.  An element is skipped (neither read nor written, no fill) exactly
 *    when the point call skips its point: it visits a chunk, and that chunk is
 *    outside the table along some dimension.  The words are reset on the stream
 *    by a device-to-device copy from words the context owns, as
 *    *d_first_outside is.
 *  - A zero count returns ZCG_OK; nothing is launched and d_outside is not
 *    written.  Argument errors are the point calls'; a NULL sel, list, base,
 *    scratch or d_outside returns ZCG_ERR_INVALID_INPUT, and so does a
 *    d_scratch that is not 16-byte aligned (the kernels read a record with
 *    two 16-byte loads).  count[d] >= 2^32 or prod(count) >= 2^60 returns
 *    ZCG_ERR_UNSUPPORTED.
 *  - Asynchronous on `stream`: the reset and two kernel launches, whatever the
 *    counts are.  The call allocates nothing and does not synchronize with the
 *    host.  The lists are read when the kernels run, so a captured call replays
 *    with new indices; the counts, strides and base are baked in. */
typedef struct zcg_osel {
    const uint64_t* index[ZCG_MAX_DIMS];  /* DEVICE: count[d] array indices along dim d */
    uint64_t count[ZCG_MAX_DIMS];         /* host-known; sizes the launch               */
    int64_t  strides[ZCG_MAX_DIMS];       /* the view's strides per array dim, elements */
    void*    base;                        /* DEVICE element (0,..,0) of the view        */
} zcg_osel;

uint64_t zcg_ortho_chunks(const zcg_region* r, const uint64_t* const* lists, const uint64_t* count,
                          uint64_t* lo, uint64_t* n, uint8_t* touched);
uint64_t zcg_ortho_scratch_bytes(uint32_t ndim, const uint64_t* count);
int zcg_read_ortho(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                   const void* const* d_chunk_table, const zcg_osel* sel,
                   void* d_scratch, uint64_t* d_outside, void* stream);
int zcg_write_ortho(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                    void* const* d_chunk_table, const zcg_osel* sel,
                    void* d_scratch, uint64_t* d_outside, void* stream);

/* ---- FilesystemHierarchy chunk files ---------------
 * The e2e path's two ends: chunk files read into pinned staging by a pool of
 * `io_threads` host threads (open + shared flock + read, as ReadableStore::get,
 * src/store/filesystem.rs:201-210), H2D, zcg_decode_batch, D2H into `dsts`
 * (N*elem_size bytes each), pipelined over two streams in sub-batches of
 * <= 256 MiB (1 GiB for xz/bzip2); status[i] = ZCG_ABSENT for a missing chunk (read_chunk -> None,
 * src/storage.rs:226-234), ZCG_ERR_IO for a filesystem error, else the decode
 * status.  The write direction encodes `elems` (N*elem_size host bytes each)
 * on the GPU and writes each file as WriteableStore::set (filesystem.rs:260-280):
 * create_dir_all(parent), open, exclusive flock, truncate, write.  Paths come
 * from the caller (get_chunk_key, storage.rs:109-127).  Blocking. */
int zcg_store_read_chunks(zcg_ctx* ctx, const zcg_array* array, uint32_t n, const char* const* paths,
                          void* const* dsts, int32_t* status, uint32_t io_threads);
int zcg_store_write_chunks(zcg_ctx* ctx, const zcg_array* array, uint32_t n, const char* const* paths,
                           const void* const* elems, int32_t* status, uint32_t io_threads);
/* Device-resident ends of the same two calls, for callers whose chunks live in
 * HBM (read_ndarray / write_ndarray, ndarray.rs:195-268,276-385, which call
 * read_chunk_into / write_chunk per chunk through the same store get()/set()):
 *  - zcg_store_read_chunks_device decodes each file straight into the caller's
 *    DEVICE slot d_dsts[i] (N*elem_size bytes); only the statuses come back.
 *    A slot whose chunk is absent or unreadable is left untouched.
 *  - zcg_store_write_chunks_device encodes the DEVICE element slots d_elems[i]
 *    and writes each file as set() does (exclusive flock, then truncate).
 * `status` is a host array; both calls block until the files are read/written.
 * Destinations of zcg_store_read_chunks that are page-locked host memory
 * (hipHostMalloc / hipHostRegister) receive the decoded chunk by a direct D2H. */
int zcg_store_read_chunks_device(zcg_ctx* ctx, const zcg_array* array, uint32_t n, const char* const* paths,
                                 void* const* d_dsts, int32_t* status, uint32_t io_threads);
int zcg_store_write_chunks_device(zcg_ctx* ctx, const zcg_array* array, uint32_t n, const char* const* paths,
                                  const void* const* d_elems, int32_t* status, uint32_t io_threads);

/* ---- several GPUs in one process -------------------------
 * Chunk i goes to devices[i mod n_devices]; one host thread and one context
 * per device, no collective (chunks are independent, chunk.rs:282,297); the
 * per-chunk status arrays are merged.  Same arguments as the single-context
 * calls; returns the first failing device's return code. */
typedef struct zcg_multi zcg_multi;
zcg_multi* zcg_multi_create(const int* devices, uint32_t n_devices);
void zcg_multi_destroy(zcg_multi* multi);
const char* zcg_multi_last_error(const zcg_multi* multi);
uint32_t zcg_multi_device_count(const zcg_multi* multi);
int zcg_multi_read_chunks_host(zcg_multi* multi, const zcg_array* array, uint32_t n, const void* const* srcs,
                               const uint64_t* src_lens, void* const* dsts, int32_t* status);
int zcg_multi_store_read_chunks(zcg_multi* multi, const zcg_array* array, uint32_t n,
                                const char* const* paths, void* const* dsts, int32_t* status,
                                uint32_t io_threads);
int zcg_multi_store_write_chunks(zcg_multi* multi, const zcg_array* array, uint32_t n,
                                 const char* const* paths, const void* const* elems, int32_t* status,
                                 uint32_t io_threads);

/* ---- array metadata JSON -------------------------
 * The Zarr v3.0-dev array document (ArrayMetadata's serde form, lib.rs:382-402;
 * DataType strings data_type.rs:165-240; ExtensibleDataType fallback
 * data_type.rs:282-310; CompressionType {"codec", "configuration"} with the
 * codecs' serde defaults, compression/mod.rs:36-51) parsed into the batch
 * API's descriptor, so a C or Rust caller can drive zcg_decode_batch from a
 * real hierarchy.  Returns ZCG_OK; ZCG_ERR_INVALID_DATA for a malformed
 * document (serde's io::ErrorKind::InvalidData); ZCG_ERR_UNSUPPORTED where the
 * reference panics (unknown endian/size character, an extended type without
 * fallback) or rejects the document (a must_understand extension,
 * storage.rs:172-176).  `err` (optional) receives a message. */
enum zcg_dtype_kind { ZCG_DT_BOOL = 0, ZCG_DT_INT = 1, ZCG_DT_UINT = 2, ZCG_DT_FLOAT = 3, ZCG_DT_RAW = 4 };
typedef struct zcg_array_meta {
    zcg_array array;            /* codec + configuration, effective dtype,
                                   chunk_num_elements = product(chunk_shape) (lib.rs:474-480) */
    uint32_t ndim;              /* len(shape) */
    uint32_t chunk_ndim;        /* len(chunk_shape) */
    uint32_t chunk_order;       /* chunk_memory_layout: 0 = "C" (RowMajor), 1 = "F" (ColumnMajor) */
    uint32_t dtype_kind;        /* enum zcg_dtype_kind of the effective type */
    uint32_t extended_type;     /* 1: data_type was an extension object (its fallback is used) */
    uint32_t has_fill_value;    /* fill_value present, not null, and convertible to the type */
    int32_t fill_value_status;  /* ZCG_OK, or why fill_value does not convert (get_effective_fill_value) */
    uint32_t reserved;
    uint64_t fill_value;        /* element bytes of the effective fill value, host order (0 = T::default()) */
    uint64_t shape[ZCG_MAX_DIMS];
    uint64_t chunk_shape[ZCG_MAX_DIMS];
    char separator[8];          /* chunk_grid.separator (get_chunk_key, storage.rs:109-127) */
} zcg_array_meta;

int zcg_array_meta_from_json(const char* json, uint64_t len, zcg_array_meta* out, char* err, uint64_t err_cap);

/* get_chunk_key (storage.rs:109-127): "/data/root/<path>/c<g0><sep><g1>...<sep><g(n-1)>",
 * with `path` canonicalised as canonicalize_path does (leading and trailing '/'
 * removed, lib.rs:187-189; an empty path gives "/data/root/c...") and `separator`
 * = chunk_grid.separator (zcg_array_meta.separator).  Writes at most cap-1 bytes
 * and a NUL (cap > 0); returns the key's full length, so a caller can size
 * `out`.  A FilesystemHierarchy file is the store root joined with the key
 * (filesystem.rs:142-190). */
uint64_t zcg_chunk_key(const char* path, const char* separator, const uint64_t* grid_position, uint32_t ndim,
                       char* out, uint64_t cap);

/* FilesystemHierarchy::get_path (src/store/filesystem.rs:151-190): the file a
 * key names under the store root `root`.  The key's leading '/'s are dropped
 * (it is taken relative to the root), empty and "." components vanish, ".."
 * stays in the path, and the key is refused with ZCG_ERR_NOT_FOUND when its
 * NET nesting (+1 per normal component, -1 per "..") is negative — the
 * reference's rule, so "a/../b" and even "../x" (net 0) are accepted, "../../x"
 * is not.  That rule lets "../x" resolve OUTSIDE the root: a reference flaw
 * restated on purpose (parity); callers writing untrusted keys should refuse
 * ".." components themselves.  The path is root + '/' + the normalised key
 * (just the key when root is empty, as PathBuf::join does).  *path_len (optional) receives its length;
 * `out` (cap bytes, NUL-terminated) may be NULL to query the length, and a cap
 * below path_len + 1 gives ZCG_ERR_OUTPUT_TOO_SMALL.  Returns ZCG_OK. */
int zcg_store_path(const char* root, const char* key, char* out, uint64_t cap, uint64_t* path_len);

/* ---- read_ndarray for many boxes, from the store to the boxes ------------
 * ZarrNdarrayReader::read_ndarray (ndarray.rs:153-268) for n_boxes boxes of one
 * shape `box_shape` (ndim) at `offsets` (n_boxes*ndim, box-major) of the array
 * `path` under the FilesystemHierarchy `root`, in one blocking call: the
 * chunks the boxes visit (the union of bounded_coord_iter's coordinates,
 * deduplicated) are each read (zcg_chunk_key + zcg_store_path, shared flock)
 * and decoded once, and one zcg_read_regions launch assembles every box.
 *  - decode flags come from meta->array.compression.flags (the verify flags
 *    work), element type and chunk order from `meta`, the fill value is
 *    meta->fill_value when has_fill_value, else 0;
 *  - an absent chunk is a NULL table entry; the first chunk whose status is
 *    neither ZCG_OK nor ZCG_ABSENT makes the call return that status,
 *    zcg_last_error names its grid position, and no box is guaranteed written;
 *  - a visited chunk outside the array's chunk grid (read_chunk panics there,
 *    storage.rs:217; the grid extent is the reference's u64_ceil_div,
 *    lib.rs:340-342, over-count included) -> ZCG_ERR_INVALID_INPUT before any
 *    file is read;
 *  - ndim != chunk_ndim -> ZCG_ERR_INVALID_DATA; a raw (rN) element type ->
 *    ZCG_ERR_INVALID_INPUT; a union chunk table above 2^24 entries, or boxes
 *    that hold more than 2^62 bytes in all, -> ZCG_ERR_UNSUPPORTED
 *    (zcg_last_error says so);
 *  - device memory: boxes are taken in consecutive groups whose unique chunks
 *    need at most slot_budget_bytes of decoded slots (0 = 4 GiB); a single box
 *    that alone exceeds the budget runs as its own group; a chunk two groups
 *    share is decoded in each.
 * zcg_store_read_boxes_device writes box i to the DEVICE view d_outs[i]
 * (out_strides per array dim, in elements; fill_missing as in zcg_region).
 * zcg_store_read_boxes writes box i to the HOST buffer outs[i], dense in the
 * chunk memory order and filled where no chunk is (read_ndarray's array), by
 * way of a device staging buffer and one D2H per group; n_boxes = 1 is the
 * reference's read_ndarray. */
int zcg_store_read_boxes_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                const uint64_t* box_shape, const int64_t* out_strides, uint32_t fill_missing,
                                const uint64_t* offsets, void* const* d_outs, uint32_t n_boxes,
                                uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_read_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                         const uint64_t* box_shape, const uint64_t* offsets, void* const* outs, uint32_t n_boxes,
                         uint64_t slot_budget_bytes, uint32_t io_threads);

/* ---- write_ndarray for many boxes, from the boxes to the store -----------
 * ZarrNdarrayWriter::write_ndarray (ndarray.rs:276-385) for n_boxes boxes of
 * one shape in one blocking call.  THE STORE ENDS UP AS IF write_ndarray HAD
 * RUN FOR BOX 0, 1, ..., n_boxes-1 IN THAT ORDER, but a chunk that k boxes
 * touch is read, encoded and written once, not k times.
 *  - Chunks written: the union of the chunks the boxes visit
 *    (bounded_coord_iter per box), each once per group, through
 *    zcg_store_write_chunks_device (set(): exclusive flock, then truncate).
 *    No other file is created or touched.
 *  - Chunks read first: take the lowest-numbered box that visits the chunk.
 *    If it does not cover the chunk's nominal bounds completely, the existing
 *    file is read and decoded (zcg_store_read_chunks_device, shared flock;
 *    decode flags, verify flags included, from meta->array.compression.flags),
 *    and an absent file makes the slot start as fill value (meta->fill_value
 *    when has_fill_value, else 0).  If it covers them completely the file is
 *    not read (ndarray.rs:327-335): a corrupt old file is then harmless.
 *  - Order: inside a group the boxes are scattered in the waves of
 *    zcg_regions_waves, in order on one stream: a later box wins every element
 *    it shares with an earlier one.
 *  - Groups: consecutive boxes whose unique chunks need at most
 *    slot_budget_bytes of decoded slots (0 = 4 GiB); a single box that alone
 *    exceeds the budget runs as its own group; a chunk two groups share is
 *    written by the first and read back by the second (zcg_store_read_boxes'
 *    grouping).
 *  - Before any file is read or written: a visited chunk outside the array's
 *    chunk grid (zcg_store_read_boxes' rule) -> ZCG_ERR_INVALID_INPUT;
 *    ndim != chunk_ndim -> ZCG_ERR_INVALID_DATA; a raw (rN) element type ->
 *    ZCG_ERR_INVALID_INPUT; a union chunk table above 2^24 entries, or boxes
 *    that hold more than 2^62 bytes in all, -> ZCG_ERR_UNSUPPORTED
 *    (zcg_last_error says so).
 *  - While running: the first chunk whose read status is neither ZCG_OK nor
 *    ZCG_ABSENT makes the call return that status, and zcg_last_error names
 *    its grid position; reads precede writes within a group, so nothing of
 *    that group has been written, and earlier groups stay written.  The first
 *    chunk that fails to write is returned and named in the same way.
 *  - n_boxes == 0, or a zero extent in box_shape, returns ZCG_OK and writes
 *    nothing.
 * zcg_store_write_boxes_device takes box i from the DEVICE view d_ins[i]
 * (in_strides per array dim, in elements).  zcg_store_write_boxes takes box i
 * from the HOST buffer ins[i], dense in the chunk memory order (the layout
 * zcg_store_read_boxes produces), staged with one H2D per group; n_boxes = 1
 * is the reference's write_ndarray. */
int zcg_store_write_boxes_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                 const uint64_t* box_shape, const int64_t* in_strides, const uint64_t* offsets,
                                 const void* const* d_ins, uint32_t n_boxes, uint64_t slot_budget_bytes,
                                 uint32_t io_threads);
int zcg_store_write_boxes(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                          const uint64_t* box_shape, const uint64_t* offsets, const void* const* ins,
                          uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads);

/* ---- read_ndarray / write_ndarray for many boxes of differing shapes ------
 * The four calls above with a shape per box: `box_shapes` holds n_boxes*ndim
 * extents, box-major, as `offsets` does.  Everything else carries over word
 * for word: the planning, the in-grid check before any file is touched, the
 * grouping by slot_budget_bytes, the rule for chunks read first (the
 * lowest-numbered box that visits the chunk covers its nominal bounds
 * completely -> the file is not read), the order (the waves of
 * zcg_regions_v_waves: a later box wins), the error reporting (the first
 * failing chunk is named by zcg_last_error) and the 2^24 table limit.  Each
 * shared chunk is read, decoded, encoded and written once; the boxes are
 * assembled or scattered by zcg_read_regions_v / zcg_write_regions_v, whose
 * bound is the largest extent per dimension among the boxes.
 *  - The _device forms take box i at the DEVICE view d_outs[i] / d_ins[i] with
 *    the strides out_strides / in_strides + i*ndim (n_boxes*ndim entries, per
 *    array dim, in elements); a NULL strides array means every box is dense in
 *    the chunk memory order.
 *  - The host forms take box i at the HOST buffer outs[i] / ins[i], dense in
 *    the chunk memory order with its own shape.
 *  - A box with a zero extent reads and writes nothing; n_boxes == 0 returns
 *    ZCG_OK.
 *  - A largest extent + chunk extent - 1 >= 2^32 along a dimension ->
 *    ZCG_ERR_UNSUPPORTED.
 * For n_boxes = 1 these calls are the reference's read_ndarray /
 * write_ndarray. */
int zcg_store_read_boxes_v_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                  const uint64_t* box_shapes, const int64_t* out_strides, uint32_t fill_missing,
                                  const uint64_t* offsets, void* const* d_outs, uint32_t n_boxes,
                                  uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_read_boxes_v(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                           const uint64_t* box_shapes, const uint64_t* offsets, void* const* outs,
                           uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_write_boxes_v_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                   const uint64_t* box_shapes, const int64_t* in_strides, const uint64_t* offsets,
                                   const void* const* d_ins, uint32_t n_boxes, uint64_t slot_budget_bytes,
                                   uint32_t io_threads);
int zcg_store_write_boxes_v(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                            const uint64_t* box_shapes, const uint64_t* offsets, const void* const* ins,
                            uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads);

/* ---- read_ndarray for many boxes with a step per dimension ----------------
 * zcg_store_read_boxes_v[_device] for strided boxes: `box_shapes` holds the
 * n_boxes*ndim SAMPLE COUNTS and `box_steps` the n_boxes*ndim steps (>= 1),
 * box-major, as `offsets` does; box b's result is what the _v call gives for
 * its hull, sliced [::step] per dimension.  Everything carries over from the _v
 * calls word for word, with one difference: THE CHUNKS READ AND DECODED ARE THE
 * UNION OF THE BOXES' TOUCHED CHUNKS (zcg_region_s_chunks), deduplicated, not
 * the hulls' grid ranges.  A chunk in a hull's range that holds no sample is
 * never opened or decoded, and its table entry stays NULL.
 *  - The slot budget and the grouping count touched chunks only.
 *  - The in-grid check (ZCG_ERR_INVALID_INPUT before any file is read) applies
 *    to touched chunks only: an untouched chunk of a hull's range outside the
 *    array's chunk grid is no error.
 *  - The 2^24 limit applies to the chunk TABLE, which covers the union of the
 *    hulls' grid ranges (per box and per group), touched or not ->
 *    ZCG_ERR_UNSUPPORTED.
 *  - A step of 0 -> ZCG_ERR_INVALID_INPUT; a hull extent + chunk extent - 1
 *    >= 2^32 along a dimension -> ZCG_ERR_UNSUPPORTED; both before any file is
 *    read.
 *  - The _device form takes box i at the DEVICE view d_outs[i] with the strides
 *    out_strides + i*ndim (NULL: dense in the chunk memory order, with the
 *    box's sample counts); fill_missing as in zcg_region.
 *  - The host form writes box i to the HOST buffer outs[i], dense in the chunk
 *    memory order with its own sample counts, and filled where no chunk is.
 * n_boxes = 1 with every step 1 is the reference's read_ndarray. */
int zcg_store_read_boxes_s_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                  const uint64_t* box_shapes, const uint64_t* box_steps, const int64_t* out_strides,
                                  uint32_t fill_missing, const uint64_t* offsets, void* const* d_outs,
                                  uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_read_boxes_s(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                           const uint64_t* box_shapes, const uint64_t* box_steps, const uint64_t* offsets,
                           void* const* outs, uint32_t n_boxes, uint64_t slot_budget_bytes, uint32_t io_threads);

/* ---- write_ndarray for many boxes with a step per dimension ----------------
 * zcg_store_write_boxes_v[_device] for strided boxes (a[o::k] = x in one call):
 * `box_shapes` holds the n_boxes*ndim SAMPLE COUNTS and `box_steps` the
 * n_boxes*ndim steps (>= 1), box-major, as `offsets` does.  The store ends up
 * as if, for box 0, 1, ... in order, the box's hull had been read
 * (read_ndarray, filled), the samples overlaid on it, and the hull's TOUCHED
 * chunks written by write_ndarray.  Everything carries over from the _v write
 * calls word for word, with the read side's _s differences:
 *  - The chunks read, encoded and written are the union of the boxes' touched
 *    chunks (zcg_region_s_chunks), each once per group.  A chunk of a hull's
 *    range that holds no sample is never opened, created, decoded or rewritten.
 *  - Chunks read first: take the lowest-numbered box that touches the chunk.
 *    The file is not read if and only if, along every dimension, every index of
 *    the chunk's nominal bounds is a sample of that box: that needs a step of 1
 *    (or a chunk extent of 1) and the run of samples across the chunk.  A
 *    corrupt old file is then harmless.  Otherwise the file is read and
 *    decoded, and an absent file makes the slot start as fill value.
 *  - The slot budget, the grouping and the in-grid check (ZCG_ERR_INVALID_INPUT
 *    before any file is touched) count touched chunks only.
 *  - The 2^24 limit applies to the chunk TABLE, which covers the union of the
 *    hulls' grid ranges -> ZCG_ERR_UNSUPPORTED.
 *  - A step of 0 -> ZCG_ERR_INVALID_INPUT; a hull extent + chunk extent - 1
 *    >= 2^32 along a dimension -> ZCG_ERR_UNSUPPORTED; both before any file is
 *    touched.
 *  - Order: inside a group the boxes are scattered by zcg_write_regions_s in
 *    the waves of zcg_regions_s_waves, in order on one stream: a later box wins
 *    every sample it shares with an earlier one, and interleaved boxes (even
 *    and odd planes) share a wave.
 *  - A call whose steps are all 1 and that has no empty box takes the _v plan
 *    and kernels, chunk for chunk and error for error.
 *  - The _device form takes box i from the DEVICE view d_ins[i] with the
 *    strides in_strides + i*ndim (NULL: dense in the chunk memory order, with
 *    the box's sample counts).  The host form takes box i from the HOST buffer
 *    ins[i], dense in the chunk memory order with its own sample counts.
 * n_boxes = 1 with every step 1 is the reference's write_ndarray. */
int zcg_store_write_boxes_s_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                   const uint64_t* box_shapes, const uint64_t* box_steps, const int64_t* in_strides,
                                   const uint64_t* offsets, const void* const* d_ins, uint32_t n_boxes,
                                   uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_write_boxes_s(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                            const uint64_t* box_shapes, const uint64_t* box_steps, const uint64_t* offsets,
                            const void* const* ins, uint32_t n_boxes, uint64_t slot_budget_bytes,
                            uint32_t io_threads);

/* ---- read_ndarray / write_ndarray for a list of coordinates -----------------
 * The _v store calls for the 1-element boxes at `coords` (HOST, n_points*ndim,
 * point-major), without the boxes: the values are one dense array of n_points
 * elements, point i being element i.  Blocking, as the box calls are.
 *  - The points are sorted on the host by chunk, then by their place in the
 *    chunk.  The chunks opened and decoded are the unique chunks a point
 *    visits (zcg_points_grid's rule), each once per group; no other file is
 *    opened.  Groups are consecutive runs of the SORTED points whose chunks fit
 *    slot_budget_bytes (0 = 4 GiB; at least one chunk); a group's table covers
 *    the bounding grid range of its chunks, and more than 2^24 entries ->
 *    ZCG_ERR_UNSUPPORTED.  One zcg_read_points / zcg_write_points launch per
 *    group, on the sorted coordinates.
 *  - Carried over from zcg_store_read_boxes_v word for word: the error
 *    reporting (the first failing chunk is named by zcg_last_error), absent
 *    files as NULL entries, the decode and verify flags of `meta`, the raw
 *    dtype and ndim checks, and the in-grid check before any file is touched: a
 *    point that visits a chunk outside the array's chunk grid ->
 *    ZCG_ERR_INVALID_INPUT, zcg_last_error names the point.
 *  - Read: the _device form writes d_out (DEVICE) in the caller's order, with
 *    fill_missing as in zcg_region; the host form fills `out` (HOST) and sets
 *    fill value where no chunk is.
 *  - Write: the store ends up as if write_ndarray had run for the 1-element
 *    boxes of point 0, 1, ... in order.  Of several points with one coordinate
 *    only the last is scattered (zcg_points_last).  Every visited chunk is read
 *    first (decoded; an absent one starts as fill value), except a chunk of one
 *    element, which its point covers; then it is scattered into, encoded and
 *    written once.  Reads precede writes inside a group.  No unvisited chunk is
 *    opened, created or rewritten; a point that visits no chunk is dropped.
 *  - n_points == 0 returns ZCG_OK; more than 2^32 points -> ZCG_ERR_UNSUPPORTED. */
int zcg_store_read_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                 const uint64_t* coords, uint64_t n_points, uint32_t fill_missing, void* d_out,
                                 uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_read_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                          const uint64_t* coords, uint64_t n_points, void* out, uint64_t slot_budget_bytes,
                          uint32_t io_threads);
int zcg_store_write_points_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                  const uint64_t* coords, uint64_t n_points, const void* d_in,
                                  uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_write_points(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                           const uint64_t* coords, uint64_t n_points, const void* in, uint64_t slot_budget_bytes,
                           uint32_t io_threads);

/* ---- an orthogonal selection against the store -------------------------------
 * The point store calls on the Cartesian product of `lists` (HOST: lists[d]
 * holds count[d] indices along dimension d) in C order, without the product:
 * the values are one dense array of prod(count) elements, C order over the
 * positions in the lists, dimension 0 slowest, whatever the chunk order is.
 *  - Plan: every list is sorted by chunk index, index and position, which costs
 *    the sum of the lists, never the product.  The touched chunks are the
 *    product of the per-dimension sets of visited grid indices
 *    (zcg_ortho_chunks); only those files are opened, and each is decoded once
 *    in the whole call.
 *  - Groups are sub-products of runs of the sorted lists, and a chunk belongs
 *    to one group: the longest suffix of dimensions whose touched grid indices
 *    fit slot_budget_bytes (0: 4 GiB) is taken whole, the dimension before it
 *    is cut into runs that fit, and the dimensions before that go one touched
 *    grid index at a time.  A read's run of indices that visit no chunk counts
 *    as one more grid index of its list here, so a group may hold one chunk
 *    fewer than the budget allows.  A group's table is the bounding grid range of its
 *    chunks (more than 2^24 entries -> ZCG_ERR_UNSUPPORTED); one zcg_read_ortho
 *    / zcg_write_ortho launch per group.  A read's indices that visit no chunk
 *    form a last run of their list and receive the fill value.
 *  - Errors, absent files (NULL entries), the decode and verify flags of
 *    `meta`, the dtype and ndim checks are the point calls'.  Before any file is
 *    touched: an index whose chunk is beyond the array's grid returns
 *    ZCG_ERR_INVALID_INPUT, and zcg_last_error names dimension and position.
 *  - Read: the host call fills elements without a chunk with the fill value;
 *    the device call does so with fill_missing set and leaves them untouched
 *    otherwise.
 *  - Write: the store ends up as after zcg_store_write_points on the product in
 *    C order, so per list the last occurrence of an index wins, and indices
 *    that visit no chunk are dropped.  Touched chunks are read first, except
 *    those the selection covers entirely; an absent one starts as the fill
 *    value.  Each touched chunk is encoded and written once; nothing else is
 *    opened, created or rewritten.
 *  - A zero count returns ZCG_OK.  count[d] >= 2^32 or 2^60 bytes of values and
 *    more -> ZCG_ERR_UNSUPPORTED.  The host calls pass the values through one
 *    device array of the selection's size. */
int zcg_store_read_ortho_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                const uint64_t* const* lists, const uint64_t* count, uint32_t fill_missing,
                                void* d_out, uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_read_ortho(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                         const uint64_t* const* lists, const uint64_t* count, void* out,
                         uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_write_ortho_device(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                                 const uint64_t* const* lists, const uint64_t* count, const void* d_in,
                                 uint64_t slot_budget_bytes, uint32_t io_threads);
int zcg_store_write_ortho(zcg_ctx* ctx, const zcg_array_meta* meta, const char* root, const char* path,
                          const uint64_t* const* lists, const uint64_t* count, const void* in,
                          uint64_t slot_budget_bytes, uint32_t io_threads);

#ifdef __cplusplus
}
#endif

#endif /* ZCHUNK_GPU_H */
