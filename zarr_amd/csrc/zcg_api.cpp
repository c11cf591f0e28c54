// zcg_api.cpp — C ABI of include/zchunk_gpu.h: context, dispatch by
// CompressionType (the reference's `match *self` in
// src/compression/mod.rs:72-108), workspace, and the host-memory
// conveniences that implement one DefaultChunk::read_chunk / write_chunk
// (src/chunk.rs:270-323) around the device batch kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "zcg_common.h"

using namespace zcg;

struct zcg_store_slots;

struct zcg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // internal stream of the host conveniences
    std::string err;
    // device workspace of the batch kernels, one per stream, so batches
    // enqueued on different streams of one ctx never share scratch
    // (at most WS_MAX of them: the least recently used one is freed when a
    // new stream needs one; a gzip workspace is ~100 MiB)
    struct Ws {
        void* stream;
        void* p;
        size_t bytes;
        uint64_t used;
        // the LZ4 decoder's side stream and its fork/join events, owned by
        // this (ctx, stream) pair: created on first use, never shared
        hipStream_t side = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
    };
    static constexpr size_t WS_MAX = 4;
    std::vector<Ws> ws;
    uint64_t ws_tick = 0;
    // host-convenience staging
    void* d_buf = nullptr;
    size_t d_buf_bytes = 0;
    void* h_pin = nullptr;
    size_t h_pin_bytes = 0;
    // store pipeline slots (zcg_store.cpp), created on first use
    zcg_store_slots* store = nullptr;
    // ZCG_MAX_DIMS device words holding UINT64_MAX: the source of the point calls'
    // reset of *d_first_outside and of the ortho calls' reset of d_outside (a copy,
    // not a memset: see launch_points)
    uint64_t* d_all_ones = nullptr;
};

namespace zcg {
int ctx_device(zcg_ctx* ctx) { return ctx->device; }
void ctx_set_error(zcg_ctx* ctx, const std::string& e) { ctx->err = e; }
zcg_store_slots* store_slots_new(int device);
void store_slots_free(zcg_store_slots* p);
zcg_store_slots* ctx_store_slots(zcg_ctx* ctx) {
    if (!ctx->store) {
        ctx->store = store_slots_new(ctx->device);
        if (!ctx->store) ctx->err = "store: stream/event creation failed";
    }
    return ctx->store;
}
}  // namespace zcg

namespace {

int fail(zcg_ctx* ctx, hipError_t e, const char* what) {
    if (ctx) {
        ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    }
    return ZCG_ERR_RUNTIME;
}

bool dtype_ok(const zcg_dtype& d) {
    if (d.is_bool) return d.elem_size == 1;
    return d.elem_size == 1 || d.elem_size == 2 || d.elem_size == 4 || d.elem_size == 8;
}

int ensure_dev(zcg_ctx* ctx, void** p, size_t* have, size_t need) {
    if (*have >= need && *p) return ZCG_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    size_t sz = need < 4096 ? 4096 : need;
    hipError_t e = hipMalloc(p, sz);
    if (e != hipSuccess) return fail(ctx, e, "hipMalloc");
    *have = sz;
    return ZCG_OK;
}

int ensure_pin(zcg_ctx* ctx, size_t need) {
    if (ctx->h_pin_bytes >= need && ctx->h_pin) return ZCG_OK;
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    ctx->h_pin = nullptr;
    ctx->h_pin_bytes = 0;
    size_t sz = need < 4096 ? 4096 : need;
    hipError_t e = hipHostMalloc(&ctx->h_pin, sz, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, e, "hipHostMalloc");
    ctx->h_pin_bytes = sz;
    return ZCG_OK;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

void ws_release(zcg_ctx::Ws& w) {
    if (w.p) (void)hipFree(w.p);
    if (w.fork) (void)hipEventDestroy(w.fork);
    if (w.join) (void)hipEventDestroy(w.join);
    if (w.side) (void)hipStreamDestroy(w.side);
    w.p = nullptr;
    w.fork = w.join = nullptr;
    w.side = nullptr;
}

// the side stream + events of a workspace (nullptr side on failure: the
// caller then runs single-stream)
void ws_side(zcg_ctx::Ws* w) {
    if (w->side) return;
    hipStream_t st = nullptr;
    hipEvent_t f = nullptr, j = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&f, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&j, hipEventDisableTiming) == hipSuccess) {
        w->side = st;
        w->fork = f;
        w->join = j;
        return;
    }
    if (j) (void)hipEventDestroy(j);
    if (f) (void)hipEventDestroy(f);
    if (st) (void)hipStreamDestroy(st);
}

// the workspace of batches enqueued on `stream`, grown to at least `need` bytes
int stream_ws(zcg_ctx* ctx, void* stream, size_t need, zcg_ctx::Ws** out) {
    zcg_ctx::Ws* w = nullptr;
    for (auto& x : ctx->ws)
        if (x.stream == stream) w = &x;
    if (!w) {
        if (ctx->ws.size() >= zcg_ctx::WS_MAX) {
            // evict the least recently used stream's workspace; that stream may
            // already be destroyed by the caller, so wait for the whole device
            size_t v = 0;
            for (size_t i = 1; i < ctx->ws.size(); i++)
                if (ctx->ws[i].used < ctx->ws[v].used) v = i;
            (void)hipDeviceSynchronize();
            ws_release(ctx->ws[v]);
            ctx->ws.erase(ctx->ws.begin() + (long)v);
        }
        ctx->ws.push_back({stream, nullptr, 0, 0});
        w = &ctx->ws.back();
    }
    w->used = ++ctx->ws_tick;
    if (w->bytes < need) (void)hipStreamSynchronize((hipStream_t)stream);  // old scratch may be in use
    const int r = ensure_dev(ctx, &w->p, &w->bytes, need);
    *out = w;
    return r;
}

}  // namespace

namespace zcg {
namespace {
std::mutex g_dev_mu;
std::map<int, uint32_t> g_dev_cus;
std::map<std::pair<const void*, int>, hipError_t> g_lds_attr;
}  // namespace

uint32_t device_cu_count() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_dev_cus.find(dev);
    if (it != g_dev_cus.end()) return it->second;
    int v = 0;
    const uint32_t cus =
        (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? (uint32_t)v
                                                                                                      : 256u;
    g_dev_cus[dev] = cus;
    return cus;
}

hipError_t lds_attr_once(const void* kernel, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    const auto key = std::make_pair(kernel, dev);
    auto it = g_lds_attr.find(key);
    if (it != g_lds_attr.end() && it->second == hipSuccess) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    g_lds_attr[key] = e;
    return e;
}
}  // namespace zcg

extern "C" {

int zcg_abi_version(void) { return ZCG_ABI_VERSION; }


const char* zcg_build_config(void) {
    static const std::string cfg = std::string(zcg::cfg_inflate_wave()) + ";" + zcg::cfg_inflate_par() + ";" +
                                   zcg::cfg_deflate() + ";" + zcg::cfg_raw() + ";" + zcg::cfg_region() + ";" +
                                   zcg::cfg_lz4_dec() + ";" + zcg::cfg_xz_opt() + ";" + zcg::cfg_bz2();
    return cfg.c_str();
}

zcg_ctx* zcg_create(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || device < 0 || device >= cnt) return nullptr;
    zcg_ctx* ctx = new zcg_ctx();
    ctx->device = device;
    (void)hipSetDevice(device);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return nullptr;
    }
    if (hipMalloc((void**)&ctx->d_all_ones, ZCG_MAX_DIMS * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(ctx->d_all_ones, 0xFF, ZCG_MAX_DIMS * sizeof(uint64_t)) != hipSuccess) {
        zcg_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void zcg_destroy(zcg_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->store) store_slots_free(ctx->store);
    for (auto& w : ctx->ws) ws_release(w);
    if (ctx->d_buf) (void)hipFree(ctx->d_buf);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->d_all_ones) (void)hipFree(ctx->d_all_ones);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* zcg_last_error(const zcg_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int32_t zcg_effective_gzip_level(int32_t level) { return (level < 0 || level > 9) ? 6 : level; }

int32_t zcg_effective_lz4_block_size(int32_t bs) {
    if (bs <= 65536) return 65536;
    if (bs <= 262144) return 262144;
    if (bs <= 1048576) return 1048576;
    return 4194304;
}

int zcg_codec_on_gpu(int32_t codec, int encode) {
    switch (codec) {
    case ZCG_CODEC_RAW: return 1;
    case ZCG_CODEC_LZ4: return 1;
    case ZCG_CODEC_GZIP: return 1;
    case ZCG_CODEC_ZLIB: return 1;
    case ZCG_CODEC_XZ: return 1;
    case ZCG_CODEC_BZIP2: return 1;
    default: return 0;
    }
}

uint64_t zcg_encode_bound(const zcg_compression* c, uint64_t n) {
    switch (c->codec) {
    case ZCG_CODEC_RAW: return n;
    case ZCG_CODEC_GZIP:  // 16 KiB segment slots (stored worst case + sync) + header/trailer
        return 18 + ((n + 16383) / 16384) * (16384 + 128) + 64;
    case ZCG_CODEC_ZLIB:  // the same, with the 2 + 4 frame bytes
        return 6 + ((n + 16383) / 16384) * (16384 + 128) + 64;
    case ZCG_CODEC_LZ4: {
        const uint64_t b = (uint64_t)zcg_effective_lz4_block_size(c->lz4_block_size);
        return 15 + (n / b + 1) * (b + 8) + 8;
    }
    case ZCG_CODEC_BZIP2:  // RLE1 can grow a block by 5/4; Huffman of that stays below 9/8
        return n + n / 4 + 65536;
    default: return n + n / 8 + 65536;
    }
}

uint64_t zcg_workspace_bytes(const zcg_array* a, uint32_t n, int encode) {
    if (!a) return 0;
    if (a->compression.codec == ZCG_CODEC_BZIP2)
        return encode ? bzip2_encode_ws_bytes(a, n) : bzip2_decode_ws_bytes(a, n);
    if (a->compression.codec == ZCG_CODEC_XZ && encode) return xz_encode_ws_bytes(a, n);
    if (a->compression.codec == ZCG_CODEC_GZIP || a->compression.codec == ZCG_CODEC_ZLIB)
        return encode ? deflate_ws_bytes(a, n) : gzip_decode_ws_bytes(a, n);
    if (a->compression.codec == ZCG_CODEC_LZ4) return encode ? lz4_encode_ws_bytes(a, n) : lz4_decode_ws_bytes(a, n);
    return 0;
}

int zcg_decode_batch(zcg_ctx* ctx, const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n,
                     int32_t* d_status, void* stream) {
    if (!ctx || !a || (n && (!d_chunks || !d_status))) return ZCG_ERR_INVALID_INPUT;
    if (!dtype_ok(a->dtype)) return ZCG_ERR_INVALID_INPUT;
    if (n == 0) return ZCG_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    switch (a->compression.codec) {
    case ZCG_CODEC_RAW: e = launch_raw(a, d_chunks, n, d_status, nullptr, 0, s); break;
    case ZCG_CODEC_LZ4: {
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, lz4_decode_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        ws_side(w);
        e = launch_lz4_decode(a, d_chunks, n, d_status, w->p, w->bytes, s, w->side, w->fork, w->join);
        break;
    }
    case ZCG_CODEC_GZIP:
    case ZCG_CODEC_ZLIB: {
        zcg_ctx::Ws* w = nullptr;
        const uint64_t need = gzip_decode_ws_bytes(a, n);  // (0: the serial kernel, no workspace)
        if (need) {
            const int r = stream_ws(ctx, stream, need, &w);
            if (r != ZCG_OK) return r;
        }
        e = launch_gzip_decode(a, d_chunks, n, d_status, w ? w->p : nullptr, w ? w->bytes : 0, s);
        break;
    }
    case ZCG_CODEC_XZ: e = launch_xz_decode(a, d_chunks, n, d_status, nullptr, 0, s); break;
    case ZCG_CODEC_BZIP2: {
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, bzip2_decode_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        e = launch_bzip2_decode(a, d_chunks, n, d_status, w->p, w->bytes, s);
        break;
    }
    default: return ZCG_ERR_INVALID_INPUT;
    }
    if (e != hipSuccess) return fail(ctx, e, "decode launch");
    return ZCG_OK;
}

int zcg_encode_batch(zcg_ctx* ctx, const zcg_array* a, const zcg_chunk* d_chunks, uint32_t n,
                     uint64_t* d_out_len, int32_t* d_status, void* stream) {
    if (!ctx || !a || (n && (!d_chunks || !d_status || !d_out_len))) return ZCG_ERR_INVALID_INPUT;
    if (!dtype_ok(a->dtype)) return ZCG_ERR_INVALID_INPUT;
    if (n == 0) return ZCG_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    switch (a->compression.codec) {
    case ZCG_CODEC_RAW: e = launch_raw(a, d_chunks, n, d_status, d_out_len, 1, s); break;
    case ZCG_CODEC_LZ4: {
        // The match-finder sort key holds (chunk, block) in 12 bits: at most
        // 4096 LZ4 blocks per chunk (256 MiB chunks at the 64 KiB default).
        const uint64_t B = (uint64_t)zcg_effective_lz4_block_size(a->compression.lz4_block_size);
        const uint64_t D = a->chunk_num_elements * (uint64_t)a->dtype.elem_size;
        if ((D + B - 1) / B > 4096) {
            ctx->err = "LZ4 encode supports at most 4096 blocks per chunk (" + std::to_string((D + B - 1) / B) +
                       " requested); use a larger block size or smaller chunks";
            return ZCG_ERR_UNSUPPORTED;
        }
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, lz4_encode_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        e = launch_lz4_encode(a, d_chunks, n, d_out_len, d_status, w->p, w->bytes, s);
        break;
    }
    case ZCG_CODEC_GZIP:
    case ZCG_CODEC_ZLIB: {
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, deflate_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        ws_side(w);
        e = launch_deflate(a, d_chunks, n, d_out_len, d_status, w->p, w->bytes, s, w->side, w->fork, w->join);
        break;
    }
    case ZCG_CODEC_XZ: {
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, xz_encode_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        e = launch_xz_encode(a, d_chunks, n, d_out_len, d_status, w->p, w->bytes, s);
        break;
    }
    case ZCG_CODEC_BZIP2: {
        const int32_t lv = a->compression.bzip2_block_size;
        if (lv < 1 || lv > 9) {  // BZ2_bzCompressInit rejects it (bzip2-rs panics)
            ctx->err = "bzip2 block size must be 1..9";
            return ZCG_ERR_INVALID_INPUT;
        }
        zcg_ctx::Ws* w = nullptr;
        const int r = stream_ws(ctx, stream, bzip2_encode_ws_bytes(a, n), &w);
        if (r != ZCG_OK) return r;
        e = launch_bzip2_encode(a, d_chunks, n, d_out_len, d_status, w->p, w->bytes, s);
        break;
    }
    default:
        ctx->err = "codec has no GPU encoder in this build";
        return ZCG_ERR_UNSUPPORTED;
    }
    if (e != hipSuccess) return fail(ctx, e, "encode launch");
    return ZCG_OK;
}

int zcg_read_chunks_host(zcg_ctx* ctx, const zcg_array* a, uint32_t n, const void* const* srcs,
                         const uint64_t* src_lens, void* const* dsts, int32_t* status) {
    if (!ctx || !a) return ZCG_ERR_INVALID_INPUT;
    if (!dtype_ok(a->dtype)) return ZCG_ERR_INVALID_INPUT;
    if (n == 0) return ZCG_OK;
    (void)hipSetDevice(ctx->device);
    const uint64_t D = a->chunk_num_elements * (uint64_t)a->dtype.elem_size;
    // device layout: [desc n][status n][src blobs (256-aligned)][dst n*D]
    size_t off_desc = 0;
    size_t off_stat = align_up(off_desc + sizeof(zcg_chunk) * n, 256);
    size_t off_src = align_up(off_stat + sizeof(int32_t) * n, 256);
    std::vector<size_t> so(n);
    size_t p = off_src;
    for (uint32_t i = 0; i < n; i++) { so[i] = p; p = align_up(p + src_lens[i], 256); }
    size_t off_dst = p;
    size_t total = align_up(off_dst + (size_t)D * n, 256);
    int r = ensure_dev(ctx, &ctx->d_buf, &ctx->d_buf_bytes, total);
    if (r) return r;
    r = ensure_pin(ctx, total);
    if (r) return r;
    uint8_t* hp = (uint8_t*)ctx->h_pin;
    uint8_t* dp = (uint8_t*)ctx->d_buf;
    zcg_chunk* hd = (zcg_chunk*)(hp + off_desc);
    for (uint32_t i = 0; i < n; i++) {
        memcpy(hp + so[i], srcs[i], src_lens[i]);
        hd[i].src = dp + so[i];
        hd[i].src_len = src_lens[i];
        hd[i].dst = dp + off_dst + (size_t)D * i;
        hd[i].dst_cap = D;
    }
    hipError_t e = hipMemcpyAsync(dp, hp, off_dst, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(ctx, e, "H2D");
    r = zcg_decode_batch(ctx, a, (const zcg_chunk*)(dp + off_desc), n, (int32_t*)(dp + off_stat),
                         ctx->stream);
    if (r) return r;
    e = hipMemcpyAsync(hp + off_stat, dp + off_stat, sizeof(int32_t) * n, hipMemcpyDeviceToHost,
                       ctx->stream);
    if (e == hipSuccess && D)
        e = hipMemcpyAsync(hp + off_dst, dp + off_dst, (size_t)D * n, hipMemcpyDeviceToHost,
                           ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, e, "D2H");
    const int32_t* hs = (const int32_t*)(hp + off_stat);
    for (uint32_t i = 0; i < n; i++) {
        status[i] = hs[i];
        if (hs[i] == ZCG_OK && D) memcpy(dsts[i], hp + off_dst + (size_t)D * i, D);
    }
    return ZCG_OK;
}

int zcg_read_chunk(zcg_ctx* ctx, const zcg_array* a, const void* src, uint64_t src_len,
                   void* dst) {
    int32_t st = ZCG_OK;
    void* const dsts[1] = {dst};
    const void* const srcs[1] = {src};
    int r = zcg_read_chunks_host(ctx, a, 1, srcs, &src_len, dsts, &st);
    return r ? r : st;
}

int zcg_write_chunk(zcg_ctx* ctx, const zcg_array* a, const void* elems, uint64_t n_elements,
                    void* out, uint64_t out_cap, uint64_t* out_len) {
    if (!ctx || !a || !out_len) return ZCG_ERR_INVALID_INPUT;
    *out_len = 0;
    if (!dtype_ok(a->dtype)) return ZCG_ERR_INVALID_INPUT;
    if (n_elements != a->chunk_num_elements) return ZCG_ERR_INVALID_DATA;  // chunk.rs:309-318
    if (!zcg_codec_on_gpu(a->compression.codec, 1)) {
        ctx->err = "codec has no GPU encoder in this build";
        return ZCG_ERR_UNSUPPORTED;
    }
    (void)hipSetDevice(ctx->device);
    const uint64_t nb = n_elements * (uint64_t)a->dtype.elem_size;
    const uint64_t cap = zcg_encode_bound(&a->compression, nb);
    // device layout: [desc][status][out_len][src nb][dst cap]
    size_t off_stat = 256, off_len = 512, off_src = 1024;
    size_t off_dst = align_up(off_src + nb, 256);
    size_t total = align_up(off_dst + cap, 256);
    int r = ensure_dev(ctx, &ctx->d_buf, &ctx->d_buf_bytes, total);
    if (r) return r;
    r = ensure_pin(ctx, total);
    if (r) return r;
    uint8_t* hp = (uint8_t*)ctx->h_pin;
    uint8_t* dp = (uint8_t*)ctx->d_buf;
    zcg_chunk* hd = (zcg_chunk*)hp;
    hd->src = dp + off_src;
    hd->src_len = nb;
    hd->dst = dp + off_dst;
    hd->dst_cap = cap;
    memcpy(hp + off_src, elems, nb);
    hipError_t e = hipMemcpyAsync(dp, hp, off_dst, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(ctx, e, "H2D");
    r = zcg_encode_batch(ctx, a, (const zcg_chunk*)dp, 1, (uint64_t*)(dp + off_len),
                         (int32_t*)(dp + off_stat), ctx->stream);
    if (r) return r;
    e = hipMemcpyAsync(hp + off_stat, dp + off_stat, off_src - off_stat, hipMemcpyDeviceToHost,
                       ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, e, "D2H");
    const int32_t st = *(int32_t*)(hp + off_stat);
    const uint64_t len = *(uint64_t*)(hp + off_len);
    if (st != ZCG_OK) return st;
    if (len > out_cap) return ZCG_ERR_OUTPUT_TOO_SMALL;
    e = hipMemcpy(out, dp + off_dst, len, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, e, "D2H");
    *out_len = len;
    return ZCG_OK;
}

uint64_t zcg_region_grid(const zcg_region* r, uint64_t* grid_lo, uint64_t* grid_n) {
    if (!r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS) return 0;
    uint64_t cnt = 1;
    for (uint32_t d = 0; d < r->ndim; d++) {
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        // bounded_coord_iter (ndarray.rs:410-432): bbox intersected with the
        // array bounds (BoundingBox::intersect, saturating), floor/ceil by chunk
        const uint64_t o = r->bbox_offset[d];
        const uint64_t e = std::min(r->bbox_offset[d] + r->bbox_shape[d], r->array_shape[d]);
        const uint64_t s = e > o ? e - o : 0;
        const uint64_t lo = o / cs, hi = (o + s + cs - 1) / cs;
        if (grid_lo) grid_lo[d] = lo;
        if (grid_n) grid_n[d] = hi - lo;
        cnt *= hi - lo;
    }
    return cnt;
}

// The array dimension at position k of the fast-first order (the chunks'
// memory order).
static uint32_t region_dim(const zcg_region* r, uint32_t k) { return r->chunk_order == 1 ? k : r->ndim - 1 - k; }

static int region_head(const zcg_ctx* ctx, const zcg_region* r) {
    if (!ctx || !r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS) return ZCG_ERR_INVALID_INPUT;
    const uint32_t es = r->elem_size;
    return es == 1 || es == 2 || es == 4 || es == 8 ? ZCG_OK : ZCG_ERR_INVALID_INPUT;
}

// What the region calls share: `r` validated and the walk filled in fast-first
// order, for a chunk table of extents tn (per array dim; NULL: no table) whose
// number of entries is returned in *entries.  The kernels hold a position
// along a dimension plus a box's offset into its first chunk in 32 bits:
// `off` is the one box's offset, or NULL for boxes at any offset (the offset
// into the chunk is then taken as chunk extent - 1); `too_far` is the error
// text of that limit.
static int region_walk(zcg_ctx* ctx, const zcg_region* r, const uint64_t* off, const uint64_t* tn,
                       const char* too_far, RegionWalk* w, uint64_t* entries) {
    const int head = region_head(ctx, r);
    if (head != ZCG_OK) return head;
    const uint32_t nd = r->ndim;
    *w = RegionWalk{};
    w->nd = nd;
    w->es = r->elem_size;
    w->fill = r->fill_missing ? 1u : 0u;
    w->V = 16 / r->elem_size;
    w->fillv = r->fill_value;
    uint64_t tstr[ZCG_MAX_DIMS];
    *entries = 1;
    for (int d = (int)nd - 1; d >= 0; d--) {
        tstr[d] = *entries;
        *entries *= tn ? tn[d] : 0;
    }
    uint64_t total = 1, cst = 1;
    for (uint32_t k = 0; k < nd; k++) {
        const uint32_t d = region_dim(r, k);
        const uint64_t cs = r->chunk_shape[d], bs = r->bbox_shape[d];
        if (cs == 0 || cs >= (1ull << 32)) return ZCG_ERR_INVALID_INPUT;
        if (bs + (off ? off[d] % cs : cs - 1) >= (1ull << 32)) {
            ctx->err = too_far;
            return ZCG_ERR_UNSUPPORTED;
        }
        w->bs[k] = (uint32_t)bs;
        w->cs[k] = (uint32_t)cs;
        w->tstr[k] = tstr[d];
        w->cstr[k] = cst;
        w->ostr[k] = r->out_strides[d];
        cst *= cs;
        total *= bs;
    }
    w->total = total;
    return ZCG_OK;
}

static int region_call(zcg_ctx* ctx, const zcg_region* r, const void* const* d_chunk_table, void* d_box,
                       void* stream, uint32_t dir) {
    uint64_t gn[ZCG_MAX_DIMS], nchunks;
    zcg_region_grid(r, nullptr, gn);
    RegionWalk w;
    const int rc = region_walk(ctx, r, r ? r->bbox_offset : nullptr, gn,
                               "region: box extent along a dimension must stay below 2^32 elements", &w, &nchunks);
    if (rc != ZCG_OK) return rc;
    if (dir) w.fill = 0;
    BoxTerms t{};
    for (uint32_t k = 0; k < w.nd; k++) {
        const uint32_t d = region_dim(r, k);
        t.orr[k] = (uint32_t)(r->bbox_offset[d] % w.cs[k]);
        t.gn[k] = (uint32_t)gn[d];  // <= offset into the chunk + box extent < 2^32
    }
    t.table = (const u8* const*)d_chunk_table;
    t.out = (u8*)d_box;
    if (w.total == 0) return ZCG_OK;
    if (!d_box || (nchunks && !d_chunk_table)) return ZCG_ERR_INVALID_INPUT;
    (void)hipSetDevice(ctx->device);
    const hipError_t e = launch_region(w, t, dir, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, e, "region launch");
    return ZCG_OK;
}

int zcg_read_region(zcg_ctx* ctx, const zcg_region* r, const void* const* d_chunk_table, void* d_out,
                    void* stream) {
    return region_call(ctx, r, d_chunk_table, d_out, stream, 0);
}

int zcg_write_region(zcg_ctx* ctx, const zcg_region* r, void* const* d_chunk_table, const void* d_in,
                     void* stream) {
    return region_call(ctx, r, (const void* const*)d_chunk_table, (void*)d_in, stream, 1);
}

// The hull of `cnt` samples `step` apart: (cnt - 1) * step + 1, saturating.
static uint64_t hull_extent(uint64_t cnt, uint64_t step) {
    if (cnt == 0) return 0;
    const unsigned __int128 e = (unsigned __int128)(cnt - 1) * step + 1;
    return e > ~0ull ? ~0ull : (uint64_t)e;
}

// The union of the boxes' grid ranges; `shapes` NULL: every box has
// r->bbox_shape.  `steps` not NULL: shapes are sample counts, a box's range is
// its hull's, and a box with a zero step adds nothing.
static uint64_t regions_grid(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                             const uint64_t* steps, uint64_t n_boxes, uint64_t* lo, uint64_t* n) {
    if (!r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS) return 0;
    const uint32_t nd = r->ndim;
    uint64_t ulo[ZCG_MAX_DIMS] = {0}, uhi[ZCG_MAX_DIMS] = {0};
    bool any = false;
    zcg_region one = *r;
    for (uint64_t b = 0; b < n_boxes && offsets; b++) {
        uint64_t blo[ZCG_MAX_DIMS], bn[ZCG_MAX_DIMS];
        bool stepped = true;
        for (uint32_t d = 0; d < nd; d++) {
            one.bbox_offset[d] = offsets[(size_t)b * nd + d];
            if (shapes) one.bbox_shape[d] = shapes[(size_t)b * nd + d];
            if (steps) {
                stepped &= steps[(size_t)b * nd + d] != 0;
                one.bbox_shape[d] = hull_extent(one.bbox_shape[d], steps[(size_t)b * nd + d]);
                // the end saturates (zcg_region_grid clips it to the array)
                if (one.bbox_offset[d] + one.bbox_shape[d] < one.bbox_offset[d])
                    one.bbox_shape[d] = ~0ull - one.bbox_offset[d];
            }
        }
        if (!stepped || zcg_region_grid(&one, blo, bn) == 0) continue;  // visits no chunk
        for (uint32_t d = 0; d < nd; d++) {
            ulo[d] = any ? std::min(ulo[d], blo[d]) : blo[d];
            uhi[d] = any ? std::max(uhi[d], blo[d] + bn[d]) : blo[d] + bn[d];
        }
        any = true;
    }
    uint64_t cnt = any ? 1 : 0;
    for (uint32_t d = 0; d < nd; d++) {
        if (lo) lo[d] = ulo[d];
        if (n) n[d] = uhi[d] - ulo[d];
        cnt *= uhi[d] - ulo[d];
    }
    return cnt;
}

uint64_t zcg_regions_grid(const zcg_region* r, const uint64_t* offsets, uint32_t n_boxes, uint64_t* lo,
                          uint64_t* n) {
    return regions_grid(r, offsets, nullptr, nullptr, n_boxes, lo, n);
}

uint64_t zcg_regions_v_grid(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes, uint32_t n_boxes,
                            uint64_t* lo, uint64_t* n) {
    return regions_grid(r, offsets, shapes, nullptr, shapes ? n_boxes : 0, lo, n);
}

uint64_t zcg_regions_s_grid(const zcg_region* r, const uint64_t* offsets, const uint64_t* shapes,
                            const uint64_t* steps, uint32_t n_boxes, uint64_t* lo, uint64_t* n) {
    return regions_grid(r, offsets, shapes, steps, shapes && steps ? n_boxes : 0, lo, n);
}

uint64_t zcg_region_s_chunks(const zcg_region* r, const uint64_t* offset, const uint64_t* shape,
                             const uint64_t* step, uint64_t* lo, uint64_t* n, uint8_t* touched) {
    if (!r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS || !offset || !shape || !step) return 0;
    const uint32_t nd = r->ndim;
    bool stepped = true;
    for (uint32_t d = 0; d < nd; d++) stepped &= step[d] != 0;
    if (!stepped) {
        for (uint32_t d = 0; d < nd; d++) {
            if (lo) lo[d] = 0;
            if (n) n[d] = 0;
        }
        return 0;
    }
    uint64_t glo[ZCG_MAX_DIMS], gn[ZCG_MAX_DIMS];
    zcg_region one = *r;
    for (uint32_t d = 0; d < nd; d++) {
        one.bbox_offset[d] = offset[d];
        one.bbox_shape[d] = hull_extent(shape[d], step[d]);
        if (one.bbox_offset[d] + one.bbox_shape[d] < one.bbox_offset[d]) one.bbox_shape[d] = ~0ull - offset[d];
    }
    const uint64_t hull_chunks = zcg_region_grid(&one, glo, gn);  // per dimension, also when the product is 0
    unsigned __int128 cnt = hull_chunks ? 1 : 0;
    for (uint32_t d = 0; d < nd; d++) {
        if (lo) lo[d] = glo[d];
        if (n) n[d] = gn[d];
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        uint64_t hit;
        if (step[d] <= cs && shape[d]) {
            // consecutive samples are at most a chunk apart: no chunk between the first and the last is skipped
            hit = gn[d];
            if (touched) memset(touched, 1, (size_t)gn[d]);
        } else {
            // every sample has a chunk of its own: those below the range's end
            const unsigned __int128 limit = (unsigned __int128)(glo[d] + gn[d]) * cs;
            const unsigned __int128 below = limit > offset[d] ? (limit - offset[d] + step[d] - 1) / step[d] : 0;
            hit = gn[d] ? (uint64_t)std::min<unsigned __int128>(below, shape[d]) : 0;
            if (touched) {
                memset(touched, 0, (size_t)gn[d]);
                for (uint64_t i = 0; i < hit; i++) touched[(offset[d] + i * step[d]) / cs - glo[d]] = 1;
            }
        }
        if (touched) touched += gn[d];
        cnt *= hit;
        if (cnt > ~0ull) cnt = ~0ull;
    }
    return (uint64_t)cnt;
}

static int regions_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        const void* const* d_chunk_table, const zcg_box* d_boxes, uint32_t n_boxes,
                        int32_t* d_status, void* stream, uint32_t dir) {
    if (n_boxes == 0) return region_head(ctx, r);
    RegionWalk w;
    uint64_t entries;
    const int rc = region_walk(ctx, r, nullptr, table_n,
                               "regions: box extent + chunk extent along a dimension must stay below 2^32 elements",
                               &w, &entries);
    if (rc != ZCG_OK) return rc;
    if (dir) w.fill = 0;
    BoxTable bt{};
    bt.nboxes = n_boxes;
    for (uint32_t k = 0; k < w.nd; k++) {
        const uint32_t d = region_dim(r, k);
        bt.dim[k] = d;
        bt.as[k] = r->array_shape[d];
        bt.tlo[k] = table_lo ? table_lo[d] : 0;
        bt.tn[k] = table_n ? table_n[d] : 0;
    }
    if (w.total == 0) return ZCG_OK;
    if (!d_boxes || !d_status || (entries && !d_chunk_table)) return ZCG_ERR_INVALID_INPUT;
    if (w.total > (1ull << 62) / n_boxes) {
        ctx->err = "regions: n_boxes x box elements must stay below 2^62";
        return ZCG_ERR_UNSUPPORTED;
    }
    (void)hipSetDevice(ctx->device);
    const hipError_t e = launch_regions(w, bt, d_chunk_table, d_boxes, d_status, dir, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, e, "regions launch");
    return ZCG_OK;
}

int zcg_read_regions(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                     const void* const* d_chunk_table, const zcg_box* d_boxes, uint32_t n_boxes,
                     int32_t* d_status, void* stream) {
    return regions_call(ctx, r, table_lo, table_n, d_chunk_table, d_boxes, n_boxes, d_status, stream, 0);
}

int zcg_write_regions(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                      void* const* d_chunk_table, const zcg_box* d_boxes, uint32_t n_boxes, int32_t* d_status,
                      void* stream) {
    return regions_call(ctx, r, table_lo, table_n, (const void* const*)d_chunk_table, d_boxes, n_boxes, d_status,
                        stream, 1);
}

uint64_t zcg_regions_v_scratch_bytes(uint32_t n_boxes) { return (regions_v_prefix_bytes(n_boxes) + 255) & ~255ull; }

uint64_t zcg_regions_s_scratch_bytes(uint32_t n_boxes) { return zcg_regions_v_scratch_bytes(n_boxes); }

// dir 0: zcg_read_regions_v, 1: zcg_write_regions_v (d_boxes: zcg_vbox); 2:
// zcg_read_regions_s, 3: zcg_write_regions_s (d_boxes: zcg_sbox, the bound is
// on the sample counts)
static int regions_v_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                          const void* const* d_chunk_table, const void* d_boxes, uint32_t n_boxes,
                          void* d_scratch, int32_t* d_status, void* stream, uint32_t dir) {
    if (n_boxes == 0) return region_head(ctx, r);
    RegionWalk w;  // w.bs, w.total: the bound
    uint64_t entries;
    const int rc = region_walk(ctx, r, nullptr, table_n,
                               "regions_v: largest box extent + chunk extent along a dimension must stay below "
                               "2^32 elements",
                               &w, &entries);
    if (rc != ZCG_OK) return rc;
    if (dir == 1 || dir == 3) w.fill = 0;
    BoxTable bt{};
    bt.nboxes = n_boxes;
    uint64_t total = 1;  // every extent is below 2^32: saturate at 2^63
    for (uint32_t k = 0; k < w.nd; k++) {
        const uint32_t d = region_dim(r, k);
        bt.dim[k] = d;
        bt.as[k] = r->array_shape[d];
        bt.tlo[k] = table_lo ? table_lo[d] : 0;
        bt.tn[k] = table_n ? table_n[d] : 0;
        w.ostr[k] = 0;
        total = w.bs[k] && total > (1ull << 63) / w.bs[k] ? 1ull << 63 : total * w.bs[k];
    }
    w.total = total;
    if (!d_boxes || !d_status || !d_scratch || ((uintptr_t)d_scratch & 7) || (entries && !d_chunk_table))
        return ZCG_ERR_INVALID_INPUT;
    // zcg_read_regions' limit, on the bound: it keeps a box's element count and
    // the 64-bit prefix sum of all boxes' work units from overflowing
    if (total > (1ull << 62) / n_boxes) {
        ctx->err = "regions_v: n_boxes x the bound's elements must stay below 2^62";
        return ZCG_ERR_UNSUPPORTED;
    }
    (void)hipSetDevice(ctx->device);
    const hipError_t e =
        dir == 3 ? launch_regions_sw(w, bt, (void* const*)d_chunk_table, (const zcg_sbox*)d_boxes, d_scratch,
                                     d_status, (hipStream_t)stream) :
        dir == 2 ? launch_regions_s(w, bt, d_chunk_table, (const zcg_sbox*)d_boxes, d_scratch, d_status,
                                    (hipStream_t)stream)
                 : launch_regions_v(w, bt, d_chunk_table, (const zcg_vbox*)d_boxes, d_scratch, d_status, dir,
                                    (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, e, dir >= 2 ? "regions_s launch" : "regions_v launch");
    return ZCG_OK;
}

int zcg_read_regions_v(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                       const void* const* d_chunk_table, const zcg_vbox* d_boxes, uint32_t n_boxes, void* d_scratch,
                       int32_t* d_status, void* stream) {
    return regions_v_call(ctx, r, table_lo, table_n, d_chunk_table, d_boxes, n_boxes, d_scratch, d_status, stream,
                          0);
}

int zcg_write_regions_v(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        void* const* d_chunk_table, const zcg_vbox* d_boxes, uint32_t n_boxes, void* d_scratch,
                        int32_t* d_status, void* stream) {
    return regions_v_call(ctx, r, table_lo, table_n, (const void* const*)d_chunk_table, d_boxes, n_boxes, d_scratch,
                          d_status, stream, 1);
}

int zcg_read_regions_s(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                       const void* const* d_chunk_table, const zcg_sbox* d_boxes, uint32_t n_boxes, void* d_scratch,
                       int32_t* d_status, void* stream) {
    return regions_v_call(ctx, r, table_lo, table_n, d_chunk_table, d_boxes, n_boxes, d_scratch, d_status, stream,
                          2);
}

int zcg_write_regions_s(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                        void* const* d_chunk_table, const zcg_sbox* d_boxes, uint32_t n_boxes, void* d_scratch,
                        int32_t* d_status, void* stream) {
    return regions_v_call(ctx, r, table_lo, table_n, (const void* const*)d_chunk_table, d_boxes, n_boxes, d_scratch,
                          d_status, stream, 3);
}

}  // extern "C"

// ---- a list of coordinates (zcg_region_p.hip) -------------------------------
// A point is the box of shape (1, ..., 1) at its coordinate: its grid range is
// zcg_region_grid's for that box, so zcg_points_grid is zcg_regions_v_grid with
// every shape 1 by construction.
extern "C" uint64_t zcg_points_grid(const zcg_region* r, const uint64_t* coords, uint64_t n_points, uint64_t* lo,
                                    uint64_t* n) {
    if (!r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS) return 0;
    zcg_region one = *r;
    for (uint32_t d = 0; d < r->ndim; d++) one.bbox_shape[d] = 1;
    return regions_grid(&one, coords, nullptr, nullptr, n_points, lo, n);
}

namespace zcg {
// zcg_read_points (dir 0) and zcg_write_points (dir 1); d_order (DEVICE,
// n_points entries, or NULL) places point p's value at element d_order[p] of
// d_vals: the store calls hand the kernel points sorted by chunk
// (zcg_points.cpp).
int points_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                const void* const* d_chunk_table, const uint64_t* d_coords, const uint64_t* d_order,
                uint64_t n_points, void* d_vals, uint64_t* d_first_outside, void* stream, uint32_t dir) {
    const int head = region_head(ctx, r);
    if (head != ZCG_OK || n_points == 0) return head;
    zcg_region one = *r;  // bbox_* are ignored
    for (uint32_t d = 0; d < r->ndim; d++) one.bbox_shape[d] = 1;
    RegionWalk w;
    uint64_t entries;
    const int rc = region_walk(ctx, &one, nullptr, table_n, "points: chunk extent must stay below 2^32 elements", &w,
                               &entries);
    if (rc != ZCG_OK) return rc;
    if (dir) w.fill = 0;
    BoxTable bt{};
    PointRecip pr{};
    for (uint32_t k = 0; k < w.nd; k++) {
        const uint32_t d = region_dim(r, k);
        bt.dim[k] = d;
        bt.as[k] = r->array_shape[d];
        bt.tlo[k] = table_lo ? table_lo[d] : 0;
        bt.tn[k] = table_n ? table_n[d] : 0;
        pr.m[k] = w.cs[k] > 1 ? ~0ull / w.cs[k] + 1 : 0;  // ceil(2^64 / chunk extent)
    }
    if (!d_coords || !d_vals || !d_first_outside || (entries && !d_chunk_table)) return ZCG_ERR_INVALID_INPUT;
    if (n_points > (1ull << 60)) {
        ctx->err = "points: n_points must stay at or below 2^60";
        return ZCG_ERR_UNSUPPORTED;
    }
    (void)hipSetDevice(ctx->device);
    const hipError_t e = launch_points(w, bt, pr, n_points, d_chunk_table, d_coords, d_order, d_vals, d_first_outside,
                                       ctx->d_all_ones, dir, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, e, "points launch");
    return ZCG_OK;
}
}  // namespace zcg

extern "C" int zcg_read_points(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                               const void* const* d_chunk_table, const uint64_t* d_coords, uint64_t n_points,
                               void* d_out, uint64_t* d_first_outside, void* stream) {
    return zcg::points_call(ctx, r, table_lo, table_n, d_chunk_table, d_coords, nullptr, n_points, d_out,
                            d_first_outside, stream, 0);
}

extern "C" int zcg_write_points(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                                void* const* d_chunk_table, const uint64_t* d_coords, uint64_t n_points,
                                const void* d_in, uint64_t* d_first_outside, void* stream) {
    return zcg::points_call(ctx, r, table_lo, table_n, (const void* const*)d_chunk_table, d_coords, nullptr, n_points,
                            (void*)d_in, d_first_outside, stream, 1);
}

// ---- an index list per dimension (zcg_region_o.hip) -------------------------
// Element (i_0, .., i_{n-1}) of the selection is the point (L_0[i_0], ..,
// L_{n-1}[i_{n-1}]), so whether an entry visits a chunk is the point rule along
// its dimension (points_kernel), and the touched chunks are the product of the
// per-dimension sets of visited grid indices.
extern "C" uint64_t zcg_ortho_chunks(const zcg_region* r, const uint64_t* const* lists, const uint64_t* count,
                                     uint64_t* lo, uint64_t* n, uint8_t* touched) {
    if (!r || r->ndim < 1 || r->ndim > ZCG_MAX_DIMS || !lists || !count) return 0;
    const uint32_t nd = r->ndim;
    uint64_t glo[ZCG_MAX_DIMS], ghi[ZCG_MAX_DIMS];
    bool every = true;
    for (uint32_t d = 0; d < nd; d++) {
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        bool any = false;
        for (uint64_t i = 0; i < count[d] && lists[d]; i++) {
            const uint64_t c = lists[d][i], q = c / cs;
            if (!(c < r->array_shape[d] || c % cs)) continue;
            glo[d] = any ? std::min(glo[d], q) : q;
            ghi[d] = any ? std::max(ghi[d], q) : q;
            any = true;
        }
        every &= any;
    }
    unsigned __int128 cnt = every ? 1 : 0;
    for (uint32_t d = 0; d < nd; d++) {
        const uint64_t gn = every ? ghi[d] - glo[d] + 1 : 0;
        if (lo) lo[d] = every ? glo[d] : 0;
        if (n) n[d] = gn;
        if (!every) continue;
        const uint64_t cs = r->chunk_shape[d] ? r->chunk_shape[d] : 1;
        uint64_t hit = 0;
        if (touched) {
            memset(touched, 0, (size_t)gn);
            for (uint64_t i = 0; i < count[d]; i++) {
                const uint64_t c = lists[d][i];
                if (!(c < r->array_shape[d] || c % cs)) continue;
                hit += touched[c / cs - glo[d]] ? 0 : 1;
                touched[c / cs - glo[d]] = 1;
            }
            touched += gn;
        } else {  // the distinct grid indices, without the flags' memory
            std::vector<uint64_t> qs;
            for (uint64_t i = 0; i < count[d]; i++)
                if (lists[d][i] < r->array_shape[d] || lists[d][i] % cs) qs.push_back(lists[d][i] / cs);
            std::sort(qs.begin(), qs.end());
            hit = (uint64_t)(std::unique(qs.begin(), qs.end()) - qs.begin());
        }
        cnt *= hit;
        if (cnt > ~0ull) cnt = ~0ull;
    }
    return (uint64_t)cnt;
}

extern "C" uint64_t zcg_ortho_scratch_bytes(uint32_t ndim, const uint64_t* count) {
    unsigned __int128 sum = 0;
    for (uint32_t d = 0; count && d < ndim && d < ZCG_MAX_DIMS; d++) sum += count[d];
    sum = sum * zcg::ORTHO_REC_BYTES + 255;
    return sum > ~0ull ? ~0ull & ~255ull : (uint64_t)sum & ~255ull;
}

namespace zcg {
// zcg_read_ortho (dir 0) and zcg_write_ortho (dir 1); d_pos (per array dim a
// DEVICE array of count[d] positions, or NULL; d_pos itself may be NULL) places
// entry i of list d at position d_pos[d][i] of the view along d: the store
// calls hand the kernels sorted lists without duplicates (zcg_boxes.cpp).
int ortho_call(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
               const void* const* d_chunk_table, const zcg_osel* sel, const uint64_t* const* d_pos, void* d_scratch,
               uint64_t* d_outside, void* stream, uint32_t dir) {
    const int head = region_head(ctx, r);
    if (head != ZCG_OK) return head;
    if (!sel) return ZCG_ERR_INVALID_INPUT;
    const uint32_t nd = r->ndim;
    for (uint32_t d = 0; d < nd; d++)
        if (sel->count[d] == 0) return ZCG_OK;
    zcg_region one = *r;  // bbox_* and out_strides are ignored
    for (uint32_t d = 0; d < nd; d++) one.bbox_shape[d] = 1;
    RegionWalk w;
    uint64_t entries;
    const int rc = region_walk(ctx, &one, nullptr, table_n, "ortho: chunk extent must stay below 2^32 elements", &w,
                               &entries);
    if (rc != ZCG_OK) return rc;
    if (dir) w.fill = 0;
    if (!sel->base || !d_scratch || ((uintptr_t)d_scratch & 15) || !d_outside || (entries && !d_chunk_table))
        return ZCG_ERR_INVALID_INPUT;
    for (uint32_t d = 0; d < nd; d++)
        if (!sel->index[d]) return ZCG_ERR_INVALID_INPUT;
    uint64_t total = 1;
    for (uint32_t d = 0; d < nd; d++) {
        if (sel->count[d] >= (1ull << 32)) {
            ctx->err = "ortho: a list must hold fewer than 2^32 indices";
            return ZCG_ERR_UNSUPPORTED;
        }
        total = total >= (1ull << 60) / sel->count[d] + 1 ? 1ull << 60 : total * sel->count[d];
    }
    if (total >= (1ull << 60)) {
        ctx->err = "ortho: the selection must hold fewer than 2^60 elements";
        return ZCG_ERR_UNSUPPORTED;
    }
    BoxTable bt{};
    PointRecip pr{}, pcount{};
    OrthoAxes ax{};
    auto recip = [](uint64_t x) { return x > 1 ? ~0ull / x + 1 : 0; };  // ceil(2^64 / x)
    uint64_t rows = 1;
    for (uint32_t k = 0; k < nd; k++) {
        const uint32_t d = region_dim(r, k);
        bt.dim[k] = d;
        bt.as[k] = r->array_shape[d];
        bt.tlo[k] = table_lo ? table_lo[d] : 0;
        bt.tn[k] = table_n ? table_n[d] : 0;
        pr.m[k] = recip(w.cs[k]);
        w.bs[k] = (uint32_t)sel->count[d];
        w.ostr[k] = sel->strides[d];
        pcount.m[k] = recip(w.bs[k]);
        ax.off[k + 1] = ax.off[k] + sel->count[d];
        ax.idx[k] = sel->index[d];
        ax.pos[k] = d_pos ? d_pos[d] : nullptr;
        if (k) rows *= sel->count[d];
    }
    ax.ppr = (uint32_t)((w.bs[0] + (uint64_t)w.V - 1) / w.V);
    ax.mppr = recip(ax.ppr);
    w.total = rows * ax.ppr;
    (void)hipSetDevice(ctx->device);
    const hipError_t e = launch_ortho(w, bt, pr, pcount, ax, d_chunk_table, sel->base, d_scratch, d_outside,
                                      ctx->d_all_ones, dir, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, e, "ortho launch");
    return ZCG_OK;
}
}  // namespace zcg

extern "C" int zcg_read_ortho(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                              const void* const* d_chunk_table, const zcg_osel* sel, void* d_scratch,
                              uint64_t* d_outside, void* stream) {
    return zcg::ortho_call(ctx, r, table_lo, table_n, d_chunk_table, sel, nullptr, d_scratch, d_outside, stream, 0);
}

extern "C" int zcg_write_ortho(zcg_ctx* ctx, const zcg_region* r, const uint64_t* table_lo, const uint64_t* table_n,
                               void* const* d_chunk_table, const zcg_osel* sel, void* d_scratch, uint64_t* d_outside,
                               void* stream) {
    return zcg::ortho_call(ctx, r, table_lo, table_n, (const void* const*)d_chunk_table, sel, nullptr, d_scratch,
                           d_outside, stream, 1);
}
