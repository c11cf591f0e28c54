// zlib_ref.cpp — TEST INFRASTRUCTURE ONLY.
//
// A serial CPU driver of zarr_amd/csrc/zcg_zlib_core.h (the zlib 1.2.11
// deflate_slow restatement the GPU gzip encoder runs): hash chains by a
// head table, zz::search at every position, zz::parse, and per block
// zz::plan_block + the bits.  tests/test_hostcore.py compares its raw-deflate
// output with the system zlib (levels 4-9) byte for byte; the GPU kernels are
// compared with this and with zlib.  Never linked into the product.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../zarr_amd/csrc/zcg_zlib_core.h"

namespace {
struct BitOut {
    uint8_t* out;
    uint64_t cap, n = 0;
    uint64_t acc = 0;
    uint32_t nb = 0;
    bool over = false;
    void byte(uint32_t b) {
        if (n < cap) out[n] = (uint8_t)b; else over = true;
        n++;
    }
    void put(uint32_t v, uint32_t bits) {
        if (!bits) return;
        acc |= (uint64_t)(v & ((bits == 32) ? 0xFFFFFFFFu : ((1u << bits) - 1))) << nb;
        nb += bits;
        while (nb >= 8) { byte((uint32_t)acc & 0xFF); acc >>= 8; nb -= 8; }
    }
    void windup() {
        if (nb) { byte((uint32_t)acc & 0xFF); acc = 0; nb = 0; }
    }
};
}  // namespace

// zlib's head[] / prev[] (window-relative Pos, 0 = NIL) for zz::parse_fast
struct FastTab {
    std::vector<uint16_t> hd, pv;
    FastTab() : hd(1u << 15, 0), pv(zz::WSIZE, 0) {}
    uint32_t head(uint32_t h) const { return hd[h]; }
    void set_head(uint32_t h, uint32_t v) { hd[h] = (uint16_t)v; }
    uint32_t prev(uint32_t i) const { return pv[i]; }
    void set_prev(uint32_t i, uint32_t v) { pv[i] = (uint16_t)v; }
    void slide() {  // slide_hash
        for (auto& x : hd) x = x >= zz::WSIZE ? (uint16_t)(x - zz::WSIZE) : 0;
        for (auto& x : pv) x = x >= zz::WSIZE ? (uint16_t)(x - zz::WSIZE) : 0;
    }
};

// What zz_host_report_blocks returns per block (ZZ_BLOCK_WORDS u32 each)
constexpr uint32_t ZZ_BLOCK_WORDS = 13;
static int64_t emit_blocks(const uint8_t* src, const std::vector<uint32_t>& syms,
                           const std::vector<zz::BlockRec>& blocks, uint8_t* out, uint64_t cap,
                           uint32_t* report = nullptr);

// The serial model's symbols and block records of one chunk (levels 1-9)
static void serial_parse(const uint8_t* src, uint32_t D, int level, std::vector<uint32_t>& syms,
                         std::vector<zz::BlockRec>& blocks) {
    using namespace zz;
    const Config cfg = level_config(level);
    if (level >= 1 && level <= 3) {  // deflate_fast: the parse builds its chains
        auto byte = [&](uint32_t i) -> uint32_t { return src[i]; };
        auto byte4 = [&](uint32_t i) -> uint32_t {
            uint32_t v;
            memcpy(&v, src + i, 4);
            return v;
        };
        FastTab tab;
        std::vector<uint32_t> pos;
        auto emit = [&](uint32_t s, uint32_t at) { syms.push_back(s); pos.push_back(at); };
        const uint32_t nsym = parse_fast(D, cfg, tab, byte4, byte, emit);
        auto P = [&](uint32_t i) -> uint32_t { return pos[i]; };
        auto Y = [&](uint32_t i) -> uint32_t { return syms[i]; };
        for (uint32_t k = 0; k < num_blocks(nsym); k++) blocks.push_back(block_rec(k, nsym, nsym, D, P, Y, true));
        return;
    }
    std::vector<uint32_t> prev(D ? D : 1, NONE), head(1u << 15, NONE);
    for (uint32_t p = 0; p + MIN_MATCH <= D; p++) {
        const uint32_t h = hash3(src[p], src[p + 1], src[p + 2]);
        prev[p] = head[h];
        head[h] = p;
    }
    auto byte = [&](uint32_t i) -> uint32_t { return src[i]; };
    auto byte4 = [&](uint32_t i) -> uint32_t {
        uint32_t v;
        memcpy(&v, src + i, 4);
        return v;
    };
    auto pr = [&](uint32_t i) -> uint32_t { return prev[i]; };
    std::vector<Match2> g(D ? D : 1);
    for (uint32_t p = 0; p < D; p++) g[p] = search(p, D, cfg, byte4, byte, pr);
    auto get = [&](uint32_t p) -> Match2 { return g[p]; };
    auto emit = [&](uint32_t, uint32_t s) { syms.push_back(s); };
    auto flush = [&](const BlockRec& b) { blocks.push_back(b); };
    parse(D, cfg, get, byte, emit, flush);
}

extern "C" int64_t zz_host_deflate(const uint8_t* src, uint32_t D, int level, uint8_t* out, uint64_t cap) {
    std::vector<uint32_t> syms;
    std::vector<zz::BlockRec> blocks;
    serial_parse(src, D, level, syms, blocks);
    return emit_blocks(src, syms, blocks, out, cap);
}

// Whether gen_bitlen had to limit this tree's lengths, read from what
// build_tree leaves behind: a leaf whose path to the root over dad[] is longer
// than max_length.  (Leaves are the nodes below `elems` with a frequency, the
// forced ones included; internal nodes are numbered from `elems` up, the root
// last.)
template <class Tree>
static uint32_t tree_limited(const Tree& t, int elems, int max_length) {
    int leaves = 0;
    for (int n = 0; n < elems; n++) leaves += t.freq[n] != 0;
    const int root = elems + leaves - 2;
    for (int n = 0; n < elems; n++) {
        if (!t.freq[n]) continue;
        int depth = 0;
        for (int m = n; m != root; m = t.dad[m]) depth++;
        if (depth > max_length) return 1;
    }
    return 0;
}

// The serial model's path through one chunk, as plain integers: per block
// s0, s1, b0, b1, in_win, last, type, opt_lenb, static_lenb, max_blindex and
// whether the literal/length, distance and code-length trees were
// length-limited.  Returns the block count (blocks past cap_blocks are not
// written).
extern "C" int32_t zz_host_report_blocks(const uint8_t* src, uint32_t D, int level, uint32_t* out,
                                         uint32_t cap_blocks) {
    std::vector<uint32_t> syms;
    std::vector<zz::BlockRec> blocks;
    serial_parse(src, D, level, syms, blocks);
    if (blocks.size() > cap_blocks) blocks.resize(cap_blocks);
    std::vector<uint8_t> sink(D + D / 8 + 1024);
    emit_blocks(src, syms, blocks, sink.data(), sink.size(), out);
    return (int32_t)blocks.size();
}

static int64_t emit_blocks(const uint8_t* src, const std::vector<uint32_t>& syms,
                           const std::vector<zz::BlockRec>& blocks, uint8_t* out, uint64_t cap, uint32_t* report) {
    using namespace zz;
    BitOut bo{out, cap};
    BlockWork* bw = new BlockWork;
    for (const BlockRec& b : blocks) {
        for (int i = 0; i < HEAP_SIZE; i++) bw->lt.freq[i] = 0;
        for (int i = 0; i < 2 * D_CODES + 1; i++) bw->dt.freq[i] = 0;
        for (uint32_t k = b.s0; k < b.s1; k++) {
            const uint32_t s = syms[k];
            if (!(s & 0x80000000u)) {
                bw->lt.freq[s & 0xFF]++;
            } else {
                bw->lt.freq[len_code(((s >> 16) & 0xFF) + 3) + LITERALS + 1]++;
                bw->dt.freq[dist_code((s & 0xFFFF) + 1)]++;
            }
        }
        bw->lt.freq[END_BLOCK] = 1;
        const BlockPlan pl = plan_block(*bw, b.b1 - b.b0, b.in_win != 0);
        if (report) {
            const uint32_t r[ZZ_BLOCK_WORDS] = {b.s0, b.s1, b.b0, b.b1, b.in_win, b.last, pl.type,
                                                (uint32_t)((pl.opt_len + 10) >> 3), (uint32_t)((pl.static_len + 10) >> 3),
                                                pl.max_blindex, tree_limited(bw->lt, L_CODES, MAX_BITS),
                                                tree_limited(bw->dt, D_CODES, MAX_BITS),
                                                tree_limited(bw->bt, BL_CODES, MAX_BL_BITS)};
            memcpy(report, r, sizeof r);
            report += ZZ_BLOCK_WORDS;
        }
        auto put = [&](uint32_t v, uint32_t n) { bo.put(v, n); };
        send_header(*bw, pl, b.last != 0, put);
        if (pl.type == BT_STORED) {
            bo.windup();
            const uint32_t len = b.b1 - b.b0;
            bo.put(len & 0xFFFF, 16);
            bo.put(~len & 0xFFFF, 16);
            for (uint32_t i = b.b0; i < b.b1; i++) bo.put(src[i], 8);
        } else {
            const bool st = pl.type == BT_STATIC;
            for (uint32_t k = b.s0; k < b.s1; k++) {
                const SymBits sb = sym_bits(syms[k], st, bw->lt.code, bw->lt.len, bw->dt.code, bw->dt.len);
                for (int j = 0; j < 4; j++) bo.put(sb.v[j], sb.n[j]);
            }
            bo.put(st ? static_lcode(END_BLOCK) : bw->lt.code[END_BLOCK], st ? 7u : bw->lt.len[END_BLOCK]);
        }
        if (b.last) bo.windup();
    }
    delete bw;
    return bo.over ? -1 : (int64_t)bo.n;
}

// The GPU's segment-parallel parse, emulated serially: every segment of `seg`
// positions parsed speculatively from a canonical start (pass 1, canonical
// loop tops marked in a bitmap), each segment's parse continued past its end
// until it reaches a canonical loop top the next segments' parses marked
// (pass 2), the true path stitched through the sync points, blocks cut by
// zz::block_rec.  Must equal zlib byte for byte for any `seg`.
struct SegParse {
    uint32_t nseg = 0, fin_src = 0, fallback = 0;  // fin_src: 0 none, 1 the last segment's pass 1, 2 a tail that ran to D
    std::vector<uint32_t> n1, nt, sync_q, into;    // per segment (sync_q NONE: the tail ran to D or the segment is the last)
    std::vector<uint32_t> syms, pos;               // the stitched stream
};
// `tailcap`: the kernel's DZ_TAILCAP, for the fallback flag alone (a tail that
// must take a step with tailcap - 1 symbols stored sends the chunk to the
// serial parse there; the model's tails go on, so the stitch is always there)
static SegParse seg_parse(const uint8_t* src, uint32_t D, int level, uint32_t seg, uint32_t tailcap) {
    using namespace zz;
    SegParse R;
    const Config cfg = level_config(level);
    std::vector<uint32_t> prev(D ? D : 1, NONE), head(1u << 15, NONE);
    for (uint32_t p = 0; p + MIN_MATCH <= D; p++) {
        const uint32_t h = hash3(src[p], src[p + 1], src[p + 2]);
        prev[p] = head[h];
        head[h] = p;
    }
    auto byte = [&](uint32_t i) -> uint32_t { return src[i]; };
    auto byte4 = [&](uint32_t i) -> uint32_t {
        uint32_t v;
        memcpy(&v, src + i, 4);
        return v;
    };
    auto pr = [&](uint32_t i) -> uint32_t { return prev[i]; };
    std::vector<Match2> g(D ? D : 1);
    for (uint32_t p = 0; p < D; p++) g[p] = search(p, D, cfg, byte4, byte, pr);
    auto get = [&](uint32_t p) -> Match2 { return g[p]; };
    const uint32_t nseg = D ? (D + seg - 1) / seg : 1;
    std::vector<std::vector<uint32_t>> sy(nseg), ps(nseg), ty(nseg), tp(nseg);
    std::vector<PState> end(nseg);
    std::vector<uint8_t> canon(D + 1, 0);
    std::vector<uint32_t> sync_q(nseg, NONE);
    std::vector<uint8_t> fin_lit(nseg, 0), tail_fin(nseg, 0);
    for (uint32_t k = 0; k < nseg; k++) {  // pass 1
        const uint32_t S0 = k * seg, S1 = (k + 1 == nseg) ? D : (k + 1) * seg;
        PState st = fresh_state(S0);
        auto em = [&](uint32_t s, uint32_t at) { sy[k].push_back(s); ps[k].push_back(at); };
        while (st.p < S1 && st.p < D) {
            if (canonical(st)) canon[st.p] = 1;
            step(st, D, cfg, get, byte, em);
        }
        if (k + 1 == nseg && st.avail) {  // Z_FINISH: the pending literal
            em(byte(st.p - 1), st.p - 1);
            st.avail = 0;
            fin_lit[k] = 1;
        }
        end[k] = st;
    }
    for (uint32_t k = 0; k + 1 < nseg; k++) {  // pass 2
        const uint32_t S1 = (k + 1) * seg;
        PState st = end[k];
        auto em = [&](uint32_t s, uint32_t at) { ty[k].push_back(s); tp[k].push_back(at); };
        while (true) {
            if (st.p >= D) {
                if (st.avail) {
                    em(byte(st.p - 1), st.p - 1);
                    tail_fin[k] = 1;
                }
                break;
            }
            if (st.p >= S1 && canonical(st) && canon[st.p]) {
                sync_q[k] = st.p;
                break;
            }
            if (ty[k].size() + 1 >= tailcap) R.fallback = 1;
            step(st, D, cfg, get, byte, em);
        }
    }
    std::vector<uint32_t>& syms = R.syms;
    std::vector<uint32_t>& pos = R.pos;
    R.nseg = nseg;
    R.into.assign(nseg, NONE);
    R.sync_q = sync_q;
    for (uint32_t k = 0; k < nseg; k++) {
        R.n1.push_back((uint32_t)sy[k].size());
        R.nt.push_back((uint32_t)ty[k].size());
        if (sync_q[k] != NONE) R.into[k] = sync_q[k] / seg;
    }
    uint32_t cur = 0, idx = 0;
    while (true) {
        for (uint32_t i = idx; i < sy[cur].size(); i++) { syms.push_back(sy[cur][i]); pos.push_back(ps[cur][i]); }
        if (cur + 1 == nseg) { R.fin_src = fin_lit[cur] ? 1u : 0u; break; }
        for (uint32_t i = 0; i < ty[cur].size(); i++) { syms.push_back(ty[cur][i]); pos.push_back(tp[cur][i]); }
        if (sync_q[cur] == NONE) { R.fin_src = tail_fin[cur] ? 2u : 0u; break; }
        const uint32_t q = sync_q[cur];
        const uint32_t nx = q / seg;
        uint32_t j = 0;
        while (j < ps[nx].size() && ps[nx][j] < q) j++;
        cur = nx;
        idx = j;
    }
    return R;
}

// The segment emulation's path: head[0..3] = nseg, final-literal source
// (0 none, 1 last segment, 2 a tail), fallback flag, stitched symbol count;
// per segment (4 u32 each, up to cap_seg segments): pass-1 symbols, tail
// symbols, sync position (NONE: ran to D), segment synced into (NONE).
extern "C" int32_t zz_host_report_seg(const uint8_t* src, uint32_t D, int level, uint32_t seg, uint32_t tailcap,
                                      uint32_t* head, uint32_t* per_seg, uint32_t cap_seg) {
    const SegParse R = seg_parse(src, D, level, seg, tailcap);
    head[0] = R.nseg, head[1] = R.fin_src, head[2] = R.fallback, head[3] = (uint32_t)R.syms.size();
    for (uint32_t k = 0; k < R.nseg && k < cap_seg; k++) {
        per_seg[4 * k] = R.n1[k], per_seg[4 * k + 1] = R.nt[k];
        per_seg[4 * k + 2] = R.sync_q[k], per_seg[4 * k + 3] = R.into[k];
    }
    return (int32_t)R.nseg;
}

// The block records zz::block_rec cuts from the stitched stream (what the GPU
// parse kernels store): s0, s1, b0, b1, in_win, last per block, 6 u32 each.
// The serial parse of zz_host_report_blocks tracks the window slides itself,
// so the two agree only if block_rec's flush top is right.
extern "C" int32_t zz_host_report_seg_blocks(const uint8_t* src, uint32_t D, int level, uint32_t seg, uint32_t* out,
                                             uint32_t cap_blocks) {
    using namespace zz;
    const SegParse R = seg_parse(src, D, level, seg, NONE);
    const uint32_t nsym = (uint32_t)R.syms.size(), nloop = nsym - (R.fin_src ? 1u : 0u);
    auto P = [&](uint32_t i) { return R.pos[i]; };
    auto Y = [&](uint32_t i) { return R.syms[i]; };
    const uint32_t nb = num_blocks(nloop);
    for (uint32_t k = 0; k < nb && k < cap_blocks; k++) {
        const BlockRec b = block_rec(k, nsym, nloop, D, P, Y);
        const uint32_t r[6] = {b.s0, b.s1, b.b0, b.b1, b.in_win, b.last};
        memcpy(out + 6 * k, r, sizeof r);
    }
    return (int32_t)nb;
}

extern "C" int64_t zz_host_deflate_seg(const uint8_t* src, uint32_t D, int level, uint32_t seg, uint8_t* out,
                                       uint64_t cap) {
    using namespace zz;
    const SegParse R = seg_parse(src, D, level, seg, NONE);
    const std::vector<uint32_t>& syms = R.syms;
    const std::vector<uint32_t>& pos = R.pos;
    const bool finlit = R.fin_src != 0;
    const uint32_t nsym = (uint32_t)syms.size(), nloop = nsym - (finlit ? 1u : 0u);
    auto P = [&](uint32_t i) { return pos[i]; };
    auto Y = [&](uint32_t i) { return syms[i]; };
    BitOut bo{out, cap};
    BlockWork* bw = new BlockWork;
    const uint32_t nb = num_blocks(nloop);
    for (uint32_t k = 0; k < nb; k++) {
        const BlockRec b = block_rec(k, nsym, nloop, D, P, Y);
        for (int i = 0; i < HEAP_SIZE; i++) bw->lt.freq[i] = 0;
        for (int i = 0; i < 2 * D_CODES + 1; i++) bw->dt.freq[i] = 0;
        for (uint32_t q = b.s0; q < b.s1; q++) {
            const uint32_t s = syms[q];
            if (!(s & 0x80000000u)) bw->lt.freq[s & 0xFF]++;
            else {
                bw->lt.freq[len_code(((s >> 16) & 0xFF) + 3) + LITERALS + 1]++;
                bw->dt.freq[dist_code((s & 0xFFFF) + 1)]++;
            }
        }
        bw->lt.freq[END_BLOCK] = 1;
        const BlockPlan pl = plan_block(*bw, b.b1 - b.b0, b.in_win != 0);
        auto put = [&](uint32_t v, uint32_t n) { bo.put(v, n); };
        send_header(*bw, pl, b.last != 0, put);
        if (pl.type == BT_STORED) {
            bo.windup();
            const uint32_t len = b.b1 - b.b0;
            bo.put(len & 0xFFFF, 16);
            bo.put(~len & 0xFFFF, 16);
            for (uint32_t i = b.b0; i < b.b1; i++) bo.put(src[i], 8);
        } else {
            const bool st = pl.type == BT_STATIC;
            for (uint32_t q = b.s0; q < b.s1; q++) {
                const SymBits sb = sym_bits(syms[q], st, bw->lt.code, bw->lt.len, bw->dt.code, bw->dt.len);
                for (int j = 0; j < 4; j++) bo.put(sb.v[j], sb.n[j]);
            }
            bo.put(st ? static_lcode(END_BLOCK) : bw->lt.code[END_BLOCK], st ? 7u : bw->lt.len[END_BLOCK]);
        }
        if (b.last) bo.windup();
    }
    delete bw;
    return bo.over ? -1 : (int64_t)bo.n;
}
