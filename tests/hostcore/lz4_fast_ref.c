/* TEST INFRASTRUCTURE ONLY: a serial restatement of liblz4 1.9.3's block
 * compressor as LZ4F calls it for lz4-rs's frames (lz.rs:85-92: level 0,
 * independent blocks), i.e. LZ4_compress_fast_extState_fastReset with
 * acceleration 1 on a cleared table, no dictionary, limitedOutput with
 * dstCapacity = srcSize - 1 (LZ4F_makeBlock stores the block raw when this
 * returns 0).  A block below LZ4_64Klimit (65 547 bytes) uses the byU16
 * table: 2^13 u16 entries, hash4 of 4 bytes, every candidate in range; a
 * larger one (lz4 blockSize 256K/1M/4M) the byU32 table: 2^12 u32 entries,
 * hash5 of 5 bytes, candidates more than 65 535 back skipped.
 * tests/test_hostcore.py checks it byte for byte against liblz4's own
 * LZ4_compress_fast; the GPU encoder (zcg_lz4_enc.hip) restates the same
 * steps with a wave-parallel search.  Never linked into the product.
 *
 * It follows liblz4's LZ4_compress_generic closely (its search order and
 * hash-table updates decide the bytes), so it carries liblz4's notice:
 *   LZ4 - Fast LZ compression algorithm.  Copyright (C) 2011-present, Yann
 *   Collet.  BSD 2-Clause License: Redistribution and use in source and
 *   binary forms, with or without modification, are permitted provided that
 *   the following conditions are met: * Redistributions of source code must
 *   retain the above copyright notice, this list of conditions and the
 *   following disclaimer.  * Redistributions in binary form must reproduce the
 *   above copyright notice, this list of conditions and the following
 *   disclaimer in the documentation and/or other materials provided with the
 *   distribution.  THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND
 *   CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT
 *   NOT LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR
 *   A PARTICULAR PURPOSE ARE DISCLAIMED.  IN NO EVENT SHALL THE COPYRIGHT
 *   OWNER OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL,
 *   SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT LIMITED
 *   TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR
 *   PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF
 *   LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING
 *   NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS
 *   SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
 * (Altered: a restatement, not liblz4's source.) */
#include <stdint.h>
#include <string.h>

typedef uint8_t u8;
typedef uint32_t u32;

#define MINMATCH 4
#define MFLIMIT 12
#define LASTLITERALS 5
#define LZ4_minLength (MFLIMIT + 1)
#define ML_BITS 4
#define ML_MASK 15u
#define RUN_MASK 15u
#define SKIP_TRIGGER 6
#define LZ4_64Klimit (65536 + MFLIMIT - 1)
#define DISTANCE_MAX 65535u

static u32 rd32(const u8* p) { u32 v; memcpy(&v, p, 4); return v; }
static uint64_t rd64(const u8* p) { uint64_t v; memcpy(&v, p, 8); return v; }
static int g_u32;  /* byU32 mode of the current block */
/* LZ4_hashPosition: hash4 (13 bits) for byU16, hash5 (12 bits) for byU32 */
static u32 hashp(const u8* p) {
    if (!g_u32) return (rd32(p) * 2654435761u) >> (32 - 13);
    return (u32)(((rd64(p) << 24) * 889523592379ull) >> (64 - 12));
}

/* LZ4_count: matching bytes of in and m, in < limit */
static u32 count(const u8* in, const u8* m, const u8* limit) {
    const u8* s = in;
    while (in < limit && *in == *m) { in++; m++; }
    return (u32)(in - s);
}

int zref_lz4_fast_block(const u8* src, int n, u8* dst, int cap) {
    static u32 table[1 << 13];
    memset(table, 0, sizeof(table));
    g_u32 = n >= LZ4_64Klimit;
    const u8* ip = src;
    const u8* anchor = src;
    const u8* const iend = src + n;
    const u8* const mflimitPlusOne = iend - MFLIMIT + 1;
    const u8* const matchlimit = iend - LASTLITERALS;
    u8* op = dst;
    u8* const olimit = dst + cap;
    if (n < LZ4_minLength) goto last_literals;
    table[hashp(ip)] = 0;  /* LZ4_putPosition(first byte) */
    ip++;
    u32 forwardH = hashp(ip);
    for (;;) {
        const u8* match;
        u8* token;
        {   /* find a match */
            const u8* forwardIp = ip;
            int step = 1;
            int searchMatchNb = 1 << SKIP_TRIGGER;
            for (;;) {
                const u32 h = forwardH;
                const u32 current = (u32)(forwardIp - src);
                const u32 matchIndex = table[h];
                ip = forwardIp;
                forwardIp += step;
                step = searchMatchNb++ >> SKIP_TRIGGER;
                if (forwardIp > mflimitPlusOne) goto last_literals;
                match = src + matchIndex;
                forwardH = hashp(forwardIp);
                table[h] = current;
                if (g_u32 && matchIndex + DISTANCE_MAX < current) continue;
                if (rd32(match) == rd32(ip)) break;
            }
        }
        /* catch up */
        while ((ip > anchor) & (match > src) && ip[-1] == match[-1]) { ip--; match--; }
        {   /* literals */
            const u32 lit = (u32)(ip - anchor);
            token = op++;
            if (op + lit + (2 + 1 + LASTLITERALS) + (lit / 255) > olimit) return 0;
            if (lit >= RUN_MASK) {
                u32 len = lit - RUN_MASK;
                *token = (u8)(RUN_MASK << ML_BITS);
                for (; len >= 255; len -= 255) *op++ = 255;
                *op++ = (u8)len;
            } else {
                *token = (u8)(lit << ML_BITS);
            }
            memcpy(op, anchor, lit);
            op += lit;
        }
    next_match:
        /* offset */
        op[0] = (u8)(ip - match);
        op[1] = (u8)((ip - match) >> 8);
        op += 2;
        {   /* match length */
            const u32 mc = count(ip + MINMATCH, match + MINMATCH, matchlimit);
            ip += mc + MINMATCH;
            if (op + (1 + LASTLITERALS) + (mc + 240) / 255 > olimit) return 0;
            if (mc >= ML_MASK) {
                u32 len = mc - ML_MASK;
                *token += ML_MASK;
                for (; len >= 510; len -= 510) { *op++ = 255; *op++ = 255; }
                if (len >= 255) { len -= 255; *op++ = 255; }
                *op++ = (u8)len;
            } else {
                *token += (u8)mc;
            }
        }
        anchor = ip;
        if (ip >= mflimitPlusOne) break;
        /* fill table */
        table[hashp(ip - 2)] = (u32)(ip - 2 - src);
        {   /* test next position */
            const u32 h = hashp(ip);
            const u32 current = (u32)(ip - src);
            const u32 matchIndex = table[h];
            match = src + matchIndex;
            table[h] = current;
            if ((!g_u32 || matchIndex + DISTANCE_MAX >= current) && rd32(match) == rd32(ip)) {
                token = op++;
                *token = 0;
                goto next_match;
            }
        }
        forwardH = hashp(++ip);
    }
last_literals:
    {
        const u32 last = (u32)(iend - anchor);
        if (op + last + 1 + ((last + 255 - RUN_MASK) / 255) > olimit) return 0;
        if (last >= RUN_MASK) {
            u32 acc = last - RUN_MASK;
            *op++ = (u8)(RUN_MASK << ML_BITS);
            for (; acc >= 255; acc -= 255) *op++ = 255;
            *op++ = (u8)acc;
        } else {
            *op++ = (u8)(last << ML_BITS);
        }
        memcpy(op, anchor, last);
        op += last;
    }
    return (int)(op - dst);
}

/* ---- the same block with a path report (tests/lz4_enc_cases.py) -----------------
 * zref_lz4_fast_block_report writes the bytes of zref_lz4_fast_block and fills
 *   rep[ZR_N]   counters of the serial path and of the GPU kernel's batches,
 *   seq[][7]    one row per sequence that has a match: position of the match
 *               (after catch-up), literal length, match length field (length
 *               - 4), offset, 1 for a rematch through next_match, bytes of
 *               catch-up, the search attempt that found it.
 * The batch counters restate le_block's search (zcg_lz4_enc.hip) from its text:
 * 64 attempts k0 .. k0 + 63 laid out on the step schedule, V of them with
 * nxt <= mflimitPlusOne, g the smallest lane of any hash shared inside the
 * batch, P = min(g + 1, V) lanes compared, the table left as attempts 0 .. m
 * leave it.  The restatement runs on a table of its own beside the serial
 * search; ZR_EMU_DIFF counts the searches whose outcome differs (and a final
 * table that differs): it must be 0.  The counters, in the order of
 * REP_FIELDS in tests/lz4_enc_cases.py: table mode; exit (ZX_*: how the block
 * ended; ZR_LOOP_END keeps how the loop ended when the last literals then do
 * not fit); size; sequences; largest attempt; longest catch-up; catch-ups that
 * stopped at anchor / at the block's start; rematches; candidates skipped for
 * distance in the search / of those with equal 4 bytes / the same two at the
 * next-position test; matches at distance 65 535; largest literal length and
 * how many had (x - 15) % 255 == 0; the same for match length fields; last
 * literals; matches that ended at matchlimit; highest position put into the
 * table.  Batches: searches; batches; batches with P < V; of those with
 * g == 0; matches at w == P - 1 of a cut batch; matches at a position an
 * earlier batch had laid out behind its cut (deferred); lanes behind a cut
 * whose table value of before the batch matches their 4 bytes while their
 * serial candidate does not (stale), and of those in a batch with g == 0;
 * batches with V < 64; with two step sizes; holding attempts 64 and 65; 128
 * and 129; searches with V == 0 at their first batch. */
enum {
    ZR_MODE, ZR_EXIT, ZR_LOOP_END, ZR_SIZE, ZR_NSEQ, ZR_MAX_ATTEMPT, ZR_MAX_CATCHUP, ZR_CATCH_ANCHOR, ZR_CATCH_SRC,
    ZR_REMATCH, ZR_FAR_SEARCH, ZR_FAR_SEARCH_EQ, ZR_FAR_NEXT, ZR_FAR_NEXT_EQ, ZR_DIST_MAX, ZR_MAX_LIT, ZR_LIT_255,
    ZR_MAX_ML, ZR_ML_255, ZR_LAST_LIT, ZR_AT_MATCHLIMIT, ZR_MAX_TAB,
    ZR_SEARCHES, ZR_BATCHES, ZR_CUT, ZR_G0, ZR_W_AT_CUT, ZR_DEFERRED, ZR_STALE, ZR_STALE_G0, ZR_VSHORT, ZR_TWO_STEPS, ZR_X64, ZR_X128,
    ZR_V0_FIRST, ZR_EMU_DIFF, ZR_N
};
/* ZR_EXIT */
enum { ZX_SEARCH_END, ZX_MATCH_END, ZX_RET0_LIT, ZX_RET0_ML, ZX_RET0_LAST };
#define ZR_LANES 64

static u32 e_stamp[1 << 13], e_bid;
static u8 e_first[1 << 13], e_last[1 << 13];

static int e_test(const u8* src, u32 c, u32 p) {
    return (!g_u32 || c + DISTANCE_MAX >= p) && rd32(src + c) == rd32(src + p);
}

/* one search of le_block from position ip on table T; returns 1 and the match
 * (position, candidate, attempt) or 0 when the search runs out */
static int e_search(const u8* src, u32* T, u32 ip, u32 mfl1, u32* rep, u32* mpos, u32* mref, u32* matt) {
    u32 s0 = ip, k0 = 0, laid = 0;
    int first = 1;
    rep[ZR_SEARCHES]++;
    for (;;) {
        u32 pos[ZR_LANES], nxt[ZR_LANES], st[ZR_LANES], h[ZR_LANES], old[ZR_LANES];
        int prev[ZR_LANES];
        u32 V = 0, s = s0, g = ZR_LANES, P, w = ZR_LANES, m, j;
        for (j = 0; j < ZR_LANES; j++) {
            const u32 k = k0 + j;
            st[j] = k == 0 ? 1u : (63u + k) >> 6;
            pos[j] = s;
            s += st[j];
            nxt[j] = s;
            if (nxt[j] <= mfl1) V = j + 1;  /* (a prefix of the lanes) */
        }
        if (!V) {
            if (first) rep[ZR_V0_FIRST]++;
            return 0;
        }
        first = 0;
        rep[ZR_BATCHES]++;
        e_bid++;
        for (j = 0; j < V; j++) {
            h[j] = hashp(src + pos[j]);
            old[j] = T[h[j]];
            prev[j] = -1;
            if (e_stamp[h[j]] == e_bid) {
                prev[j] = e_last[h[j]];
                if (e_first[h[j]] < g) g = e_first[h[j]];
            } else {
                e_stamp[h[j]] = e_bid;
                e_first[h[j]] = (u8)j;
            }
            e_last[h[j]] = (u8)j;
        }
        P = g + 1 < V ? g + 1 : V;
        for (j = 0; j < P; j++)
            if (e_test(src, old[j], pos[j])) { w = j; break; }
        /* the serial attempts on this layout: the lanes behind the cut whose
         * table value of before the batch would have matched, though the
         * candidate an earlier lane of the batch leaves there does not */
        for (j = 0; j < V; j++) {
            const u32 cand = prev[j] >= 0 ? pos[prev[j]] : old[j];
            const int sm = e_test(src, cand, pos[j]);
            if (j >= P && prev[j] >= 0 && !sm && e_test(src, old[j], pos[j])) {
                rep[ZR_STALE]++;
                if (g == 0) rep[ZR_STALE_G0]++;
            }
            if (sm) break;
        }
        if (P < V) rep[ZR_CUT]++;
        if (P < V && g == 0) rep[ZR_G0]++;
        if (V < ZR_LANES) rep[ZR_VSHORT]++;
        if (st[0] != st[V - 1]) rep[ZR_TWO_STEPS]++;
        if (k0 <= 64 && k0 + V - 1 >= 65) rep[ZR_X64]++;     /* attempts 64 (step 1) and 65 (step 2) */
        if (k0 <= 128 && k0 + V - 1 >= 129) rep[ZR_X128]++;  /* attempts 128 (step 2) and 129 (step 3) */
        m = w < ZR_LANES ? w : P - 1;
        for (j = 0; j <= m; j++) T[h[j]] = pos[j];
        if (w < ZR_LANES) {
            if (P < V && w == P - 1) rep[ZR_W_AT_CUT]++;
            if (pos[w] <= laid && laid) rep[ZR_DEFERRED]++;
            *mpos = pos[w];
            *mref = old[w];
            *matt = k0 + w;
            return 1;
        }
        if (P == V && V < ZR_LANES) return 0;
        if (pos[V - 1] > laid) laid = pos[V - 1];
        s0 = nxt[P - 1];
        k0 += P;
    }
}

static void zr_len(u32* rep, int kmax, int k255, u32 x) {
    if (x > rep[kmax]) rep[kmax] = x;
    if (x >= 15 && (x - 15) % 255 == 0) rep[k255]++;
}

int zref_lz4_fast_block_report(const u8* src, int n, u8* dst, int cap, u32* rep, u32* seq, int seqcap) {
    static u32 table[1 << 13], etab[1 << 13];
    memset(table, 0, sizeof(table));
    memset(etab, 0, sizeof(etab));
    memset(e_stamp, 0, sizeof(e_stamp));
    memset(rep, 0, ZR_N * sizeof(u32));
    e_bid = 0;
    g_u32 = n >= LZ4_64Klimit;
    rep[ZR_MODE] = (u32)g_u32;
    const u8* ip = src;
    const u8* anchor = src;
    const u8* const iend = src + n;
    const u8* const mflimitPlusOne = iend - MFLIMIT + 1;
    const u8* const matchlimit = iend - LASTLITERALS;
    u8* op = dst;
    u8* const olimit = dst + cap;
    int ret = 0;
    rep[ZR_LOOP_END] = ZX_SEARCH_END;
    if (n < LZ4_minLength) goto last_literals;
    table[hashp(ip)] = 0;
    ip++;
    u32 forwardH = hashp(ip);
    for (;;) {
        const u8* match;
        u8* token;
        u32 att = 0, kind = 0;
        {   /* the kernel's search on its own table, then the serial one */
            u32 empos = 0, emref = 0, ematt = 0;
            const int efound = e_search(src, etab, (u32)(ip - src), (u32)(mflimitPlusOne - src), rep, &empos, &emref,
                                        &ematt);
            const u8* forwardIp = ip;
            int step = 1, found = 0;
            int searchMatchNb = 1 << SKIP_TRIGGER;
            for (;; att++) {
                const u32 h = forwardH;
                const u32 current = (u32)(forwardIp - src);
                const u32 matchIndex = table[h];
                ip = forwardIp;
                forwardIp += step;
                step = searchMatchNb++ >> SKIP_TRIGGER;
                if (forwardIp > mflimitPlusOne) break;
                if (att > rep[ZR_MAX_ATTEMPT]) rep[ZR_MAX_ATTEMPT] = att;
                match = src + matchIndex;
                forwardH = hashp(forwardIp);
                table[h] = current;
                if (current > rep[ZR_MAX_TAB]) rep[ZR_MAX_TAB] = current;
                if (g_u32 && matchIndex + DISTANCE_MAX < current) {
                    rep[ZR_FAR_SEARCH]++;
                    if (rd32(match) == rd32(ip)) rep[ZR_FAR_SEARCH_EQ]++;
                    continue;
                }
                if (rd32(match) == rd32(ip)) { found = 1; break; }
            }
            if (found != efound ||
                (found && (empos != (u32)(ip - src) || emref != (u32)(match - src) || ematt != att)))
                rep[ZR_EMU_DIFF]++;
            if (!found) goto last_literals;
        }
        /* catch up */
        {
            const u8* const ip0 = ip;
            while ((ip > anchor) & (match > src) && ip[-1] == match[-1]) { ip--; match--; }
            const u32 cu = (u32)(ip0 - ip);
            if (cu > rep[ZR_MAX_CATCHUP]) rep[ZR_MAX_CATCHUP] = cu;
            if (cu && ip == anchor) rep[ZR_CATCH_ANCHOR]++;
            if (cu && match == src) rep[ZR_CATCH_SRC]++;
            if (seq && (int)rep[ZR_NSEQ] < seqcap) seq[7 * rep[ZR_NSEQ] + 5] = cu;
        }
        {   /* literals */
            const u32 lit = (u32)(ip - anchor);
            token = op++;
            if (op + lit + (2 + 1 + LASTLITERALS) + (lit / 255) > olimit) { rep[ZR_EXIT] = ZX_RET0_LIT; goto done; }
            zr_len(rep, ZR_MAX_LIT, ZR_LIT_255, lit);
            if (lit >= RUN_MASK) {
                u32 len = lit - RUN_MASK;
                *token = (u8)(RUN_MASK << ML_BITS);
                for (; len >= 255; len -= 255) *op++ = 255;
                *op++ = (u8)len;
            } else {
                *token = (u8)(lit << ML_BITS);
            }
            memcpy(op, anchor, lit);
            op += lit;
        }
    next_match_r:
        if ((u32)(ip - match) == DISTANCE_MAX) rep[ZR_DIST_MAX]++;
        op[0] = (u8)(ip - match);
        op[1] = (u8)((ip - match) >> 8);
        op += 2;
        {   /* match length */
            const u32 mc = count(ip + MINMATCH, match + MINMATCH, matchlimit);
            if (seq && (int)rep[ZR_NSEQ] < seqcap) {
                u32* r = seq + 7 * rep[ZR_NSEQ];
                r[0] = (u32)(ip - src); r[1] = (u32)(ip - anchor); r[2] = mc; r[3] = (u32)(ip - match);
                r[4] = kind; r[6] = att;
                if (kind) r[5] = 0;
            }
            ip += mc + MINMATCH;
            if (op + (1 + LASTLITERALS) + (mc + 240) / 255 > olimit) { rep[ZR_EXIT] = ZX_RET0_ML; goto done; }
            rep[ZR_NSEQ]++;
            zr_len(rep, ZR_MAX_ML, ZR_ML_255, mc);
            if (ip == matchlimit) rep[ZR_AT_MATCHLIMIT]++;
            if (mc >= ML_MASK) {
                u32 len = mc - ML_MASK;
                *token += ML_MASK;
                for (; len >= 510; len -= 510) { *op++ = 255; *op++ = 255; }
                if (len >= 255) { len -= 255; *op++ = 255; }
                *op++ = (u8)len;
            } else {
                *token += (u8)mc;
            }
        }
        anchor = ip;
        if (ip >= mflimitPlusOne) { rep[ZR_LOOP_END] = ZX_MATCH_END; break; }
        /* fill table */
        {
            const u32 h2 = hashp(ip - 2), p2 = (u32)(ip - 2 - src);
            table[h2] = p2;
            etab[h2] = p2;
            if (p2 > rep[ZR_MAX_TAB]) rep[ZR_MAX_TAB] = p2;
        }
        {   /* test next position */
            const u32 h = hashp(ip);
            const u32 current = (u32)(ip - src);
            const u32 matchIndex = table[h];
            match = src + matchIndex;
            table[h] = current;
            etab[h] = current;
            if (current > rep[ZR_MAX_TAB]) rep[ZR_MAX_TAB] = current;
            if (g_u32 && matchIndex + DISTANCE_MAX < current) {
                rep[ZR_FAR_NEXT]++;
                if (rd32(match) == rd32(ip)) rep[ZR_FAR_NEXT_EQ]++;
            } else if (rd32(match) == rd32(ip)) {
                token = op++;
                *token = 0;
                rep[ZR_REMATCH]++;
                kind = 1;
                goto next_match_r;
            }
        }
        forwardH = hashp(++ip);
    }
last_literals:
    {
        const u32 last = (u32)(iend - anchor);
        rep[ZR_LAST_LIT] = last;
        if (op + last + 1 + ((last + 255 - RUN_MASK) / 255) > olimit) { rep[ZR_EXIT] = ZX_RET0_LAST; goto done; }
        rep[ZR_EXIT] = rep[ZR_LOOP_END];
        if (last >= RUN_MASK) {
            u32 acc = last - RUN_MASK;
            *op++ = (u8)(RUN_MASK << ML_BITS);
            for (; acc >= 255; acc -= 255) *op++ = 255;
            *op++ = (u8)acc;
        } else {
            *op++ = (u8)(last << ML_BITS);
        }
        memcpy(op, anchor, last);
        op += last;
    }
    ret = (int)(op - dst);
    if (memcmp(table, etab, sizeof(table))) rep[ZR_EMU_DIFF]++;
done:
    rep[ZR_SIZE] = (u32)ret;
    return ret;
}
