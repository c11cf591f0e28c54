"""Directed blocks for the GPU LZ4 encoder (zcg_lz4_enc.hip).  TEST INFRASTRUCTURE ONLY.

The encoder's promise is liblz4's frame.  Generic payloads decide by accident
which branches of le_block write it: the batch of 64 search attempts and its
cut behind the first shared hash, the table mode, the distance limit at its
two sites, catch-up 64 bytes at a time, the three return-0 sites, put_len,
LZ4_count's lanes.  A search that is wrong in one of them writes a stream
that still decodes.  Each case here is one batch of equal-length chunks and a
block-size parameter, built to reach one of those branches, with a WITNESS:
a statement over the path report of the CPU model (tests/hostcore/
lz4_fast_ref.c: zref_lz4_fast_block_report) that it does.  The report counts
what the serial compressor does (exit, sequences, attempts, catch-up,
rematches, distance skips, length fields) and restates the kernel's batches
from its text: lanes k0 .. k0 + 63 on the step schedule, the lanes behind a
match included, V from nxt <= mflimitPlusOne, g the smallest lane of any hash
shared inside the batch, P = min(g + 1, V).  `stale` counts the lanes behind
a cut whose table value of before the batch matches their 4 bytes while their
serial candidate does not: the case the cut exists for.

tests/test_lz4_enc_cases_host.py asserts every witness, that the model's
bytes are liblz4's LZ4_compress_fast(.., n - 1, 1) for every block, and that
the restated batches find what the serial search finds; tests/
test_gpu_lz4_enc_craft.py encodes the same batches on the GPU and compares
every frame with liblz4's.

Two cases hold a block of 262 144 bytes (mode_tail_*): a tail block of
65 546 / 65 547 bytes behind a full one needs it; that block is text, one
match long.  Catch-up of exactly 64 or 128 bytes is not built: where the
search lands inside a copy follows from the whole step history, so the
catch-up case (6 522 bytes: 101 full steps of the `c == 64` loop and a part)
was found by trying, as were the literal runs above 64 bytes (Runs.seq_exact).

NOT REACHED (no case: a test here must not pass vacuously)

  (none of the mandatory classes)
"""
import ctypes
import functools

import numpy as np

MFLIMIT, LASTLIT, LIMIT64K, LANES = 12, 5, 65536 + 12 - 1, 64   # zcg_lz4_enc.hip (pinned by test_lz4_enc_cases_host.py)
DIST_MAX = 65535

REP_FIELDS = ("mode", "exit", "loop_end", "size", "nseq", "max_attempt", "max_catchup", "catch_anchor", "catch_src",
              "rematch", "far_search", "far_search_eq", "far_next", "far_next_eq", "dist_max", "max_lit", "lit_255",
              "max_ml", "ml_255", "last_lit", "at_matchlimit", "max_tab",
              "searches", "batches", "cut", "g0", "w_at_cut", "deferred", "stale", "stale_g0", "vshort", "two_steps",
              "x64", "x128", "v0_first", "emu_diff")
SEARCH_END, MATCH_END, RET0_LIT, RET0_ML, RET0_LAST = range(5)   # Rep.exit


def step(k):
    """The step behind search attempt k (le_block: `k == 0 ? 1u : (63u + k) >> 6`)."""
    return 1 if k == 0 else (63 + k) >> 6


def eff_block(B):
    return 65536 if B <= 65536 else 262144 if B <= 262144 else 1048576 if B <= 1048576 else 4194304


def _host():
    from test_hostcore import host
    h = host()
    h.zref_lz4_fast_block_report.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    h.zref_lz4_fast_block_report.restype = ctypes.c_int
    return h


class Rep:
    """The path report of one block: REP_FIELDS, `out` (the model's bytes, b""
    when it returns 0: the block is stored), `S`, and `seq`: per sequence with
    a match (position, literals, match length - 4, offset, rematch, catch-up,
    attempt)."""

    def __init__(self, S, ret, out, rep, seq):
        self.S, self.ret, self.out, self.seq = S, ret, out, seq
        for k, v in zip(REP_FIELDS, rep):
            setattr(self, k, int(v))
        self.stored = ret == 0

    def __repr__(self):
        return "Rep(S=%d, " % self.S + ", ".join(f"{k}={getattr(self, k)}" for k in REP_FIELDS) + ")"

    def lits(self):
        return [r[1] for r in self.seq if not r[4]]

    def mls(self):
        return [r[2] for r in self.seq]

    def chains(self):
        """Lengths of the runs of matches joined by next_match (1: no rematch)."""
        out = []
        for r in self.seq:
            if r[4]:
                out[-1] += 1
            else:
                out.append(1)
        return out


@functools.lru_cache(maxsize=256)
def report(block):
    n = len(block)
    a = np.frombuffer(block, np.uint8) if n else np.zeros(1, np.uint8)
    out = np.zeros(n + 64, np.uint8)
    rep = np.zeros(len(REP_FIELDS), np.uint32)
    cap = n // 4 + 4
    seq = np.zeros((cap, 7), np.uint32)
    ret = _host().zref_lz4_fast_block_report(a.ctypes.data, n, out.ctypes.data, max(n - 1, 0), rep.ctypes.data,
                                             seq.ctypes.data, cap)
    ns = int(rep[REP_FIELDS.index("nseq")])
    assert ns <= cap
    return Rep(n, ret, out[:max(ret, 0)].tobytes(), rep, [tuple(int(x) for x in r) for r in seq[:ns]])


def blocks_of(chunk, B):
    e = eff_block(B)
    return [chunk[i:i + e] for i in range(0, len(chunk), e)]


def reports(chunk, B):
    return [report(b) for b in blocks_of(chunk, B)]


# ---- payload pieces ------------------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def walk(n, seed):
    """A +-3 walk of little-endian i16: short matches and rematches everywhere."""
    return np.cumsum(np.random.default_rng(seed).integers(-3, 4, n // 2 + 1)).astype("<i2").tobytes()[:n]


def text(n):
    return (b"the quick brown fox jumps over the lazy dog %d\n" * (n // 40 + 2))[:n]


def hash4(w):
    return ((int.from_bytes(w[:4], "little") * 2654435761) & 0xFFFFFFFF) >> 19


def hash5(w):
    return ((((int.from_bytes(w[:5], "little") << 24) & (2 ** 64 - 1)) * 889523592379) & (2 ** 64 - 1)) >> 52


def colliding(target, hf, n, seed):
    """n random bytes with the hash of `target` and other first 4 bytes (brute force)."""
    rng = np.random.default_rng(seed)
    while True:
        w = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if hf(w) == hf(target) and w[:4] != target[:4]:
            return w


class Runs:
    """A block of noise literals and runs of one byte value.  The first byte
    of a run is a literal; on a step of 1 (fewer than 65 literals) the search
    finds the run one attempt later at offset 1, so seq(lit, mc) is a sequence
    of exactly `lit` literals and a match whose length field is `mc`."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.a = bytearray()
        self.v = 0

    def lits(self, n, avoid=()):
        """n noise bytes: the first differs from the byte before, none of the ends is in `avoid`."""
        b = bytearray(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        bad = set(avoid) | ({self.a[-1]} if self.a else set())
        for k in ((0, n - 1) if n else ()):
            while b[k] in bad:
                b[k] = int(self.rng.integers(0, 256))
        self.a += b
        return self

    def seq(self, lit, mc):
        assert lit >= 1 and mc >= 0
        self.v = self.v % 255 + 1
        self.lits(lit - 1, (self.v,))
        self.a += bytes([self.v]) * (mc + 5)
        return self

    def seq_exact(self, lit, mc):
        """The same after more than 64 literals, where the search's step s is
        above 1: the run is met at its s-th byte (offset s), so it gets s - 1
        bytes more and the noise as many fewer; found by trying."""
        state = (bytes(self.a), self.v, self.rng.bit_generator.state)
        for s in range(1, 64):
            self.a, self.v = bytearray(state[0]), state[1]
            self.rng.bit_generator.state = state[2]
            self.v = self.v % 255 + 1
            self.lits(lit - s, (self.v,))
            self.a += bytes([self.v]) * (mc + 4 + s)
            row = report(bytes(self.a) + b"\0" + noise(12, 1))
            if row.seq and row.seq[-1][1:3] == (lit, mc):
                return self
        raise AssertionError((lit, mc))

    def bytes(self):
        return bytes(self.a)


class Case:
    """name, the LZ4 block-size parameter B, equal-length chunks, a witness
    over the reports; `short`: {chunk index: src_len below D} (refused chunks);
    `raw`: what a bool array holds where the stream holds 0 / 1."""

    def __init__(self, name, B, chunks, witness, short=None, raw=None):
        self.name, self.B, self.chunks, self.witness, self.short, self.raw = name, B, list(chunks), witness, \
            short or {}, raw
        self.D = len(self.chunks[0])

    def reps(self, i):
        return reports(self.chunks[i], self.B)

    def is_bits(self):
        return self.D > 0 and all(max(x) <= 1 for x in self.chunks)


def one(c, i=0):
    """The report of chunk i, which is one block."""
    r, = c.reps(i)
    return r


# ======== 1: a stale candidate excluded by the cut ===========================================
def _stale(mode, g0):
    """Words A and B of one hash, A at position 10.  The second batch of the
    first search (attempts 64 .., positions 65 ..) has B at lane 5 (g0: lane 0)
    and A at lane 15: that lane's table value of before the batch is position
    10, which matches its 4 bytes, while the serial candidate is B's position,
    which does not.  The cut behind B's lane keeps the lane out; with P = V it
    would report a match liblz4 does not have.  `stored`: noise alone, liblz4
    returns 0; else a zero run follows and the block is compressed."""
    hf, n = (hash5, 5) if mode else (hash4, 4)
    pb = 65 if g0 else 70
    chunks = []
    for stored in ((True, False) if not mode else (False,)):
        for seed in range(100 + 10 * mode + g0, 10000, 20):
            a = bytearray(noise(166 if stored else 400, seed))
            A = colliding(bytes(a[pb:pb + n]), hf, n, seed + 1000)
            a[10:10 + n] = A
            a[80:80 + n] = A
            if not stored:
                a[200:] = bytes((66000 if mode else 400) - 200)
            r = report(bytes(a))
            if r.stale == 1 and r.stored == stored and r.stale_g0 == g0:
                break
        else:
            raise AssertionError("no such block")
        chunks.append(bytes(a))
    if not mode:   # (one D per case: the 166-byte block on its own)
        chunks = chunks[1:] if g0 else chunks

    def witness(c):
        for i in range(len(c.chunks)):
            r = one(c, i)
            assert r.mode == mode and r.stale == 1 and r.stale_g0 == g0 and r.cut >= 1, r
            assert r.seq == [] or r.seq[0][0] > 200, r.seq   # no match at the stale lane
        return True
    return chunks, witness


def _class1():
    out = []
    (stored, comp), w = _stale(0, 0)
    out.append(Case("stale_u16_stored", 65536, [stored], lambda c: w(c) and one(c).stored))
    out.append(Case("stale_u16", 65536, [comp], lambda c: w(c) and not one(c).stored))
    ch, w0 = _stale(0, 1)
    out.append(Case("stale_u16_g0", 65536, ch, lambda c: w0(c) and not one(c).stored))
    for g0 in (0, 1):
        ch, w1 = _stale(1, g0)
        out.append(Case("stale_u32" + ("_g0" if g0 else ""), 262144, ch,
                        (lambda w1: lambda c: w1(c) and not one(c).stored and one(c).mode == 1)(w1)))
    return out


# ======== 2: cut batches on compressible data ===================================================
def _class2():
    D = 20000
    w = walk(D - 40, 200) + noise(40, 204)
    # a search of more than 130 attempts over noise, then the walk
    straddle = noise(330, 201) + w[330:]
    # the last match ends at mflimitPlusOne - 1 and the next position does not
    # match: the next search has no valid attempt (V = 0 at its first batch)
    N = noise(28, 202)
    v0 = w[:D - 60] + N + N[4:24] + noise(12, 203)
    chunks = [w, straddle, v0]

    def witness(c):
        a, s, z = (one(c, i) for i in range(3))
        assert not (a.stored or s.stored or z.stored)
        assert a.cut > 100 and a.deferred >= 1 and a.w_at_cut >= 1 and a.g0 >= 1, a
        assert a.vshort >= 1 and a.exit == SEARCH_END, a       # the last batch of the last search
        assert s.x64 >= 1 and s.x128 >= 1 and s.max_attempt >= 130, s
        assert z.v0_first == 1 and z.seq[-1][0] + 4 + z.seq[-1][2] == c.D - MFLIMIT, (z, z.seq[-1])
        return True
    return [Case("cut_batches", 65536, chunks, witness)]


def _bits():
    """Random 0 / 1 bytes: 16 different words, so nearly every batch is cut at
    once (and the chunk runs as a bool array on the GPU)."""
    rng = np.random.default_rng(210)
    bits = rng.integers(0, 2, 8192).astype(np.uint8)
    raw = np.where(bits == 0, 0, rng.choice(np.array([1, 2, 255], np.uint8), bits.size)).astype(np.uint8)

    def witness(c):
        r = one(c)
        assert c.is_bits() and (np.frombuffer(c.raw[0], np.uint8) != 0).astype(np.uint8).tobytes() == c.chunks[0]
        assert not r.stored and r.g0 >= 10 and r.rematch > 100, r
        return True
    return [Case("bits", 65536, [bits.tobytes()], witness, raw=[raw.tobytes()])]


# ======== 3: the 65 535 distance limit ==========================================================
def _class3():
    """byU32 blocks: 40 noise bytes, a 24-byte marker, zeros, the marker again
    d bytes behind the first, 3 000 noise bytes.  The zero run's match ends at
    the second marker, so the next-position test meets the first marker as its
    candidate: a rematch at d <= 65 535, skipped beyond.  `search`: two noise
    bytes in front of the second marker, so the search meets it instead."""
    out = []
    for search in (0, 1):
        for d in (65534, 65535, 65536, 65537):
            mk = noise(24, 300)
            gap = noise(2, 303) if search else b""
            a = noise(40, 301) + mk + bytes(d - 24 - len(gap)) + gap + mk + noise(3000, 302)

            def witness(c, d=d, search=search):
                r = one(c)
                far = d > DIST_MAX
                assert r.mode == 1 and not r.stored and r.nseq == (1 if far else 2), r
                assert r.dist_max == (d == DIST_MAX), r
                if search:
                    assert r.rematch == 0 and (r.far_search_eq >= 1) == far and r.far_next_eq == 0, r
                else:
                    assert r.rematch == (0 if far else 1) and r.far_next_eq == (1 if far else 0), r
                if not far:
                    assert r.seq[1][3] == d and r.seq[1][2] == 20, r.seq
                return True
            out.append(Case(f"distance_{'search' if search else 'next'}_{d}", 262144, [a], witness))
    return out


# ======== 4: the table mode goes by the block's length ==========================================
def _class4():
    out = []
    for S in (65535, 65536, 65546, 65547, 65548):
        chunks = [walk(S, 400 + S % 100), text(S)]

        def witness(c, S=S):
            for i in range(2):
                r = one(c, i)
                assert r.S == S and r.mode == (S >= LIMIT64K) and not r.stored and r.emu_diff == 0, r
            assert S != 65546 or one(c, 0).max_tab >= 65000
            assert one(c, 0).cut > 1000
            return True
        for B in (262144, 1048576):
            out.append(Case(f"mode_{S}_{B >> 10}k", B, chunks, witness))
    for S in (65546, 65547):
        chunk = text(262144) + walk(S, 450 + S % 100)

        def witness_tail(c, S=S):
            full, tail = c.reps(0)
            assert full.S == 262144 and full.mode == 1 and not full.stored
            assert tail.S == S and tail.mode == (S >= LIMIT64K) and not tail.stored and tail.cut > 1000, tail
            assert S != 65546 or tail.max_tab >= 65000, tail
            return True
        out.append(Case(f"mode_tail_{S}", 262144, [chunk], witness_tail))
    return out


# ======== 5: catch-up ============================================================================
def _class5():
    b = bytearray(noise(150000, 500))
    b += b[125000:148000]

    def witness_long(c):
        r = one(c)
        assert r.mode == 1 and not r.stored and r.max_catchup > 128 and r.max_attempt > 4000, r
        return True
    # a copy of the block's first bytes met on a step of 25: caught up to the block's start
    s = bytearray(noise(20000, 501))
    s += s[0:200] + noise(56, 502)

    def witness_src(c):
        r = one(c)
        assert not r.stored and r.catch_src == 1 and r.seq[0][3] == r.seq[0][0] and r.seq[0][5] >= 1, r.seq
        return True

    def witness_anchor(c):
        r = one(c)
        assert not r.stored and r.catch_anchor >= 1 and any(x[1] == 0 and not x[4] for x in r.seq), r
        return True
    w = walk(20256, 504)
    return [Case("catchup_6522", 262144, [bytes(b)], witness_long), Case("catchup_src", 65536, [bytes(s)], witness_src),
            Case("catchup_anchor", 65536, [w], witness_anchor)]


# ======== 6: exits ================================================================================
def _tail_copy(lit, S, seed):
    """`lit` noise bytes, then a copy from offset 100 up to S."""
    b = bytearray(noise(lit, seed))
    while len(b) < S:
        b.append(b[100 + len(b) - lit])
    return bytes(b)


def _lit_edge(S, seed=60):
    """3 062 literals, a 17-byte copy of bytes 20 .., 5 noise bytes (S = 3 084:
    every check passes with nothing to spare); one match byte fewer (3 083)."""
    L = 3062
    a = bytearray(noise(L, seed))
    a += a[20:20 + 3084 - L - 5] + noise(5, seed + 100)
    return bytes(a) if S == 3084 else bytes(a[:3084 - 6] + a[3084 - 5:])


def _last_edge(T):
    return noise(20, 62) + b"\x07" * 12 + noise(T, 63)


def _class6():
    def ex(want, size_is_cap=False):
        def witness(c):
            for i in range(len(c.chunks)):
                r = one(c, i)
                assert r.exit == want and r.stored == (want >= RET0_LIT), r
                assert not size_is_cap or r.size == c.D - 1, r
            return True
        return witness
    out = [Case("exit_ret0_lit_5228", 65536, [_tail_copy(5200, 5228, 50)], ex(RET0_LIT)),
           Case("exit_ret0_lit_3083", 65536, [_lit_edge(3083)], ex(RET0_LIT)),
           Case("exit_lit_fits_3084", 65536, [_lit_edge(3084)], ex(MATCH_END, True)),
           Case("exit_ret0_ml_5230", 65536, [_tail_copy(5200, 5230, 50)], ex(RET0_ML)),
           Case("exit_ret0_ml_5231", 65536, [_tail_copy(5200, 5231, 50)], ex(RET0_ML)),
           Case("exit_ml_fits_5232", 65536, [_tail_copy(5200, 5232, 50)], ex(MATCH_END, True)),
           Case("exit_ret0_last_5232", 65536, [_tail_copy(5210, 5232, 50)], ex(RET0_LAST)),
           Case("exit_ret0_last_1322", 65536, [_last_edge(1290)], ex(RET0_LAST)),
           Case("exit_last_fits_1321", 65536, [_last_edge(1289)], ex(SEARCH_END, True))]
    for S in (12, 13, 14):
        chunks = [noise(S, 600 + S), bytes(S), text(S), (b"ab" * 7)[:S]]

        def witness(c, S=S):
            rs = [one(c, i) for i in range(4)]
            assert all(r.searches == (0 if S < 13 else 1) for r in rs), rs
            # 12: no search, 13 literals do not fit; 13 and 14: the zeros' match runs to matchlimit
            assert rs[0].stored and rs[2].stored and rs[1].stored == (S == 12), rs
            assert S == 12 or (rs[1].exit == MATCH_END and rs[1].at_matchlimit == 1 and rs[1].size == 10), rs[1]
            return True
        out.append(Case(f"tiny_{S}", 65536, chunks, witness))
    return out


# ======== 7: length fields =====================================================================
LIT_EDGES = (14, 15, 269, 270, 271, 15 + 255 * 64 + 1)
ML_EDGES = (14, 15, 269, 270, 524, 525)


def _class7():
    r = Runs(700).seq(40, 20)
    for lit in LIT_EDGES:
        r.seq_exact(lit, 60)
    for mc in ML_EDGES:
        r.seq(9, mc)
    r.seq(11, 255 * 64 + 7).lits(30)
    a = r.bytes()

    def witness(c):
        rep = one(c)
        assert not rep.stored and set(LIT_EDGES) <= set(rep.lits()) and set(ML_EDGES) <= set(rep.mls()), rep.seq
        assert rep.max_ml == 255 * 64 + 7 and rep.max_lit == LIT_EDGES[-1] and rep.lit_255 >= 1 and rep.ml_255 >= 2
        assert all(x[3] == 1 for x in rep.seq if x[1] < 64)
        return True
    D = 17000
    lasts = []
    for last in LIT_EDGES:
        q = Runs(710 + last % 100).seq(40, D - 40 - last - 5).lits(last)
        lasts.append(q.bytes())

    def witness_last(c):
        got = [one(c, i) for i in range(len(LIT_EDGES))]
        assert [x.last_lit for x in got] == list(LIT_EDGES) and not any(x.stored for x in got), got
        assert all(x.exit == SEARCH_END for x in got)
        return True
    return [Case("length_fields", 65536, [a.ljust((len(a) + 7) & ~7, b"\xee")], witness),
            Case("last_literal_lengths", 65536, lasts, witness_last)]


# ======== 8: LZ4_count ===========================================================================
def count_lane(S, row):
    """(lane, byte, in the byte-wise tail) of le_block's LZ4_count for a
    sequence: the compare starts at position + 4, 256 bytes per step, lane f
    has 4 bytes and goes byte by byte when they reach past matchlimit."""
    pos, mc = row[0], row[2]
    f, j = (mc % 256) // 4, mc % 4
    a = pos + 4 + mc - j
    return f, j, a + 4 > S - LASTLIT


def _class8():
    D = 2400
    mcs = (0, 1, 2, 3, 140, 141, 142, 143, 256, 512, 257, 60)

    def body(seed):
        r = Runs(seed).seq(30, 8)
        for mc in mcs:
            r.seq(7, mc)
        return r
    # the last match: ends at matchlimit in lane 5; the same at mc = 256 (lane 0 of the second step);
    # a mismatch one byte short of matchlimit, byte 1 of lane 5
    chunks = []
    for kind in ("limit", "limit256", "short"):
        r = body(800)
        mc = {"limit": 23, "limit256": 256, "short": 21}[kind]
        v = r.v % 255 + 1
        if kind == "short":      # the run's first byte at D - 11 - mc, the first byte behind it at D - 6
            r.seq(7, D - 17 - mc - len(r.a) - 17)       # (a run as filler: the step stays 1)
            r.lits(6, (r.v % 255 + 1,)).seq(7, mc).lits(6)
        else:                    # the run's first byte at D - 10 - mc, the match from the next up to D - 5
            r.seq(7, D - 16 - mc - len(r.a) - 17)
            v = r.v % 255 + 1
            r.lits(6, (v,)).lits(6, (v,))
            r.a += bytes([v]) * (D - len(r.a))
        assert len(r.a) == D
        chunks.append(r.bytes())

    def witness(c):
        reps = [one(c, i) for i in range(3)]
        for rep in reps:
            assert not rep.stored and set(mcs) <= set(rep.mls()), rep.seq
            lanes = {count_lane(c.D, x)[:2] for x in rep.seq}
            assert {(0, 0), (0, 1), (0, 2), (0, 3), (35, 0), (35, 1), (35, 2), (35, 3)} <= lanes, lanes
        a, b, s = (x.seq[-1] for x in reps)
        mlim = c.D - LASTLIT
        assert reps[0].at_matchlimit == 1 and a[0] + 4 + a[2] == mlim and count_lane(c.D, a) == (5, 3, True), a
        assert reps[1].at_matchlimit == 1 and b[2] == 256 and count_lane(c.D, b) == (0, 0, True), b
        assert reps[2].at_matchlimit == 0 and s[0] + 4 + s[2] == mlim - 1 and count_lane(c.D, s) == (5, 1, True), s
        return True
    return [Case("count_lanes", 65536, chunks, witness)]


# ======== 9: rematch chains ======================================================================
def _class9():
    D = 4096
    w = walk(D, 900)
    base = noise(70, 901)
    tail = base + noise(20, 902) + base[4:14] + base[20:30] + base[36:60]
    chunks = [w, w[:D - len(tail)] + tail]

    def witness(c):
        a, b = one(c, 0), one(c, 1)
        assert not a.stored and max(a.chains()) >= 3 and a.rematch > 100, a
        assert not b.stored and b.chains()[-1] == 3 and b.loop_end == MATCH_END and b.at_matchlimit == 1, b.seq[-4:]
        return True
    return [Case("rematch_chains", 65536, chunks, witness)]


# ======== 10: the frame =========================================================================
def near_slot(k0=1):
    """A 65 536-byte block that compresses to 1 .. 15 bytes under its slot:
    noise and a run of R equal bytes at its end."""
    for R in range(280, 400):
        a = noise(65536 - R, 1000) + b"\x09" * R
        r = report(a)
        if not r.stored and k0 <= 65536 - r.size <= 15:
            return a
    raise AssertionError("no such block")


def _class10():
    chunk = noise(65536, 1001) + near_slot() + noise(65536, 1002) + walk(65536, 1003) + noise(65536, 1004) + \
        walk(3001, 1005) + bytes(7)

    def witness(c):
        rs = c.reps(0)
        assert [r.stored for r in rs] == [True, False, True, False, True, False], rs
        assert 1 <= 65536 - rs[1].size <= 15
        assert sum((4 + r.size) % 16 != 0 for r in rs if not r.stored) >= 2
        return True
    return [Case("frame_mixed", 65536, [chunk], witness)]


# ======== 11: the content checksum ==============================================================
XXH_D = (1, 15, 16, 17, 111, 112, 127, 128, 129, 143, 144, 147)


def _class11():
    out = []
    # lz4_content_xxh32 by D: (16-byte stripes: 8 at a time, then singly; 4-byte tail words; tail bytes)
    shape = {1: (0, 0, 1), 15: (0, 3, 3), 16: (1, 0, 0), 17: (1, 0, 1), 111: (6, 3, 3), 112: (7, 0, 0),
             127: (7, 3, 3), 128: (8, 0, 0), 129: (8, 0, 1), 143: (8, 3, 3), 144: (9, 0, 0), 147: (9, 0, 3)}
    for D in XXH_D:
        out.append(Case(f"xxh_{D}", 65536, [noise(D, 1100 + D), text(D), bytes(D)],
                        lambda c: (c.D // 16, c.D % 16 // 4, c.D % 4) == shape[c.D]))
    for n in (15, 16, 17):
        D = 1000
        chunks = [noise(D, 1200 + i) if i % 3 == 0 else walk(D, 1200 + i) if i % 3 == 1 else text(D)[i:] + bytes(i)
                  for i in range(n)]
        out.append(Case(f"xxh_batch_{n}", 65536, chunks, (lambda n: lambda c: len(c.chunks) == n)(n)))
    chunks = [walk(1000, 1300 + i) for i in range(17)]
    out.append(Case("xxh_refused_5", 65536, chunks, lambda c: c.short == {5: 999} and len(c.chunks) == 17,
                    short={5: 999}))
    return out


# ---- the table --------------------------------------------------------------------------------------
def _build():
    return _class1() + _class2() + _bits() + _class3() + _class4() + _class5() + _class6() + _class7() + \
        _class8() + _class9() + _class10() + _class11()


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(_build())


def case(name):
    return next(c for c in all_cases() if c.name == name)


CASE_NAMES = tuple(c.name for c in all_cases())
