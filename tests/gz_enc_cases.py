"""Directed payloads for the GPU gzip encoder (zcg_deflate.hip), levels 1-9.
TEST INFRASTRUCTURE ONLY.

The encoder's promise is zlib's bytes.  Generic payloads (zeros, noise, a
random walk, text) decide by accident which branches of the GPU-only code
write them: the candidate walk of dz_search_run, the stitch of dz_parse and
its serial fallback, the register window and LDS ring of dz_parse_fast, the
length limiting behind dz_plan.  Each case here is one batch of equal-length
chunks built to reach one of those branches, with a WITNESS: a statement,
evaluated on the CPU, that it does.  A witness is stated on

  * zlib's own stream, read by deflate_kit.read_blocks (tokens, code lengths,
    the code-length symbols as sent), or
  * the path report of the CPU model (tests/hostcore/zlib_ref.cpp:
    zz_host_report_blocks, zz_host_report_seg), which tests/
    test_gz_enc_cases_host.py proves equal to zlib on the same chunk.

tests/test_gz_enc_cases_host.py asserts every witness and that the model and
its segment emulation equal zlib; tests/test_gpu_gzip_enc_craft.py encodes the
same batches on the GPU and compares every member with zlib.

NOT REACHED (no case: a test here must not pass vacuously)

  * Distance-tree length limiting.  One attempt: 16 383 literals, then copies
    of 4-6 bytes at distances drawn from 16, 17 and 18 consecutive distance
    codes (from code 14, 13 and 12 up) with the counts of `overflow_counts`,
    two seeds each.  The distance tree was never limited at levels 1, 6 and
    9; its longest code had 10 to 13 bits.  Nearer occurrences of the copied
    bytes take the matches and flatten the counts.
  * Literal/length-tree length limiting at level 1.  `lit_overflow` reaches it
    at levels 4-9 only: deflate_fast does not insert the positions inside
    the longer copies, so later copies of copied bytes come out as literals
    (850 of them at level 1).  With every source in the literals
    (`lit_overflow_fast`) levels 2 and 3 reach it; level 1 (chain 4) still
    leaves some 35 literals and a longest code of 12 bits.  One more attempt,
    the 4-byte copies made the rarest so that few inner positions are
    inserted, does not fit the 30 000 bytes behind the literals.
"""
import ctypes
import functools

import numpy as np

from deflate_kit import deflate, read_blocks

SLOW = (4, 5, 6, 7, 8, 9)
FAST = (1, 2, 3)
ALL = FAST + SLOW
NONE = 0xFFFFFFFF
DZ_TAILCAP = 2048          # zcg_deflate.hip (pinned by test_gz_enc_cases_host.py)
BLOCK_SYMS = 16383
MAX_DIST = 32506
# zlib's configuration_table: good, lazy (max_insert at levels 1-3), nice, chain
CONFIG = {1: (4, 4, 8, 4), 2: (4, 5, 16, 8), 3: (4, 6, 32, 32), 4: (4, 4, 16, 16), 5: (8, 16, 32, 32),
          6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096)}


def zlib_raw(b, level):
    """zlib's raw deflate stream as flate2 asks for it (deflate_kit.deflate's defaults)."""
    return deflate(b, level)


# ---- the CPU model (tests/hostcore, loaded by test_hostcore.host) -------------------------------
def gpu_seg(D):
    from test_hostcore import gpu_seg as f
    return f(D)


def _host():
    from test_hostcore import host
    h = host()
    u8, u32p = ctypes.c_char_p, ctypes.c_void_p
    h.zz_host_report_blocks.argtypes = [u8, ctypes.c_uint32, ctypes.c_int, u32p, ctypes.c_uint32]
    h.zz_host_report_blocks.restype = ctypes.c_int32
    h.zz_host_report_seg.argtypes = [u8, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p,
                                     ctypes.c_uint32]
    h.zz_host_report_seg.restype = ctypes.c_int32
    h.zz_host_report_seg_blocks.argtypes = [u8, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, u32p, ctypes.c_uint32]
    h.zz_host_report_seg_blocks.restype = ctypes.c_int32
    return h


def host_deflate(b, level, seg=None):
    """The serial model's raw deflate stream; with `seg`, the segment emulation's (levels 4-9)."""
    import test_hostcore as th
    return th.host_deflate(b, level) if seg is None else th.host_deflate_seg(b, level, seg)


class BlockRep:
    FIELDS = ("s0", "s1", "b0", "b1", "in_win", "last", "type", "opt_lenb", "static_lenb", "max_blindex", "lim_l",
              "lim_d", "lim_bl")

    def __init__(self, row):
        for k, v in zip(self.FIELDS, row):
            setattr(self, k, int(v))

    def __repr__(self):
        return "B(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.FIELDS) + ")"


@functools.lru_cache(maxsize=64)
def block_report(b, level):
    cap = len(b) // BLOCK_SYMS + 2
    out = np.zeros((cap, len(BlockRep.FIELDS)), np.uint32)
    n = _host().zz_host_report_blocks(b, len(b), level, out.ctypes.data, cap)
    assert 1 <= n <= cap
    return [BlockRep(r) for r in out[:n]]


@functools.lru_cache(maxsize=64)
def seg_block_records(b, level, seg=None):
    """(s0, s1, b0, b1, in_win, last) per block as zz::block_rec cuts them from
    the stitched stream of the segment emulation: what dz_parse stores."""
    seg = gpu_seg(len(b)) if seg is None else seg
    cap = len(b) // BLOCK_SYMS + 2
    out = np.zeros((cap, 6), np.uint32)
    n = _host().zz_host_report_seg_blocks(b, len(b), level, seg, out.ctypes.data, cap)
    assert 1 <= n <= cap
    return [tuple(int(x) for x in r) for r in out[:n]]


class SegRep:
    """nseg, fin (0 none, 1 the last segment's pass 1, 2 a tail that ran to D),
    fallback, nsym; per segment n1, nt, sync (NONE: ran to D), into (NONE)."""

    def __init__(self, head, per):
        self.nseg, self.fin, self.fallback, self.nsym = (int(x) for x in head)
        self.n1, self.nt, self.sync, self.into = (per[:, k].astype(np.int64) for k in range(4))
        self.tails = self.nseg - 1  # the last segment has no tail

    def synced(self):
        return self.sync[:self.tails] != NONE


@functools.lru_cache(maxsize=64)
def seg_report(b, level, seg=None):
    seg = gpu_seg(len(b)) if seg is None else seg
    nseg = max(1, -(-len(b) // seg))
    head, per = np.zeros(4, np.uint32), np.zeros((nseg, 4), np.uint32)
    n = _host().zz_host_report_seg(b, len(b), level, seg, DZ_TAILCAP, head.ctypes.data, per.ctypes.data, nseg)
    assert n == nseg
    return SegRep(head, per)


# ---- zlib's stream -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def zblocks(b, level):
    return read_blocks(zlib_raw(b, level))


@functools.lru_cache(maxsize=16)
def ztokens(b, level):
    """{input position: (length, distance)} of zlib's stream (a literal: (0, byte))."""
    return {p: (n, d) for blk in zblocks(b, level) for p, n, d in blk.tokens}


def is_match(b, level, p, n, d):
    return ztokens(b, level).get(p) == (n, d)


def literals(b, level, p, n=1):
    """Positions p .. p + n - 1 are literals in zlib's stream."""
    t = ztokens(b, level)
    return all(t.get(q, (1,))[0] == 0 for q in range(p, p + n))


# ---- payload pieces ------------------------------------------------------------------------------
def fresh(n, seed, lo=0, hi=200, seen=None):
    """n bytes in [lo, hi) in which no three bytes occur twice (nor in `seen`,
    a set of trigrams that is extended): every byte is a literal in any parse."""
    rng = np.random.default_rng(seed)
    seen = set() if seen is None else seen
    out = bytearray()
    draws = rng.integers(lo, hi, 2 * n + 64).tolist()
    k = 0
    while len(out) < n:
        if k == len(draws):
            draws, k = rng.integers(lo, hi, 2 * n + 64).tolist(), 0
        x = draws[k]
        k += 1
        if len(out) >= 2:
            t = (out[-2], out[-1], x)
            if t in seen:
                continue
            seen.add(t)
        out.append(x)
    return bytes(out)


def walk(n, seed, start=100):
    """A +-1 walk: short matches everywhere, so speculative parses meet quickly."""
    s = np.random.default_rng(seed).integers(0, 2, n) * 2 - 1
    return ((start + np.cumsum(s)) & 0xFF).astype(np.uint8).tobytes()


def period7(n):
    return (b"abcdefg" * (n // 7 + 1))[:n]


class Case:
    def __init__(self, name, levels, chunks, witness, dt="u1", src=None):
        self.name, self.levels, self.chunks, self.witness, self.dt, self.src = name, tuple(levels), chunks, witness, \
            dt, src
        self.D = len(chunks[0])

    def native(self):
        """What the device gets: the array's native bytes (chunks are the serialised ones)."""
        return self.src if self.src is not None else self.chunks


def swapped(c, name):
    """The same serialised bytes as a big-endian u16 array: dz_best then runs zz::search over ser4."""
    assert c.D % 2 == 0
    src = [np.frombuffer(x, np.uint8).reshape(-1, 2)[:, ::-1].tobytes() for x in c.chunks]
    return Case(name, c.levels, c.chunks, c.witness, ">u2", src)


# ======== match search (levels 4-9; the window rules at 1-3 too) ==========================================
MARK = bytes([249, 250, 251, 252, 253, 254, 255, 249])


def _clean_chains(a, strings, lo, hi, seed):
    """Redraws bytes of a[lo:hi] until no position there has the hash of a
    3-byte window of `strings`: those strings' chains then hold only what the
    case puts there (zlib's chains are per hash, not per three bytes)."""
    rng = np.random.default_rng(seed)
    hs = np.unique(np.concatenate([_hash(x) for x in strings]))
    while True:
        bad = np.flatnonzero(np.isin(_hash(bytes(a[lo:hi + 2])), hs)) + lo
        if not bad.size:
            return
        for q in bad.tolist():
            a[q] = int(rng.integers(0, 200))


def _hash(b):
    a = np.frombuffer(bytes(b), np.uint8).astype(np.uint32)
    return ((a[:-2] << 10) ^ (a[1:-1] << 5) ^ a[2:]) & 0x7FFF


def _marked(D, at, seed):
    a = bytearray(np.random.default_rng(seed).integers(0, 200, D).astype(np.uint8).tobytes())
    a[32768:32776] = MARK
    a[at:at + 8] = MARK
    _clean_chains(a, [MARK], 32776, at - 2, seed + 1)
    _clean_chains(a, [MARK], at + 8, D - 2, seed + 2)
    return bytes(a)


def _window_base(D):
    """Random bytes below 200, an 8-byte marker at 32768 and again at 65273 /
    65274 / 65275, nothing else in the marker's chains.  The window slides at
    the first loop top from 65274 on, or from 65275 on while 262 bytes of
    input remain (D = 70 000; not for D = 65 400), and a hash head at the slid
    window's base reads as NIL:
      D = 70 000  65273: (8, 32505).  65274: (8, 32506), the head at exactly
                  MAX_DIST before the slide.  65275: no match (the head is the
                  base, and too far).
      D = 65 400  65274: the slide has happened, the head 32768 is the base
                  and reads NIL though it is within MAX_DIST: a literal, then
                  (7, 32506) at 65275.
    The fourth chunk's only candidate is position 0, NIL before any slide."""
    if D != 70000:   # the chunk that differs, and its neighbour
        chunks = [_marked(D, at, 100 + at) for at in (65274, 65275)]

        def witness_end(c, level):
            b, n = c.chunks
            assert literals(b, level, 65274) and is_match(b, level, 65275, 7, 32506), ztokens(b, level).get(65275)
            assert literals(n, level, 65275, 8)
            return True
        return Case(f"window_base_{D}", ALL, chunks, witness_end)
    chunks = [_marked(D, at, 100 + at) for at in (65273, 65274, 65275)]
    a = bytearray(np.random.default_rng(99).integers(0, 200, D).astype(np.uint8).tobytes())
    a[0:8] = MARK
    a[1000:1008] = MARK
    _clean_chains(a, [MARK], 8, 998, 98)
    chunks.append(bytes(a))

    def witness(c, level):
        a, b, n, z = c.chunks
        assert is_match(a, level, 65273, 8, 32505)
        assert is_match(b, level, 65274, 8, 32506)
        assert literals(n, level, 65275, 8)
        assert literals(z, level, 1000) and is_match(z, level, 1001, 7, 1000)
        return True
    return Case(f"window_base_{D}", ALL, chunks, witness)


def _max_dist():
    """Before any slide.  A marker whose copy is the head of its chain at
    distance 32506 (MAX_DIST: taken) and 32507 (not); and with a nearer
    3-byte prefix of the marker as the head, so that the marker is a later
    candidate, which must be nearer than MAX_DIST: at 32506 it is not looked
    at (a literal, then 7 bytes at 32506 from the next position, where it is
    the head again), at 32505 it is."""
    D = 40000
    chunks = []
    for d, near in ((MAX_DIST, 0), (MAX_DIST + 1, 0), (MAX_DIST, 1), (MAX_DIST - 1, 1)):
        a = bytearray(np.random.default_rng(200 + d + near).integers(0, 200, D).astype(np.uint8).tobytes())
        a[100:108] = MARK
        a[100 + d:108 + d] = MARK
        if near:
            a[20000:20003] = MARK[:3]
        _clean_chains(a, [MARK], 108, 19998, 210)
        _clean_chains(a, [MARK], 20003, 100 + d - 2, 211)
        chunks.append(bytes(a))

    def witness(c, level):
        a, b, x, y = c.chunks
        p = 100 + MAX_DIST
        assert is_match(a, level, p, 8, MAX_DIST)
        assert literals(b, level, p + 1, 8)
        if level >= 4:   # (the 3 bytes at 20000 are TOO_FAR)
            assert literals(x, level, p) and is_match(x, level, p + 1, 7, MAX_DIST), ztokens(x, level).get(p)
        else:
            assert is_match(x, level, p, 3, p - 20000), ztokens(x, level).get(p)
        assert is_match(y, level, p - 1, 8, MAX_DIST - 1)
        return True
    return Case("max_dist", ALL, chunks, witness)


PREFIX_LENGTHS = (3, 15, 16, 17, 31, 32, 33, 35, 36, 257, 258)


def _prefix_chunk(tail, seed):
    """Matches of every length of PREFIX_LENGTHS (one candidate each, broken by
    the next byte), and a last match of `tail` bytes that starts at D - tail
    and ends at D.  Returns (bytes, [(position, length, distance)])."""
    seen = set()
    a = bytearray(fresh(3000, seed, seen=seen))
    want = []
    for n in PREFIX_LENGTHS:
        src = len(a) - 2000 if n > 3 else len(a) - 900
        a += fresh(5, seed + n, 200, 256, seen)          # bytes the source never has: the match starts here
        at = len(a)
        a += a[src:src + n]
        want.append((at, n, at - src))
        a += bytes([(a[src + n] + 1) % 200 + 0])         # breaks the match
        a += fresh(300 if n < 200 else 30, seed + 1000 + n, 0, 200, seen)
    pad = 36 - tail  # all three chunks of the batch have one length
    a += fresh(pad + 5, seed + 7, 200, 256, seen)
    at, src = len(a), 1000
    a += a[src:src + tail]
    want.append((at, tail, at - src))
    return bytes(a), want


def _prefix_lengths():
    """dz_search_run compares 16 and then 32 bytes of a candidate at a time and
    hands the last 32 positions of the chunk to zz::search (p + 32 <= D)."""
    built = [_prefix_chunk(tail, 300) for tail in (33, 32, 31)]
    chunks = [b for b, _ in built]
    assert len({len(b) for b in chunks}) == 1 and len(chunks[0]) % 2 == 0, [len(b) for b in chunks]

    def witness(c, level):
        for (b, want), tail in zip(built, (33, 32, 31)):
            assert want[-1][0] == len(b) - tail and want[-1][1] == tail
            assert [x[1] for x in want[:-1]] == list(PREFIX_LENGTHS)
            for p, n, d in want:
                assert is_match(b, level, p, n, d), (p, n, d, ztokens(b, level).get(p))
        return True
    return Case("prefix_lengths", SLOW, chunks, witness)


TRI = bytes([250, 251, 252])


def _budget_chunk(level, nfill, reduced, D):
    """A string TRI + G far back, `nfill` fillers TRI + x between, then the
    probe TRI + G: the far string is candidate nfill + 1 of the probe's chain
    (+ 1 more for `reduced`, where a 4-byte-shorter match at probe - 1 puts
    the search at the probe under the reduced budget)."""
    good, lazy, nice, chain = CONFIG[level]
    n1 = good + 2                      # the match at probe - 1: >= good_match, < max_lazy
    assert not reduced or n1 < lazy
    G = fresh(n1 + 20, 400 + level, 0, 100)
    a = bytearray()
    a += TRI + G + b"\xc8"             # the far string
    far = 0
    if reduced:
        a += b"\xc9\xf0" + TRI + G[:n1 - 4] + b"\xca"   # z TRI G[:n1-4]: n1 bytes match at probe - 1
    for k in range(nfill):
        a += TRI + bytes([101 + k % 90])
    a += b"\xcb"
    if reduced:
        a += b"\xf0"
    probe = len(a)
    a += TRI + G + b"\xcc\xcd\xce"
    lead = D - len(a)
    assert lead >= 1
    return fresh(lead, 500 + level, 210, 249) + bytes(a), lead + probe, lead + far, len(G) + 3


def _chain_budget(level):
    """The best candidate is the chain-th of the probe's chain in chunk 0 and
    the (chain + 1)-th in chunk 1; and (levels with good_match < max_lazy) the
    last of the reduced budget in chunk 2, the first past it in chunk 3."""
    good, lazy, nice, chain = CONFIG[level]
    red = good + 2 < lazy
    D = 4 * chain + 400
    D += D % 2
    spec = [(chain - 1, False), (chain, False)] + ([((chain >> 2) - 2, True), ((chain >> 2) - 1, True)] if red else [])
    built = [_budget_chunk(level, n, r, D) for n, r in spec]

    def witness(c, lv):
        assert lv == level
        for k, (b, probe, far, n) in enumerate(built):
            got = ztokens(b, lv).get(probe)
            if k % 2 == 0:
                assert got == (n, probe - far), (k, got)
                if k == 2:
                    assert literals(b, lv, probe - 1)       # the shorter match at probe - 1 was replaced
            else:
                assert got != (n, probe - far), (k, got)
                if k == 3:                                  # probe - 1's match of good + 2 stands
                    assert ztokens(b, lv).get(probe - 1, (0,))[0] == good + 2, ztokens(b, lv).get(probe - 1)
        return True
    return Case(f"chain_budget_l{level}", (level,), [x[0] for x in built], witness)


def _nice_and_tie():
    """The nearer of two candidates is nice_length long and ends the walk
    though the farther is longer (level 6; at level 9 nice is 258 and the
    farther wins); of two candidates of one length the nearer is kept."""
    seen = set()
    S = fresh(200, 600, 0, 100, seen)
    T = fresh(20, 601, 100, 200, seen)
    a = bytearray(fresh(50, 602, 200, 256, seen))
    far = len(a)
    a += S + b"\xd0"
    near = len(a)
    a += S[:130] + b"\xd1"
    a += fresh(9, 603, 200, 256, seen)
    probe = len(a)
    a += S + b"\xd2"
    t0 = len(a)
    a += T + b"\xd3"
    t1 = len(a)
    a += T + b"\xd4" + fresh(7, 604, 200, 256, seen)
    tp = len(a)
    a += T + b"\xd5\xd6"
    a += fresh(len(a) % 2, 605, 200, 256, seen)
    b = bytes(a)

    def witness(c, level):
        want = (130, probe - near) if CONFIG[level][2] <= 130 else (200, probe - far)
        assert ztokens(b, level).get(probe) == want, (ztokens(b, level).get(probe), want)
        assert is_match(b, level, tp, 20, tp - t1) and t1 != t0
        return True
    return Case("nice_and_tie", (6, 9), [b], witness)


def _sorted_start(k):
    """Chunk 0 has exactly k positions with hash 0 (three zero bytes), so
    their chains start at sorted indices 0 .. k - 1, below the 4 candidates
    dz_search_run loads at a time; chunk 1 is the same payload, its hash-0
    chains just behind chunk 0's entries."""
    a = bytearray(fresh(1500, 700 + k, 1, 32))
    tail = fresh(6, 710, 1, 32)
    at = [200 + 150 * i for i in range(k)]
    for p in at:
        a[p:p + 9] = b"\0\0\0" + tail
    b = bytes(a)

    def witness(c, level):
        assert c.chunks[0] == c.chunks[1]
        assert int((_hash(b) == 0).sum()) == k
        for i in range(1, k):
            assert is_match(b, level, at[i], 9, 150), ztokens(b, level).get(at[i])
        return True
    return Case(f"sorted_start_{k}", SLOW, [b, b], witness)


def _bool_matches():
    """A bool array whose source bytes are 0, 1, 2 and 255: the stream holds 0 / 1."""
    rng = np.random.default_rng(800)
    bits = rng.integers(0, 2, 6000).astype(np.uint8)
    bits[3000:3300] = bits[100:400]       # a long match among the short ones
    raw = np.where(bits == 0, 0, rng.choice(np.array([1, 2, 255], np.uint8), bits.size)).astype(np.uint8)
    b = bits.tobytes()

    def witness(c, level):
        assert set(raw.tolist()) == {0, 1, 2, 255} and (raw != 0).astype(np.uint8).tobytes() == c.chunks[0]
        assert max(n for n, _ in ztokens(b, level).values()) >= 16 and len(ztokens(b, level)) > 100
        return True
    return Case("bool_matches", (4, 6, 9), [b], witness, "bool", [raw.tobytes()])


# ======== lazy parse and stitch (levels 4-9) ==================================================
# zero-filled chunks: the longest tail of the model's segment parse has this
# many symbols (asserted by the witness).  536 416 is the longest that still
# stitches; 538 625 is the first zero-filled size that goes serial (the tails
# of 536 600 .. 538 624 are shorter: the segment grows by 32 at 536 577 and at
# 538 625).  Tails of 2 047 and 2 048 symbols, on both sides of
# `nt + 1 >= DZ_TAILCAP`, are in `tail_cap_edge`.
TAIL_D = {536416: 2047, 538625: 2055}


def _tail_cap(D, longest, fallback):
    b = bytes(D)

    def witness(c, level):
        r = seg_report(b, level)
        assert int(r.nt.max()) == longest and r.fallback == fallback, (int(r.nt.max()), r.fallback)
        return True
    return Case(f"tail_cap_{longest}", SLOW, [b], witness)


def _tail_cap_edge():
    """Zeros and then a +-1 walk (D = 540 000): the tails run through the
    zeros and sync in the walk, so the zeros' length sets the longest tail:
    2 047 symbols (stitched) and 2 048 (the first that goes serial)."""
    D = 540000
    w = walk(D, 3000)
    chunks = [bytes(Z) + w[Z:] for Z in (536408, 536666)]

    def witness(c, level):
        a, b = (seg_report(x, level) for x in c.chunks)
        assert (int(a.nt.max()), a.fallback) == (DZ_TAILCAP - 1, 0), (int(a.nt.max()), a.fallback)
        assert (int(b.nt.max()), b.fallback) == (DZ_TAILCAP, 1), (int(b.nt.max()), b.fallback)
        return True
    return Case("tail_cap_edge", SLOW, chunks, witness)


def _tail_far_over():
    """Noise: no parse is ever canonical, segment 0's tail runs to D."""
    b = fresh(20000, 900, 0, 256)

    def witness(c, level):
        r = seg_report(b, level)
        assert r.fallback == 1 and int(r.nt.max()) > 8 * DZ_TAILCAP
        return True
    return Case("tail_far_over", SLOW, [b], witness)


def _sync_shapes():
    """D = 6 000 (seg 96).  A +-1 walk: every tail syncs, some of them empty
    (a match ends exactly at the segment's end, the sync is the next
    segment's first position).  Zeros: a sync that skips more than 8
    segments.  A 7-byte period: some tails sync, the others run to D."""
    D = 6000
    assert gpu_seg(D) == 96
    chunks = [walk(D, 3000), bytes(D), period7(D)]

    def witness(c, level):
        w, z, p = (seg_report(x, level) for x in c.chunks)
        assert w.tails == 62 and w.synced().all()
        k = np.arange(w.tails)
        assert ((w.nt[:w.tails] == 0) & (w.sync[:w.tails] == (k + 1) * 96)).any()
        k = np.flatnonzero(z.synced())
        assert k.size and int((z.into[k] - k).max()) > 8, (z.into[k] - k)
        assert 0 < p.synced().sum() < p.tails
        assert not (w.fallback or z.fallback or p.fallback)
        return True
    return Case("sync_shapes", SLOW, chunks, witness)


def _no_sync():
    """2 000 bytes without a match: no parse is ever canonical, so no tail
    syncs; all 62 run to D, none past the cap, and the pending literal comes
    from segment 0's tail."""
    b = fresh(2000, 1000, 0, 64)

    def witness(c, level):
        r = seg_report(b, level)
        return r.nseg == 63 and not r.synced().any() and not r.fallback and r.fin == 2
    return Case("no_sync", ALL, [b], witness)


SMALL_D = (0, 1, 2, 3, 32, 33, 64, 65, 2048, 2049)


def _small(D):
    """nseg = 1, nseg < 64 and seg = 32: zeros, a 7-byte period, a +-1 walk.
    No tail of the zeros or the period syncs.  Of the walk's tails (on the
    model, every level alike): none of 1 at D = 33, 1 of 1 at 64, 1 of 2 at
    65, 62 of 63 at 2 048 and 31 of 32 at 2 049."""
    chunks = [bytes(D), period7(D), walk(D, 1100 + D)]

    def witness(c, level):
        seg = gpu_seg(D)
        nseg = max(1, -(-D // seg))
        assert (seg, nseg) == {0: (32, 1), 1: (32, 1), 2: (32, 1), 3: (32, 1), 32: (32, 1), 33: (32, 2), 64: (32, 2),
                               65: (32, 3), 2048: (32, 64), 2049: (64, 33)}[D]
        z, p, w = (seg_report(x, level) for x in c.chunks)
        assert z.nseg == p.nseg == w.nseg == nseg
        assert not z.synced().any() and not p.synced().any()
        want = {33: (0, 1), 64: (1, 1), 65: (1, 2), 2048: (62, 63), 2049: (31, 32)}.get(D, (0, 0))
        assert (int(w.synced().sum()), w.tails) == want, (w.sync, w.tails)
        return True
    return Case(f"small_{D}", SLOW, chunks, witness)


def _empty():
    """D = 0 at every level: one static block that holds END_BLOCK alone."""
    def witness(c, level):
        return c.D == 0 and zlib_raw(b"", level) == b"\x03\x00"
    return Case("empty", ALL, [b"", b""], witness)


def _final_literal():
    """The pending literal at Z_FINISH: from the last segment's pass 1 (a
    walk: the stitch arrives there), from a tail that ran to D (noise), or
    absent (a match that ends at D)."""
    D = 5000
    w = bytearray(walk(D, 1200))
    w[-1] = 250
    n = fresh(D, 1201)
    m = bytearray(walk(D, 1202))
    m[-40:] = m[-2000:-1960]
    z = bytes(D)
    chunks = [bytes(w), n, bytes(m), z]

    def witness(c, level):
        fins = [seg_report(x, level).fin for x in c.chunks]
        assert fins[0] == 1 and fins[1] == 2 and fins[2] == 0 and fins[3] == 0, fins
        return True
    return Case("final_literal", SLOW, chunks, witness)


def _parse_rules():
    """TOO_FAR: a 3-byte match at distance 4096 is kept, at 4097 dropped.  A
    match replaced by a longer one at p + 1.  prev_length >= max_lazy: no
    search at p + 1, so the shorter match stands: the 5-byte match at level 4
    (max_lazy 4) only, the 17-byte match at levels 4, 5 and 6 (max_lazy 4, 16,
    16); at the other levels the longer match at p + 1 replaces it."""
    chunks, marks = [], []
    for d in (4096, 4097):
        seen = set()
        a = bytearray(fresh(9000, 1300, 0, 200, seen))
        m = bytes([240, 241, 242])
        a[300:303] = m
        a[300 + d:303 + d] = m
        # x + S[:n - 1] earlier, S elsewhere, then x + S: n bytes match at q, len(S) at q + 1
        at = {}
        for n, ls, x in ((5, 20, 243), (17, 40, 244)):
            S = fresh(ls, 1310 + n, 200, 240, seen)
            p0 = 6000 + 40 * n
            a[p0:p0 + n + 1] = bytes([x]) + S[:n - 1] + bytes([245])
            a[p0 + 100:p0 + 101 + ls] = S + bytes([246])
            q = p0 + 200
            a[q - 1:q + ls + 2] = bytes([247, x]) + S + bytes([248])
            at[n] = (q, ls, p0)
        chunks.append(bytes(a))
        marks.append(at)

    def witness(c, level):
        k, f = c.chunks
        assert is_match(k, level, 300 + 4096, 3, 4096)
        assert literals(f, level, 300 + 4097, 3)
        lazy = CONFIG[level][1]
        for n, (q, ls, p0) in marks[0].items():
            if n >= lazy:
                assert is_match(k, level, q, n, q - p0), (n, ztokens(k, level).get(q))
            else:
                assert literals(k, level, q) and is_match(k, level, q + 1, ls, 101), (n, ztokens(k, level).get(q + 1))
        return True
    return Case("parse_rules", SLOW, chunks, witness)


def _block_cut(kind):
    """16 382 literals, then the 16 383rd symbol of the block:
      match258  a match of 258 bytes, and more input behind it;
      exact     a match that ends at D: the loop's symbols are a multiple of
                16 383, the last block holds END_BLOCK alone;
      pending   the same and one more byte (levels 4-9: the pending literal,
                tallied at Z_FINISH without a flush check).
    deflate_slow flushes at the top after the symbol's start, deflate_fast at it."""
    seen = set()
    a = bytearray(fresh(BLOCK_SYMS - 1, 1400, 0, 64, seen))
    n = 258 if kind == "match258" else 20
    a += a[5000:5000 + n]
    if kind == "match258":
        a += fresh(1000, 1401, 0, 64, seen)
    elif kind == "pending":
        a += bytes([(a[5000 + n] + 1) % 64])
    b = bytes(a)

    def witness(c, level):
        r = block_report(b, level)
        assert r[0].s1 - r[0].s0 == BLOCK_SYMS and r[0].b1 == BLOCK_SYMS - 1 + n and not r[0].last, r
        assert is_match(b, level, BLOCK_SYMS - 1, n, BLOCK_SYMS - 1 - 5000)
        assert len(r) == 2 and r[1].last and r[1].b0 == r[0].b1
        assert r[1].s1 - r[1].s0 == {"match258": 1000, "exact": 0, "pending": 1}[kind], r
        return True
    return Case(f"block_cut_{kind}", ALL, [b], witness)


def _flush_top():
    """The first block's 16 383rd symbol is a literal that starts at 65274,
    with more than 262 bytes behind it: deflate_slow tallies it at the loop
    top 65275, where the window slides, so the block, which starts at 0, is
    no longer in the window (in_win = 0); deflate_fast tallies it at 65274,
    before the slide (in_win = 1).  16 191 literals, a 258-byte period
    repeated over 49 083 bytes (190 matches of 258 and one of 63), the literal.
    The bytes are the same either way (the block is never cheaper stored), so
    the witness is stated on the block records of both model paths."""
    seen = set()
    a = bytearray(fresh(16191, 1450, 0, 64, seen))
    for _ in range(49083):
        a.append(a[-258])
    assert len(a) == 65274 and a[-258] < 64
    a += fresh(1000, 1451, 200, 256, seen)
    b = bytes(a)

    def witness(c, level):
        r = block_report(b, level)
        t = ztokens(b, level)
        assert r[0].s1 - r[0].s0 == BLOCK_SYMS and r[0].b0 == 0 and r[0].b1 == 65275 and t[65274][0] == 0, r[0]
        assert t[16191] == (258, 258) and t[65274 - 63] == (63, 258) and len(b) - 65274 > 262
        assert r[0].in_win == (1 if level < 4 else 0) and r[0].type == 2, r[0]
        if level >= 4:   # the records zz::block_rec cuts (the kernels' path) against the serial parse's
            want = [(x.s0, x.s1, x.b0, x.b1, x.in_win, x.last) for x in r]
            assert seg_block_records(b, level) == want and seg_block_records(b, level, 32) == want
        return True
    return Case("flush_top", ALL, [b], witness)


# ======== greedy parse (levels 1-3) ==========================================================
def reloads(b, level):
    """dz_parse_fast's register window: the loop tops (token starts of zlib's
    stream) at which it reloads (p - wb >= 250), each with the length of the
    token before it (0: a literal)."""
    wb, out, before = 0, [], None
    for blk in zblocks(b, level):
        for p, n, d in blk.tokens:
            if p - wb >= 250:
                wb = p & ~3
                out.append((p, before))
            before = n
    return out


def _fast_lengths():
    """Matches and runs of 255 .. 258 bytes (the ballot compare covers 256,
    then the byte loop), a last match clamped by the end of the input, and
    the register window reloaded behind a literal and behind a 258-byte match."""
    seen = set()
    a = bytearray(fresh(2000, 1500, 0, 200, seen))
    want = []
    for n in (255, 256, 257, 258):
        a += fresh(40 + n % 7, 1501 + n, 200, 256, seen)
        at, src = len(a), 300 * (n - 254)
        a += a[src:src + n]
        want.append((at, n, at - src))
        a += bytes([(a[src + n] + 1) % 200])
        a += fresh(3, 1600 + n, 200, 256, seen)
        at = len(a)
        a += bytes([230 + n % 4]) * (n + 1)     # a run: one literal, then (n, 1)
        want.append((at + 1, n, 1))
    a += fresh(5, 1700, 200, 256, seen)
    at = len(a)
    a += a[1600:1700]                           # could go on (the source does): clamped at D
    want.append((at, 100, at - 1600))
    b = bytes(a)

    def witness(c, level):
        for p, n, d in want:
            assert is_match(b, level, p, n, d), (p, n, d, ztokens(b, level).get(p))
        assert want[-1][0] + 100 == len(b)
        before = {n for _, n in reloads(b, level)}
        assert 0 in before and 258 in before, before
        return True
    return Case("fast_lengths", FAST, [b], witness)


def _literal_store(D):
    """63, 64 and 65 literals: dz_parse_fast stores its symbols 64 at a time."""
    b = fresh(D, 1800 + D, 0, 16)

    def witness(c, level):
        t = ztokens(b, level)
        return len(t) == D and all(n == 0 for n, _ in t.values())
    return Case(f"literal_store_{D}", FAST, [b], witness)


def _max_insert():
    """deflate_fast inserts the positions inside a match only if the match is
    no longer than max_insert_length (4 / 5 / 6 at levels 1 / 2 / 3).  For
    m = 4 .. 7: a match of m bytes at p, and later the 5 bytes from p + m - 1,
    the match's last byte and four new ones: found at p + m - 1 if that
    position was inserted, else a literal and 4 bytes at p + m."""
    seen = set()
    a = bytearray(fresh(1000, 1900, 0, 32, seen))
    at = {}
    for m in (4, 5, 6, 7):
        a += fresh(20, 1900 + m, 32, 48, seen)
        p = len(a)
        a += a[100 * m:100 * m + m]
        a += fresh(30, 1910 + m, 48, 64, seen)
        q = len(a)
        a += a[p + m - 1:p + m + 4]
        at[m] = (p, q)
    a += fresh(20, 1920, 32, 48, seen)
    b = bytes(a)

    def witness(c, level):
        for m, (p, q) in at.items():
            assert is_match(b, level, p, m, p - 100 * m)
            if m <= CONFIG[level][1]:
                assert is_match(b, level, q, 5, q - (p + m - 1)), (m, ztokens(b, level).get(q))
            else:
                assert literals(b, level, q) and is_match(b, level, q + 1, 4, q + 1 - (p + m)), (m, level)
        return True
    return Case("max_insert", FAST, [b], witness)


def _two_slides():
    """D > 98 304 + 262: two slides, so head and prev entries below and at or
    above 32 768 are slid twice; matches whose candidates' bytes straddle
    32 768, 65 536 and 98 304 (the LDS ring wraps inside the compare); the
    reload crossed by literals and by 258-byte matches on the way."""
    D = 99000
    seen = set()
    a = bytearray(fresh(D, 2000, 0, 200, seen))
    want = []
    for edge in (32768, 65536, 98304):
        src = edge - 100
        at = edge + 200
        a[at - 1] = 250
        a[at:at + 258] = a[src:src + 258]
        a[at + 258] = (a[src + 258] + 1) % 200
        want.append((at, 258, at - src))
    for at in (40000, 70000):       # candidates on both sides of 32 768 in the slid tables
        a[at - 1] = 251
        a[at:at + 30] = a[at - 20000:at - 20000 + 30]
        a[at + 30] = (a[at - 20000 + 30] + 1) % 200
        want.append((at, 30, 20000))
    b = bytes(a)

    def witness(c, level):
        for p, n, d in want:
            assert is_match(b, level, p, n, d), (p, n, d, ztokens(b, level).get(p))
        before = {n for _, n in reloads(b, level)}
        assert 0 in before and 258 in before
        return D > 98304 + 262
    return Case("two_slides", ALL, [b], witness)


# ======== trees and bits ===================================================================
OVERFLOW_LENGTHS = (4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51)  # one per length code


def overflow_counts(n):
    """1, 1, 3, 5, 9, 15, ...: each the sum of the two before plus 1.  (Exact
    Fibonacci counts do not overflow: zlib's depth tie-break flattens the tree.)"""
    c = [1, 1]
    while len(c) < n:
        c.append(c[-1] + c[-2] + 1)
    return c


def _overflow_payload(ncodes, seed, literals_only=False):
    """16 383 literals (one block), then one copy per item out of the
    bytes up to 30 000 back (the literals while they reach), the item lengths over `ncodes` length
    codes with overflow_counts, shuffled; every copy is chosen so that the byte
    behind its source is not the next byte of the payload.  `literals_only`:
    every source lies in the literals, whose positions deflate_fast always
    inserts (it does not insert the inside of a copy longer than max_insert)."""
    rng = np.random.default_rng(seed)
    a = bytearray(fresh(BLOCK_SYMS, seed, 0, 256))
    lens = np.repeat(np.array(OVERFLOW_LENGTHS[:ncodes]), overflow_counts(ncodes)[::-1])
    rng.shuffle(lens)
    stop = None  # the byte the next item must not start with
    for n in lens.tolist():
        lo = max(0, len(a) - 30000)
        assert not literals_only or lo + n + 10 < BLOCK_SYMS
        while True:
            s = int(rng.integers(lo, (BLOCK_SYMS if literals_only else max(BLOCK_SYMS, lo + 2000)) - n))
            if a[s] != stop and a[s - 1] != a[-1]:
                break
        a += a[s:s + n]
        stop = a[s + n]
    return bytes(a)


def _lit_overflow():
    """The second block's literal/length tree is deeper than 15 bits before
    gen_bitlen's repair.  (Levels 4-9 only: see NOT REACHED at the top.)"""
    b = _overflow_payload(16, 2101)

    def witness(c, level):
        r = block_report(b, level)
        assert any(x.lim_l for x in r[1:]), r
        assert max(max(blk.ll) for blk in zblocks(b, level) if blk.type == 2) == 15
        return True
    return Case("lit_overflow", SLOW, [b], witness)


def _lit_overflow_fast():
    """The same for deflate_fast, every copy taken out of the literals: the
    tree is limited at levels 2 and 3.  (Not at level 1: see NOT REACHED.)"""
    b = _overflow_payload(16, 0, literals_only=True)

    def witness(c, level):
        r = block_report(b, level)
        assert any(x.lim_l for x in r[1:]), r
        assert max(max(blk.ll) for blk in zblocks(b, level) if blk.type == 2) == 15
        return True
    return Case("lit_overflow_fast", (2, 3), [b], witness)


def _stored_disallowed():
    """The 18-length variant: its second block starts at 16 383 and is flushed
    after the window has slid, so a stored block is not allowed (in_win = 0)."""
    b = _overflow_payload(18, 2101)

    def witness(c, level):
        r = block_report(b, level)
        return any(not x.in_win for x in r)
    return Case("stored_disallowed", SLOW, [b], witness)


def _bl_overflow():
    """The code-length tree is deeper than 7 bits before the repair."""
    b = BL_OVERFLOW()

    def witness(c, level):
        return any(x.lim_bl for x in block_report(b, level))
    return Case("bl_overflow", (1, 6, 9), [b], witness)


def BL_OVERFLOW():
    return np.cumsum(np.random.default_rng(BL_SEED).integers(-3, 4, BL_N)).astype("<i2").tobytes()


BL_SEED, BL_N = 4, 32000


def _runs(lens):
    """[(value, run length)] of the maximal runs of a code-length array."""
    out = []
    for x in lens:
        if out and out[-1][0] == x:
            out[-1][1] += 1
        else:
            out.append([x, 1])
    return [tuple(r) for r in out]


def _clen_gaps():
    """Literal alphabets with gaps of exactly 2, 3, 10, 11 and 138 unused
    codes (chunk 0) and 139 (chunk 1): two plain zeros, REPZ_3_10 of 3 and 10,
    REPZ_11_138 of 11 and 138, and 138 + one plain zero."""
    used0 = [0, 1, 4, 5, 9, 10, 21, 22, 34, 35, 174, 175]
    used1 = [0, 1, 141, 142, 150, 151, 152, 153, 154, 155, 156, 157]
    chunks = []
    for used, seed in ((used0, 2200), (used1, 2201)):
        rng = np.random.default_rng(seed)
        p = np.array([2.0 ** -(1 + i // 2) for i in range(len(used))])
        chunks.append(rng.choice(np.array(used, np.uint8), 4000, p=p / p.sum()).tobytes())

    def witness(c, level):
        for b, used in zip(c.chunks, (used0, used1)):
            assert sorted(set(b)) == used
        s0 = [blk for blk in zblocks(c.chunks[0], level) if blk.type == 2][0]
        s1 = [blk for blk in zblocks(c.chunks[1], level) if blk.type == 2][0]
        zr = [r for r in _runs(s0.ll[:176]) if r[0] == 0]
        assert [n for _, n in zr] == [2, 3, 10, 11, 138], zr
        sent = s0.sent
        assert (17, 3) in sent and (17, 10) in sent and (18, 11) in sent and (18, 138) in sent
        k = s1.sent.index((18, 138))
        assert s1.sent[k + 1] == (0, 1) and (0, 139) in _runs(s1.ll)
        return True
    return Case("clen_gaps", (1, 6), chunks, witness)


def arranged(counts, seed):
    """The multiset {value: count} in an order in which no three bytes occur
    twice (no match in any parse, so the literal counts are the counts)."""
    for attempt in range(200):
        rng = np.random.default_rng(seed + attempt)
        left, out, seen = dict(counts), [], set()
        while left:
            vals = [v for v in left if len(out) < 2 or (out[-2], out[-1], v) not in seen]
            if not vals:
                break
            w = np.array([left[v] for v in vals], float)
            v = vals[int(rng.choice(len(vals), p=w / w.sum()))]
            if len(out) >= 2:
                seen.add((out[-2], out[-1], v))
            out.append(v)
            left[v] -= 1
            if not left[v]:
                del left[v]
        if not left:
            return bytes(out)
    raise AssertionError("no arrangement")


def _clen_runs():
    """Runs of 3, 6 and 7 equal non-zero code lengths (three plain lengths;
    one plain and REP_3_6 of 5; one plain and REP_3_6 of 6).  Dyadic counts fix
    the lengths: 32 values of weight 8 (16 of them in the runs; END_BLOCK and
    a value of 7 make one) get 6 bits, 4 of weight 64 (one behind each run) 3."""
    counts = {v: 8 for v in range(10, 28)}
    counts.update({13: 64, 20: 64, 28: 64, 130: 64, 120: 7})
    counts.update({v: 8 for v in range(100, 115)})
    b = arranged(counts, 2300)

    def witness(c, level):
        blk, = zblocks(b, level)
        assert blk.type == 2 and all(n == 0 for _, n, _ in blk.tokens)
        assert _runs(blk.ll[10:29]) == [(6, 3), (3, 1), (6, 6), (3, 1), (6, 7), (3, 1)], _runs(blk.ll[:29])
        k = blk.sent.index((17, 10))
        assert blk.sent[k + 1:k + 12] == [(6, 1)] * 3 + [(3, 1), (6, 1), (16, 5), (3, 1), (6, 1), (16, 6), (3, 1)] + \
            [(18, 71)], blk.sent[k:k + 12]
        return True
    return Case("clen_runs", (1, 6), [b], witness)


def _degenerate():
    """D = 1.  A dynamic block with no match: the distance tree is forced to
    two codes.  A dynamic block whose matches all have one distance code."""
    lits = fresh(3000, 2400, 0, 48)
    runs = b"".join(bytes([x]) * 15 for x in range(200))   # every byte value in one run: distance 1 alone

    def witness(c, level):
        a, = zblocks(lits, level)
        assert a.type == 2 and all(n == 0 for _, n, _ in a.tokens) and a.dl == [1, 1], (a.type, a.dl)
        r, = zblocks(runs, level)
        ds = {d for _, n, d in r.tokens if n}
        assert r.type == 2 and ds == {1} and r.dl == [1, 1], (r.type, ds, r.dl)
        return True
    one = Case("one_byte", ALL, [b"\x00", b"\xff", b"a"], lambda c, level: len(c.chunks[0]) == 1)
    return [one, Case("degenerate_trees", ALL, [lits, runs], witness)]


def _block_types():
    """dynamic, stored, dynamic and a static last block in one chunk: the
    stored block's header starts inside a byte, and so does the static block."""
    seen = set()
    a = fresh(BLOCK_SYMS, 2500, 0, 48, seen) + fresh(BLOCK_SYMS, 2501, 0, 256, seen)
    a += fresh(BLOCK_SYMS, 2502, 100, 148, seen) + fresh(12, 2503, 0, 256, seen)
    b = a

    def witness(c, level):
        z = zblocks(b, level)
        assert [x.type for x in z] == [2, 0, 2, 1], [x.type for x in z]
        assert z[1].bit % 8 not in (0, 6, 7) and z[3].bit % 8 != 0, [x.bit % 8 for x in z]
        assert [x.type for x in block_report(b, level)] == [2, 0, 2, 1]
        return True
    return Case("block_types", ALL, [b], witness)


# ---- the table --------------------------------------------------------------------------------------
def _build():
    cases = [_window_base(70000), _window_base(65400), _max_dist(), _prefix_lengths()]
    cases += [_chain_budget(lv) for lv in (4, 6, 9)]
    cases += [_nice_and_tie()]
    cases += [_sorted_start(k) for k in (1, 2, 3, 4, 5)]
    cases += [swapped(cases[3], "prefix_lengths_be2")] + [swapped(c, c.name + "_be2") for c in cases[4:7]]
    cases += [_bool_matches()]
    cases += [_tail_cap(D, n, int(n >= DZ_TAILCAP)) for D, n in TAIL_D.items()] + [_tail_cap_edge()]
    cases += [_tail_far_over(), _sync_shapes(), _no_sync()] + [_small(D) for D in SMALL_D] + [_empty()]
    cases += [_final_literal(), _parse_rules()] + [_block_cut(k) for k in ("match258", "exact", "pending")] + \
        [_flush_top()]
    cases += [_fast_lengths()] + [_literal_store(D) for D in (63, 64, 65)] + [_max_insert(), _two_slides()]
    cases += [_lit_overflow(), _lit_overflow_fast(), _stored_disallowed(), _bl_overflow(), _clen_gaps(), _clen_runs()]
    cases += _degenerate() + [_block_types()]
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(_build())


def case(name):
    return next(c for c in all_cases() if c.name == name)


CASE_NAMES = tuple(c.name for c in all_cases())
# (name, level) of every GPU encode call and CPU witness
RUNS = tuple((c.name, lv) for c in all_cases() for lv in c.levels)
