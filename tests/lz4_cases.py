"""The case tables of the directed LZ4 frames.  TEST INFRASTRUCTURE ONLY.

Every case is Case(name, frame, length, want, ...): the frame's bytes, the
full decoded length (from the sequence list alone) and the status the
reference decoder must give at the batch's D: "ok", "invalid" or "eof".
Cases are grouped into batches that share one D (`batches()`); a case is
padded to its batch's D with literals, in its final literal-only sequence
(the tail, at least 12 bytes) or, where the final sequence is the subject,
in a long first sequence.  tests/test_lz4_craft_host.py checks every case
against the reference decoder and the model and pins `census()`;
tests/test_gpu_lz4_craft.py names the kernel branch each family is for.
"""
import functools
import struct
from collections import defaultdict
from typing import NamedTuple

import numpy as np

import lz4_craft as lc

CAP = 65536      # block maximum of block-size id 4
CAP5 = 262144    # of id 5
MAIN = 49152     # D of the batches of families A to D (a block of mostly literals must stay below CAP compressed)

LIT_LENGTHS = [0, 1, 14, 15, 16, 269, 270, 271, 525, 1023, 1024, 1025, 2047, 2048, 2049, 5000]
MATCH_LENGTHS = [4, 18, 19, 20, 273, 274, 275, 529, 1024, 1025, 2048, 2049, 40000]
CHAIN_BYTES = list(range(14, 21))  # length bytes of 255 in one chain
# window offsets of a chain's token.  The format's shortest sequence is three
# bytes, so no token can sit one byte behind a window start: 3 stands for 1.
CHAIN_WINDOW_OFFSETS = [0, 3, 15, 16, 47, 48, 49, 62, 63]
C1_OFFSETS = list(range(16))
C1_ML = [4, 15, 16, 17, 31, 32, 33, 48, 100, 1030]
PHASES = [0, 1, 15, 16, 17, 64, 111, 112, 113, 127]  # match start mod 128
C2_NEAR = list(range(90, 101))                      # every ring phase, ml 20 and 40
C2_OFFSETS = [16, 17, 31, 32, 63, 64, 65, 123, 124, 127, 128, 129]
C2_ML = [20, 40]
C3_FAR = [2047, 2048, 2049, 4095]
C3_RING_SWEEP = list(range(1900, 2050))  # 2048 - k for every k a step's total can take here
HEAVY_SIZES = [1024, 1025, 2048, 2049, 3073]
HEAVY_OFFSETS = [1, 7, 16, 100, 1000, 1024, 1025, 2047, 2048, 2049, 3000]
H_START = 1408   # where family H's sequence starts (a multiple of 128)
H_FULL = 3600    # decoded length of family H's streams


class Case(NamedTuple):
    name: str
    frame: bytes
    length: int      # full decoded length
    want: str        # at D
    family: str
    batch: str
    D: int
    blocks: list     # what model() takes
    linked: bool


_POOL = np.random.default_rng(20240).integers(1, 256, (1 << 20) + 300000, dtype=np.uint8).tobytes()
_cur = [0]
_census = defaultdict(set)


def P(n):
    """n literal bytes (none of them zero: offset 0 decodes to zeros)."""
    s = _POOL[_cur[0]:_cur[0] + n]
    _cur[0] = (_cur[0] + n + 1) % (1 << 20)
    return s


def note(key, *item):
    _census[key].add(item if len(item) > 1 else item[0])


class Blk:
    """One compressed block in the making: the sequences, the output position
    and the stream position after them."""

    def __init__(self):
        self.seqs, self.op, self.ip, self.k = [], 0, 0, 0

    def add(self, lit, off=None, ml=None):
        if isinstance(lit, int):
            lit = P(lit)
        self.seqs.append((lit, off, ml))
        self.ip += lc.seq_len(len(lit), ml)
        self.op += len(lit) + (ml or 0)
        return self

    def fill_off(self, nlit=0):
        """Some legal offset (1..60) for a filler match behind nlit literals."""
        avail = self.op + nlit
        self.k += 1
        return 0 if avail == 0 else 1 + (self.k * 7) % min(avail, 60)

    def light(self, nlit, ml=4):
        return self.add(nlit, self.fill_off(nlit), ml)

    def advance(self, delta):
        """delta (0, or >= 4) output bytes of short sequences (lit <= 7, ml 4)."""
        assert delta == 0 or delta >= 4
        while delta:
            t = min(delta, 11)
            if 0 < delta - t < 4:
                t = delta - 4
            self.light(t - 4)
            delta -= t
        return self

    def phase(self, ph):
        """Short sequences until the output position is ph mod 128."""
        d = (ph - self.op) % 128
        return self.advance(d + 128 if 0 < d < 4 else d)

    def stream(self, n):
        """n (0, or >= 3) stream bytes of short sequences (lit <= 6, ml 4)."""
        assert n == 0 or n >= 3
        while n:
            t = min(n, 9)
            if 0 < n - t < 3:
                t = n - 3
            self.light(t - 3)
            n -= t
        return self

    def to_block_offset(self, w):
        """Short sequences until the stream position is w mod 64."""
        d = (w - self.ip) % 64
        return self.stream(d + 64 if 0 < d < 3 else d)

    def window(self):
        """A sequence longer than the wave kernel's 64-byte window: the next
        sequence is the first of a window."""
        return self.light(70)

    def settle(self):
        """64 stream bytes of short sequences: the wave kernel's step that
        holds the sequences before them ends without a long sequence in it
        (one sequence above LZ_LIGHT sends a whole step down the heavy path)."""
        return self.stream(64)

    def tail(self, D):
        assert D - self.op >= 12, (D, self.op)
        self.add(D - self.op)
        return self.seqs


def full_block():
    """A compressed block that decodes to exactly CAP bytes."""
    return Blk().light(200).add(b"", 150, CAP - 204 - 40).tail(CAP)


def front_padded(D, body):
    """[a long first sequence, body...] decoding to exactly D: body(b) adds
    the rest, the final sequence included."""
    probe = Blk().light(100)
    body(probe)
    b = Blk().light(D - (probe.op - 104) - 4)
    body(b)
    assert b.op == D
    return b.seqs


_cases = []


def case(family, name, blocks, want="ok", batch=None, D=MAIN, frame=None, **fkw):
    f = lc.frame(blocks, **fkw) if frame is None else frame
    _cases.append(Case(f"{family}-{name}", f, lc.decoded_len(blocks), want, family, batch or family, D, blocks,
                       bool(fkw.get("linked", False))))


# ---- A. input-side parse ------------------------------------------------------------------------
def family_a():
    for n in LIT_LENGTHS:
        b = Blk().light(n).settle()
        note("A.lit", n)
        case("A", f"lit{n}-first", [b.tail(MAIN)])
    for m in MATCH_LENGTHS:
        b = Blk().light(8, m).settle()
        note("A.ml", m)
        case("A", f"ml{m}-first", [b.tail(MAIN)])
    for half in (0, 32):  # token at block offsets 0..63 (two blocks: the literal lengths add up to 62 KiB)
        b = Blk()
        for w in range(half, half + 32):
            b.to_block_offset(w)
            note("A.lit_token_at", b.ip % 64)
            b.light(LIT_LENGTHS[w % 16])
        case("A", f"lit-placed{half}", [b.tail(MAIN)])
    b = Blk()
    for w in range(64):
        b.to_block_offset(w)
        note("A.ml_token_at", b.ip % 64)
        b.light(2, MATCH_LENGTHS[w % 12])
    case("A", "ml-placed", [b.tail(MAIN)])
    b = Blk().light(100).light(8, 40000)  # (40000 once: it does not fit 64 placements)
    case("A", "ml40000-late", [b.tail(MAIN)])
    for nb in CHAIN_BYTES:
        for w in CHAIN_WINDOW_OFFSETS:
            b = Blk().stream(w)
            assert b.ip == w
            r = 0 if w == 16 else (nb * 37 + w) % 255
            b.light(15 + 255 * nb + r)
            note("A.lit_chain", nb, w)
            case("A", f"chain{nb}-lit-at{w}", [b.tail(MAIN)])
        # a match-length chain behind 10 literals: its bytes start at 13 and leave the 16-byte window
        b = Blk().stream(47).light(10, 19 + 255 * nb + (nb * 11) % 255)
        note("A.ml_chain", nb, 47)
        case("A", f"chain{nb}-ml-at47", [b.tail(MAIN)])
        b = Blk().stream(3).light(15, 19 + 255 * nb)  # both nibbles 15, remainder bytes 0
        note("A.ml_chain", nb, 3)
        case("A", f"chain{nb}-both-at3", [b.tail(MAIN)])


# ---- B. the wave window -------------------------------------------------------------------------
def family_b():
    b = Blk().add(b"", 0, 4)  # 25 three-byte sequences from the block start (offset 0 at position 0 is legal)
    for i in range(24):
        b.add(b"", 1 + i % 4, 4)
    case("B", "min25-first", [b.settle().tail(MAIN)])
    b = Blk().window()
    for i in range(30):
        b.add(b"", 1 + (i * 5) % 31, 4)
    case("B", "min30-late", [b.settle().tail(MAIN)])
    for n in (63, 64, 65):  # the successor's window offset
        b = Blk().stream(n).light(5, 6).settle()
        note("B.successor_at", n)
        case("B", f"succ{n}-light", [b.tail(MAIN)])
        b = Blk().light(29).stream(n - 33).light(5, 6)  # one 33-byte sequence: the heavy path
        assert b.seqs[-1] and b.ip - lc.seq_len(5, 6) == n
        case("B", f"succ{n}-heavy", [b.tail(MAIN)])
        b = Blk().window().stream(n).light(5, 6).settle()
        case("B", f"succ{n}-late", [b.tail(MAIN)])
    b = Blk().stream(56).light(14)      # literals at window bytes 57..70
    case("B", "lits-cross-14", [b.tail(MAIN)])
    b = Blk().stream(40).light(28)      # 32 bytes, light: literals at 42..69
    case("B", "lits-cross-28", [b.tail(MAIN)])
    b = Blk().window().stream(60).light(14).stream(50).light(13).settle()
    case("B", "lits-cross-late", [b.tail(MAIN)])
    # the final sequence first in a window (12 bytes: light; 40: heavy) and at a window's last offset
    case("B", "final-at0-12", [front_padded(MAIN, lambda b: b.add(12))])
    case("B", "final-at0-40", [front_padded(MAIN, lambda b: b.add(40))])
    case("B", "final-at0-exit", [front_padded(MAIN, lambda b: b.stream(64).add(12))])
    case("B", "final-at63-12", [front_padded(MAIN, lambda b: b.stream(63).add(12))])
    case("B", "final-at63-33", [front_padded(MAIN, lambda b: b.stream(63).add(33))])
    for nlit, ml in ((0, 32), (28, 4), (29, 4), (0, 33)):  # LZ_LIGHT: 32 is light, 33 heavy
        for lead in (0, 3):
            b = Blk().window()
            for _ in range(lead):
                b.light(2)
            b.light(nlit, ml)
            for _ in range(4):
                b.light(1)
            b.settle()
            note("B.total", nlit, ml)
            case("B", f"total-{nlit}+{ml}-lead{lead}", [b.tail(MAIN)])


# ---- C. offsets ---------------------------------------------------------------------------------
def family_c1():
    for off in C1_OFFSETS:
        b = Blk().light(140)
        for ml in C1_ML:
            for ph in PHASES:
                b.phase(ph)
                assert b.op % 128 == ph
                b.add(b"", off, ml)
                note("C1", off, ml, ph)
        case("C1", f"off{off}", [b.tail(MAIN)])


def family_c2():
    for off in C2_OFFSETS:
        b = Blk().light(140)
        for ml in C2_ML:
            for ph in PHASES:
                b.phase(ph)
                b.add(b"", off, ml)
                note("C2", off, ml, ph)
        case("C2", f"off{off}", [b.tail(MAIN)])
    for off in C2_NEAR:
        b = Blk().light(140)
        for ml, stride in ((20, 27), (40, 47)):  # odd strides visit all 128 phases
            b.phase(0)
            for _ in range(128):
                note("C2.near", off, ml, b.op % 128)
                b.add(b"", off, ml)
                b.advance(stride - ml)
        case("C2", f"near{off}", [b.tail(MAIN)])


def family_c3():
    for off in C3_FAR:  # the source is the output of the window just before
        for ml in (20, 40):
            b = Blk().light(4200).add(b"", off, ml).light(3).add(b"", off, ml).settle()
            note("C3.far", off, ml)
            case("C3", f"off{off}-ml{ml}", [b.tail(MAIN)])
    for ml in (20, 100):  # sources just inside and just outside the ring, light and heavy steps
        b = Blk().light(2100)
        for off in C3_RING_SWEEP:
            b.window().add(b"", off, ml)
            note("C3.ring", off, ml)
            if ml == 20:
                b.stream(64)
        case("C3", f"ring-sweep-ml{ml}", [b.tail(MAIN)])
    full = full_block()
    for d, want in ((0, "ok"), (1, "invalid")):  # offset == position, position + 1
        for nlit, ml in ((50, 8), (20, 40), (10, 8)):  # (the last: a light step)
            bad = "-invalid" if d else ""
            b = Blk().add(nlit, nlit + d, ml).settle()
            note("C3.block_start", d, 0)
            case("C3", f"off=op+{d}-{nlit}-block0", [b.tail(MAIN)], want, batch="C3" + bad)
            b = Blk().light(nlit).light(3)
            b.add(b"", b.op + d, ml).settle()
            case("C3", f"off=op+{d}-{nlit}-late-block0", [b.tail(MAIN)], want, batch="C3" + bad)
            b = Blk().add(nlit, nlit + d, ml).settle()
            note("C3.block_start", d, 1)
            case("C3", f"off=op+{d}-{nlit}-block1", [full, b.tail(1000)], want, batch="C3b" + bad, D=CAP + 1000)
    for ml in (20, 40):  # 65535 needs a block longer than 64 KiB: block-size id 5
        b = Blk().light(65531).add(b"", 65535, ml).light(3).add(b"", 65535, ml).settle()
        note("C3.far", 65535, ml)
        case("C3", f"off65535-ml{ml}", [b.tail(2 * CAP)], batch="C3-256k", D=2 * CAP, block_max_id=5)


def family_c4():
    # within one window: literals <- match (ml >= off) <- match (ml < off) <- match (ml >= off) <- ...
    b = Blk().window().add(8, 8, 12).add(b"", 10, 6).add(b"", 5, 9).add(b"", 3, 4).add(b"", 12, 5).add(b"", 2, 7)
    b.settle().window().add(4, 4, 4)
    for i in range(12):
        b.add(b"", 4 + i % 3, 4 + i % 5)
    case("C4", "depth", [b.settle().tail(MAIN)])
    b = Blk().light(140)
    for off in range(16, 32):  # overlapping matches
        b.light(5).add(b"", off, 100)
        note("C4.overlap", off, 100)
    case("C4", "overlap", [b.tail(MAIN)])


# ---- D. heavy rounds ----------------------------------------------------------------------------
def family_d():
    for n in HEAVY_SIZES:
        b = Blk().window().light(n - 4)
        note("D.lit", n)
        case("D", f"lit{n}", [b.tail(MAIN)])
        case("D", f"final{n}", [front_padded(MAIN, lambda b: b.add(n))])
    for off in HEAVY_OFFSETS:
        b = Blk().light(3100)
        for n in HEAVY_SIZES:
            b.window().add(b"", off, n)
            note("D.match", off, n)
        case("D", f"match-off{off}", [b.tail(MAIN)])


# ---- E. the block end at capacity ---------------------------------------------------------------
E_SHAPES = [  # name, match start below cap, ml, final literals, want
    ("end-cap5", 25, 20, 5, "ok"), ("end-cap4", 24, 20, 4, "invalid"),
    ("start-cap12", 12, 7, 5, "ok"), ("start-cap11", 11, 6, 5, "invalid"), ("start-cap9", 9, 4, 5, "invalid"),
    ("lits-cap", 100, 20, 80, "ok"), ("lits-cap+1", 100, 20, 81, "invalid"),
    ("match-past-cap", 10, 30, 0, "invalid"),
]


def family_e():
    for cap, bid, tag in ((CAP, 4, ""), (CAP5, 5, "-256k")):
        for name, start, ml, final, want in E_SHAPES:
            for off in (3, 200):
                b = Blk().light(100)
                b.add(b"", 33, cap - start - b.op - 50)  # (a match: mostly literals would not fit the block compressed)
                b.add(50, off, ml).add(final)
                note("E", name + tag, want)
                case("E", f"{name}-off{off}{tag}", [b.seqs], want,
                     batch="E" + tag + ("" if want == "ok" else "-invalid"), D=cap, block_max_id=bid)


# ---- F. block size word against content ---------------------------------------------------------
# The reference decoder's verdict for size words 1..42 of the two blocks
# (o = ok, i = invalid, e = eof), recorded from its own run; the host test
# holds every case against it.
F_WANT = {"a": "i" * 39 + "o" + "ii", "b": "i" * 39 + "o" + "ii"}
# (a cut right behind a sequence's literals leaves a well-formed last sequence: the block is
# short and the frame ends early)
F_CUT_WANT = {"a": "i" * 5 + "e" + "i" * 33, "b": "i" * 17 + "e" + "i" * 21, "c": "i" * 272 + "e" + "i" * 16}
_LETTER = {"o": "ok", "i": "invalid", "e": "eof"}


def f_blocks():
    a = [(P(5), 3, 6), (P(3), 8, 20), (b"", 1, 4), (P(20), None, None)]
    b = [(P(16), 16, 19), (P(2), 2, 5), (P(13), None, None)]
    assert len(lc.block(a)) == 40 and len(lc.block(b)) == 40
    return {"a": a, "b": b}


def family_f():
    for key, seqs in f_blocks().items():
        data = lc.block(seqs)
        D = lc.decoded_len([seqs])
        head = lc.frame([], end_mark=False)
        for word in range(1, len(data) + 3):
            f = head + struct.pack("<I", word) + data + struct.pack("<I", 0)
            want = _LETTER[F_WANT[key][word - 1]]
            case("F", f"{key}-word{word}", [seqs], want, batch=f"F{key}-{'ok' if want == 'ok' else 'bad'}", D=D,
                 frame=f)
        # the block cut at every byte, in a frame that is well formed around it (the size
        # word cases above mostly end at the garbage read as the next block header)
        for n in range(1, len(data)):
            want = _LETTER[F_CUT_WANT[key][n - 1]]
            case("F", f"{key}-cut{n}", [seqs], want, batch=f"F{key}-bad", D=D, frame=lc.frame([("sized", n, data[:n])]))
    # a block whose lengths have chains (255, then 0), cut at every byte: the `iend - 15` and
    # `iend - 4` rules of the length loops
    c = [(P(270), 5, 274), (P(12), None, None)]
    data, D = lc.block(c), lc.decoded_len([c])
    assert len(data) == 290 and len(F_CUT_WANT["c"]) == 289
    for n in range(1, len(data)):
        case("F", f"c-cut{n}", [c], _LETTER[F_CUT_WANT["c"][n - 1]], batch="Fc-bad", D=D,
             frame=lc.frame([("sized", n, data[:n])]))
    case("F", "c-whole", [c], "ok", batch="Fc-ok", D=D)
    a = f_blocks()["a"]
    D = lc.decoded_len([a])
    case("F", "empty-block-then-a", [[(b"", None, None)], a], "ok", batch="Fa-ok", D=D)
    case("F", "empty-block-alone", [[(b"", None, None)]], "eof", batch="Fa-bad", D=D)
    case("F", "a-then-empty-block", [a, [(b"", None, None)]], "ok", batch="Fa-ok", D=D)
    for word in (CAP + 1, lc.STORED | (CAP + 1), 0x7FFFFFFF):
        f = lc.frame([], end_mark=False) + struct.pack("<I", word) + lc.block(a) + struct.pack("<I", 0)
        case("F", f"word{word:#x}", [a], "invalid", batch="Fa-bad", D=D, frame=f)


# ---- G. placement and the serial path -----------------------------------------------------------
G_BODY = 6000   # decoded bytes of a body block
G_FIRST = 300   # of the short first block


def g_bodies():
    """One body per distinct branch of the serial block decoder."""
    out = {}
    out["off0"] = Blk().add(5, 0, 8).add(b"", 0, 40).light(3).add(20, 0, 100)
    out["near-short"] = Blk().add(5, 3, 20).add(1, 1, 32).add(14, 15, 31).add(2, 2, 4).add(9, 9, 17)
    out["near-long"] = Blk().add(7, 7, 100).add(2, 13, 33).add(b"", 1, 1030).add(3, 15, 48)
    out["far"] = Blk().add(40, 20, 50).add(3, 16, 100).add(200, 200, 30).add(b"", 243, 600).add(1, 17, 33)
    b = Blk()
    for n in (16, 17, 13, 1, 15, 0, 14, 12, 20, 3, 16, 11, 2, 16, 5, 100, 16):  # in and out of the 16-byte window
        b.light(n)
    out["lits"] = b
    out["long"] = Blk().light(3700).light(2, 2049)
    for b in out.values():
        b.tail(G_BODY)
    return {k: b.seqs for k, b in out.items()}


def family_g():
    D = G_FIRST + G_BODY
    far = CAP + G_BODY
    for name, body in g_bodies().items():
        first = [(P(G_FIRST), None, None)]
        case("G", f"{name}-short-first", [first, body], D=D)              # st = -1: serial, low = out
        case("G", f"{name}-linked", [first, body], D=D, linked=True)     # low = 0
        case("G", f"{name}-stored-first", [("stored", P(G_FIRST)), body], D=D)
        case("G", f"{name}-ends-early", [body], "eof", batch="G-bad", D=D)
        case("G", f"{name}-ends-early-suffix", [body], "eof", batch="G-bad", D=D, content_size=G_BODY,
             content_checksum=True)
    body = g_bodies()["far"]
    case("G", "ends-early-wrong-size", [body], "invalid", batch="G-bad", D=D, content_size=G_BODY + 1)
    case("G", "ends-early-wrong-checksum", [body], "invalid", batch="G-bad", D=D, content_checksum=True,
         content=b"x")
    first = [(P(G_FIRST), None, None)]
    for ml in (20, 400):  # a linked block's match reaching the frame's first bytes
        for d, want in ((0, "ok"), (-1, "ok"), (1, "invalid")):
            b = Blk().add(10, G_FIRST + 10 + d, ml)
            note("G.reach", d, ml)
            case("G", f"reach-op{d:+d}-ml{ml}", [first, b.tail(G_BODY)], want, batch="G" if want == "ok" else "G-bad",
                 D=D, linked=True)
            b = Blk().add(10, G_FIRST + 10 + d, ml)
            case("G", f"reach-op{d:+d}-ml{ml}-independent", [first, b.tail(G_BODY)], "invalid", batch="G-bad", D=D)
        b = Blk().add(10, 65535, ml).light(3).add(b"", 65535, ml)
        note("G.reach", 65535, ml)
        case("G", f"reach65535-ml{ml}", [full_block(), b.tail(G_BODY)], batch="G-far", D=far, linked=True)
        b = Blk().add(10, 65535, ml)
        case("G", f"reach65535-ml{ml}-stored", [("stored", P(CAP)), b.tail(G_BODY)], batch="G-far", D=far, linked=True)
    # stored and compressed blocks in one frame
    bodies = g_bodies()
    case("G", "stored-then-body", [("stored", P(CAP)), bodies["near-long"]], batch="G-far", D=far)
    b = Blk()
    for s in bodies["far"][:-1]:
        b.add(*s)
    case("G", "body-then-stored", [b.tail(CAP), ("stored", P(G_BODY))], batch="G-far", D=far)
    case("G", "body-then-stored-linked", [b.seqs, ("stored", P(G_BODY))], batch="G-far", D=far, linked=True)


# ---- H. D inside the block ----------------------------------------------------------------------
def h_streams():
    """(name, sequences, end of the sequence that starts at H_START)."""
    out = []
    for name, nlit, off, ml in (("c1", 0, 7, 100), ("c2", 0, 96, 40), ("heavy", 0, 1000, 2049), ("lit", 270, 5, 4)):
        b = Blk().light(H_START - 4)
        assert b.op == H_START
        b.add(nlit, off, ml)
        out.append((name, b.tail(H_FULL), H_START + nlit + ml))
    return out


def h_values():
    ds = set()
    for _, _, end in h_streams():
        ds |= {H_START - 1, H_START, H_START + 1}
        ds |= {end - k for k in (33, 32, 17, 16, 5, 4, 3, 1, 0, -1)}
        ds |= {end // 64 * 64 + k for k in (-64, 0, 64)}  # LZ_LPC pieces
    return sorted(ds)


def family_h():
    streams = h_streams()
    for D in h_values():
        for name, seqs, _ in streams:
            case("H", f"{name}@{D}", [seqs], batch=f"H@{D}", D=D)
            case("H", f"{name}-linked@{D}", [seqs], batch=f"H@{D}", D=D, linked=True)  # the serial lz4_block


# ---- what the wave kernel makes of a block -------------------------------------------------------
def wave_steps(seqs):
    """The wave kernel's steps over a block, from its constants (a 64-byte
    window, at most 32 sequences a step, LZ_LIGHT = 32, LZ_ROUND = 1024):
    dicts of first sequence i, end j, stream start e, output position op,
    total, heavy, and the window offset the next step starts at."""
    starts, outs, ip = [], [], 0
    for lit, _, ml in seqs:
        starts.append(ip)
        ip += lc.seq_len(len(lit), ml)
        outs.append(len(lit) + (ml or 0))
    i, op, res = 0, 0, []
    while i < len(seqs):
        j = i
        while j < len(seqs) and starts[j] - starts[i] < 64 and j - i < 32:
            j += 1
        total = sum(outs[i:j])
        res.append(dict(i=i, j=j, e=starts[i], op=op, total=total, heavy=max(outs[i:j]) > 32 or total > 1024,
                        exit=starts[j] - starts[i] if j < len(seqs) else None, starts=starts[i:j]))
        op += total
        i = j
    return res


def step_census():
    """{(family, what): steps or rounds} over the valid cases of A to E: which
    paths of the wave kernel the tables reach (LZ_RING = 2048: "ring+0" is a
    match whose first source byte is the oldest the ring still holds,
    "ring-1" the first that comes from HBM)."""
    out = defaultdict(int)
    for c in all_cases():
        if c.want != "ok" or c.family in "FGH":
            continue
        for b in c.blocks:
            if isinstance(b, tuple):
                continue
            for s in wave_steps(b):
                kind = "heavy" if s["heavy"] else "light"
                out[c.family, kind] += 1
                out[c.family, "21+ sequences"] += s["j"] - s["i"] >= 21
                if s["exit"] in (64, 65):
                    out[c.family, f"exit{s['exit']}-{kind}"] += 1
                out[c.family, "successor at 63"] += s["starts"][-1] - s["e"] == 63
                o = s["op"]
                for k in range(s["i"], s["j"]):
                    lit, off, ml = b[k]
                    start = s["starts"][k - s["i"]] - s["e"]
                    if not s["heavy"]:
                        out[c.family, "final-light"] += ml is None
                        out[c.family, "literals past 64-light"] += bool(lit) and start + lc.seq_len(len(lit)) > 64
                        src = o + len(lit) - (off or 0)
                        if off and src < s["op"] and abs(src + 2048 - s["op"] - s["total"]) <= 1:
                            out[c.family, f"ring{src + 2048 - s['op'] - s['total']:+d}-light"] += 1
                    else:
                        n = len(lit) + (ml or 0)
                        for r0 in range(0, n, 1024):
                            rn = min(1024, n - r0)
                            if rn in (1, 1024):
                                out[c.family, f"round of {rn}"] += 1
                            m = max(r0, len(lit))  # the round's first match byte
                            if off and m < r0 + rn:
                                src = o + len(lit) - off + (m - len(lit)) % off
                                if src < o + r0 and abs(src + 2048 - o - r0 - rn) <= 1:
                                    out[c.family, f"ring{src + 2048 - o - r0 - rn:+d}-heavy"] += 1
                    o += len(lit) + (ml or 0)
    return {k: v for k, v in out.items() if v}


# ---- the tables ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_cases():
    _cur[0] = 0
    _cases.clear()
    _census.clear()
    for fam in (family_a, family_b, family_c1, family_c2, family_c3, family_c4, family_d, family_e, family_f,
                family_g, family_h):
        fam()
    names = [c.name for c in _cases]
    assert len(set(names)) == len(names)
    return tuple(_cases)


def batches():
    """{batch name: (D, [cases])}; a batch is all "ok" or has no "ok" case."""
    out = {}
    for c in all_cases():
        out.setdefault(c.batch, (c.D, []))[1].append(c)
        assert out[c.batch][0] == c.D
    for name, (_, cs) in out.items():
        oks = sum(c.want == "ok" for c in cs)
        assert oks in (0, len(cs)), name
    return out


def census():
    """Counts per family and want, and the offsets, lengths and phases present."""
    cases = all_cases()
    out = {"cases": defaultdict(int), "want": defaultdict(int)}
    for c in cases:
        out["cases"][c.family] += 1
        out["want"][c.family, c.want] += 1
    out["cases"], out["want"] = dict(out["cases"]), dict(out["want"])
    out["sets"] = {k: set(v) for k, v in _census.items()}
    return out
