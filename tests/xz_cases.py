"""The case tables of the directed LZMA2 / .xz streams.  TEST INFRASTRUCTURE ONLY.

Every case is Case(name, family, frame, D, want, spec, trace): the stream's
bytes (tests/xz_craft.py writes them symbol by symbol), the D it is decoded
at and the status the reference decoder must give there: "ok", "eof" or
"invalid".  Filler is stored chunks of seeded noise, which cost nothing to
write and next to nothing to decode; unless a case says otherwise it is
lc/lp/pb = 3/0/2, check CRC64, D = 64 KiB.  `batches()` groups the cases by
family and D, at most 64 streams each.  tests/test_xz_craft_host.py checks
every case against the reference decoder, the model and the host build of
the core (with every index counted) and pins `census()`;
tests/test_gpu_xz_craft.py runs the same batches on the device.

The constants of zarr_amd/csrc/zcg_xz.hip that family E is built around are
restated here (RINGS, MARGIN, the R / 2 flush trigger and copy_in's 256-byte
pieces, in `Ring`): when they move there, move them here.
"""
import functools
from collections import defaultdict
from typing import NamedTuple

import numpy as np

import xz_craft as xc

MAIN = 65536                # D of most batches
FAR = (1 << 20) + 4096      # D of the one batch that reaches distance slot 39
SMALL = 6144                # D of family H's placement cases
RINGS = (4096, 32768)       # XZ_RING, XZ_RING_BIG
MARGIN = 512                # in_ring: a source at most R - MARGIN back is read from the ring
PIECE = 256                 # copy_in's pieces
LENGTHS = [2, 9, 10, 17, 18, 272, 273]
LCLP = [(0, 0), (4, 0), (0, 4), (2, 2), (1, 3), (3, 0)]
E_LENGTHS = [2, 63, 64, 65, 128, 273]
E_BACK = [514, 513, 512, 511, 510]          # the match's first source byte lies R - this behind pos
E_PHASES = [-273, -64, -1, 0, 1]            # pos mod R (R - 1 is 15 mod 16, R + 1 is 1)
E_OVERLAP = [1, 2, 3, 63, 64, 65, 272, 273]


class Case(NamedTuple):
    name: str
    family: str
    frame: bytes
    D: int
    want: str
    spec: dict
    trace: list
    length: int     # decoded length of the whole stream by the model (None: it has none)
    exact: bool     # the frame is the spec's (not cut, not altered)


_POOL = np.random.default_rng(20241).integers(0, 256, 1 << 21, dtype=np.uint8).tobytes()
_cur = [0]


def noise(n):
    s = _POOL[_cur[0]:_cur[0] + n]
    _cur[0] = (_cur[0] + n + 7) % (1 << 20)
    assert len(s) == n
    return s


def sym_len(s):
    return 1 if s[0] in ("lit", "srep") else 0 if s[0] == "eopm" else s[2]


class Ring:
    """The device IO's ring positions (zcg_xz.hip put / copy / copy_in / flush /
    finish) for one ring size: pos, gfl and what each copy did."""

    def __init__(self, R, D):
        self.R, self.D, self.pos, self.gfl, self.log = R, D, 0, 0, []

    def flush(self, e):
        self.gfl = min(e, self.D)

    def put(self):
        self.pos += 1
        if self.pos - self.gfl > self.R // 2:
            self.log.append(("put-flush", self.pos))
            self.flush(self.pos & ~15)

    def copy(self, d, n):
        R, trig = self.R, self.pos + n - self.gfl - self.R // 2
        if trig > 0:
            self.flush(self.pos & ~15)
        lo, hi = self.pos - d, self.pos - d + min(d, n) - 1     # the sources
        edge = self.pos - (R - MARGIN)                          # sources below it come from HBM
        where = "ring" if lo >= edge else "hbm" if hi < edge else "split"
        safe = where == "ring" or min(hi, edge - 1) < self.gfl  # an HBM source is flushed
        wrap = self.pos // R != (self.pos + n - 1) // R
        self.log.append(("copy", self.pos, d, n, where, trig, wrap, safe))
        self.pos += n

    def back(self, d):
        s = self.pos - d
        in_ring = s + (self.R - MARGIN) >= self.pos
        self.log.append(("back", self.pos, d, "ring" if in_ring else "hbm", in_ring or s < self.gfl))

    def copy_in(self, n):
        while n > 0:
            k = min(n, PIECE)
            if abs(self.pos + k - self.gfl - self.R // 2) <= 1:
                self.log.append(("copy_in-trigger%+d" % (self.pos + k - self.gfl - self.R // 2),))
            if self.pos + k - self.gfl > self.R // 2:
                self.log.append(("copy_in-flush", self.pos, k))
                self.flush(self.pos & ~15)
            self.pos += k
            n -= k

    def finish(self):
        self.flush(self.pos)


class S:
    """A stream in the making: blocks of chunks, the output position, and the
    two rings' positions as the device would have them (full length)."""

    def __init__(self, check=4):
        self.check, self.blocks, self.cur, self.pos = check, [], None, 0
        self.rings = {R: Ring(R, 1 << 40) for R in RINGS}
        self.reps, self.need_props = [1, 1, 1, 1], True
        self.block()

    # -- blocks
    def block(self, **opts):
        opts.setdefault("dict_prop", 12)  # 256 KiB
        if self.cur is not None and not self.cur["chunks"] and not self.blocks:
            self.cur["opts"] = opts  # the first block, still empty: these are its options
            return self
        if self.cur is not None:
            self.end_block()
        self.cur = dict(chunks=[], opts=opts)
        self.first, self.need_props = True, True
        return self

    def end_block(self):
        self.blocks.append(xc.block(self.cur["chunks"], **self.cur["opts"]))
        if self.check in (1, 4, 10) or self.cur["opts"].get("filters"):
            for r in self.rings.values():
                r.finish()
        self.cur = None

    # -- chunks
    def stored(self, data, ctl=None, **opts):
        if isinstance(data, int):
            data = noise(data)
        while data:
            part, data = data[:65536], data[65536:]
            c = ctl if ctl is not None else 1 if self.first else 2
            self.cur["chunks"].append(xc.stored(c, part, **opts))
            if c == 1:
                self.need_props = True
            self.first = False
            self.pos += len(part)
            for r in self.rings.values():
                r.copy_in(len(part))
        return self

    def lz(self, syms, kind=None, **opts):
        syms = list(syms)
        if kind is None:
            kind = 0xE0 if self.first else 0xC0 if self.need_props else 0x80
        if kind >= 0xC0:
            opts.setdefault("props", (3, 0, 2))
            self.need_props = False
        self.first = False
        self.cur["chunks"].append(xc.lzma(kind, syms, **opts))
        if kind >= 0xA0:
            self.reps = [1, 1, 1, 1]
        for s in syms:
            n = sym_len(s)
            if s[0] == "match":
                self.reps = [s[1]] + self.reps[:3]
            elif s[0] == "rep":
                self.reps.insert(0, self.reps.pop(s[1]))
            for r in self.rings.values():
                if s[0] == "lit":
                    r.put()
                elif s[0] == "srep":
                    r.back(self.reps[0])
                    r.put()
                elif n:
                    r.copy(self.reps[0], n)
            self.pos += n
        return self

    def raw(self, data):
        self.cur["chunks"].append(xc.raw(data))
        self.first = False
        return self

    def to(self, pos):
        """Stored filler up to the output position pos."""
        assert pos >= self.pos, (pos, self.pos)
        return self.stored(pos - self.pos) if pos > self.pos else self

    def gap(self, R):
        return self.rings[R].pos - self.rings[R].gfl

    def approach(self, R, g):
        """Stored filler until pos - gfl of ring R is g (< R / 2 - PIECE)."""
        assert g <= R // 2 - PIECE
        if self.gap(R) > g:  # force a flush: afterwards the gap is what the last pieces left
            for n in range(R // 2 - PIECE, R // 2 + 2 * PIECE + 17):
                r = Ring(R, 1 << 40)
                r.pos, r.gfl = self.rings[R].pos, self.rings[R].gfl
                r.copy_in(n)
                if r.pos - r.gfl <= g and n <= 65536:
                    self.stored(n)
                    break
        assert self.gap(R) <= g, (R, g, self.gap(R))
        if self.gap(R) < g:
            self.stored(g - self.gap(R))
        assert self.gap(R) == g
        return self

    def spec(self, pad_to=None, **opts):
        if pad_to is not None and self.pos < pad_to:
            self.to(pad_to)
        self.end_block()
        return xc.stream(self.blocks, self.check, **opts)


_cases = []


def add(name, family, spec, want, D=MAIN, frame=None):
    if isinstance(spec, S):
        spec = spec.spec(pad_to=D if want == "ok" else None)
    trace = []
    f = xc.write(spec, trace)
    m = xc.model(spec)
    _cases.append(Case(name, family, f if frame is None else frame, D, want, spec, trace,
                       None if m is None else len(m), frame is None))


def lits(n):
    return [("lit", b) for b in noise(n)]


# ---- A: the state machine -------------------------------------------------------------
def next_state(st, kind):
    if kind == "lit":
        return 0 if st < 4 else st - 3 if st < 10 else st - 6
    return {"match": 7, "rep": 8, "srep": 9}[kind] if st < 7 else 10 if kind == "match" else 11


def state_walk(seed):
    """Symbols that enter every one of the 12 states and leave it by every
    symbol kind: 48 (state, kind) pairs, in an order the seed picks."""
    rng = np.random.default_rng(seed)
    kinds = ["lit", "match", "rep", "srep"]
    todo = {(st, k) for st in range(12) for k in kinds}
    syms, st, dpos, nrep = [], 0, 0, 0

    def emit(kind, sym=None):
        nonlocal st, dpos, nrep
        if sym is not None:
            syms.append(sym)
        elif kind == "lit":
            syms.append(("lit", int(rng.integers(0, 256))))
        elif kind == "match":
            syms.append(("match", int(rng.integers(1, min(dpos, 70) + 1)), int(rng.integers(2, 12))))
        elif kind == "rep":
            syms.append(("rep", nrep % 4, int(rng.integers(2, 12))))
            nrep += 1
        else:
            syms.append(("srep",))
        todo.discard((st, kind))
        st = next_state(st, kind)
        dpos += sym_len(syms[-1])

    for _ in range(40):
        emit("lit")
    for d in (7, 19, 33, 38):  # four different reps over noise
        emit("match", ("match", d, 3))
    while todo:
        # the nearest state with something left, by breadth-first search over the kinds
        seen, queue = {st: []}, [st]
        while queue:
            s = queue.pop(0)
            left = [k for k in kinds if (s, k) in todo]
            if left:
                for k in seen[s]:
                    emit(k)
                emit(left[int(rng.integers(0, len(left)))])
                break
            for k in kinds:
                t = next_state(s, k)
                if t not in seen:
                    seen[t] = seen[s] + [k]
                    queue.append(t)
    return syms


def family_a():
    for seed, props in enumerate([(3, 0, 2), (0, 0, 0), (1, 2, 4), (2, 2, 1), (0, 4, 3), (4, 0, 2)]):
        add("A-walk-%d%d%d" % props, "A", S().lz(state_walk(seed), props=props), "ok")
    # a matched literal that agrees with the match byte, or first differs at bit 7..0
    syms = lits(50)
    for k in [None] + list(range(7, -1, -1)):
        for kind in ("match", "rep"):
            d = 5 + (k or 0)
            syms += [("match", d, 3)] if kind == "match" else [("match", d, 2), ("lit", 77), ("rep", 0, 4)]
            sofar = xc.model_block([xc.lzma(0xE0, syms)])
            mb = sofar[-d]
            low = int(noise(1)[0]) & ((1 << k) - 1) if k else 0
            syms.append(("lit", mb if k is None else (mb ^ (1 << k)) & ~((1 << k) - 1) & 0xFF | low))
    add("A-matched-literal", "A", S().lz(syms), "ok")
    # rep1, rep2 and rep3 after a known history: a wrong rotation copies other bytes
    for k in (1, 2, 3):
        hist = [("match", 5, 3), ("match", 11, 3), ("match", 23, 3), ("match", 37, 3)]
        add("A-rep%d" % k, "A", S().lz(lits(48) + hist + [("rep", k, 6), ("lit", 1), ("rep", k, 5), ("rep", 1, 4),
                                                          ("rep", 2, 3), ("rep", 3, 2), ("srep",)]), "ok")
    add("A-srep-at-dpos1", "A", S().lz([("lit", 200), ("srep",), ("srep",), ("lit", 3)]), "ok")
    add("A-srep-at-dpos0", "A", S().lz([("srep",), ("lit", 3)]), "invalid")
    add("A-rep-at-dpos0", "A", S().lz([("rep", 0, 2), ("lit", 3)]), "invalid")
    add("A-rep1-at-dpos0", "A", S().lz([("rep", 1, 2), ("lit", 3)]), "invalid")
    add("A-srep-at-dpos0-after-reset", "A", S().stored(100).lz([("srep",)], kind=0xE0), "invalid")
    add("A-rep-at-dpos0-after-reset", "A", S().lz(lits(9)).lz([("rep", 0, 5)], kind=0xE0), "invalid")
    add("A-srep-at-dpos1-after-reset", "A", S().lz(lits(9)).lz([("lit", 5), ("srep",)], kind=0xE0), "ok")


# ---- B: lengths and contexts ------------------------------------------------------------
def family_b():
    for lc, lp in LCLP:
        for pb in range(5):
            syms, pos = lits(40), 40
            for i, (ps, n) in enumerate((ps, n) for ps in range(1 << pb) for n in LENGTHS):  # every length at every pos_state
                while pos & ((1 << pb) - 1) != ps:
                    syms.append(("lit", noise(1)[0]))
                    pos += 1
                syms += [("match", 1 + (i * 7) % 39, n), ("lit", noise(1)[0])]
                pos += n + 1
                while pos & ((1 << pb) - 1) != ps:
                    syms.append(("lit", noise(1)[0]))
                    pos += 1
                syms += [("rep", i % 4, n), ("lit", noise(1)[0])]
                pos += n + 1
            add("B-%d%d%d" % (lc, lp, pb), "B", S().lz(syms, props=(lc, lp, pb)), "ok")
    # the slot context min(len - 2, 3)
    syms = lits(40)
    for n in (2, 3, 4, 5, 6):
        for d in (1, 9, 30):
            syms += [("match", d, n), ("lit", noise(1)[0])]
    add("B-slot-context", "B", S().lz(syms), "ok")
    # a dictionary reset in mid-block where the output position is no multiple
    # of 16: the contexts follow pos - dict_start
    body = lits(5) + [("match", 3, 9), ("lit", 9), ("match", 2, 18), ("lit", 1), ("rep", 0, 3)] + lits(20) + \
        [("match", 17, 273), ("lit", 4)]
    for props in ((0, 4, 4), (2, 2, 4), (3, 0, 2)):
        tag = "%d%d%d" % props
        add("B-reset-01-C0-" + tag, "B", S().lz(lits(37), props=props).stored(21, ctl=1).lz(body, kind=0xC0, props=props),
            "ok")
        add("B-reset-E0-" + tag, "B", S().lz(lits(37), props=props).lz(body, kind=0xE0, props=props), "ok")
        add("B-reset-stored-E0-" + tag, "B", S().stored(1001).lz(body, kind=0xE0, props=props), "ok")


# ---- C: distances -------------------------------------------------------------------------
def slot_dists(slots):
    out = []
    for slot in slots:
        lo, hi = xc.slot_range(slot)
        out += sorted({lo, (lo + hi) // 2, hi})
    return out


def family_c():
    # slots 0..29 inside 64 KiB: the literal trees, the reverse trees (4..13), direct bits and align
    for name, slots in (("C-slots-0-13", range(0, 14)), ("C-slots-14-21", range(14, 22)), ("C-slots-22-29", range(22, 30))):
        s = S(check=1).stored(33000)
        s.lz([x for d in slot_dists(slots) for x in (("match", d + 1, 2 + d % 5), ("lit", d & 0xFF))], kind=0xC0)
        add(name, "C", s, "ok")
    s = S().stored(5000)
    s.lz([x for a in range(16) for x in (("match", (1 << 10) + 16 * a + a + 1, 4), ("lit", a))], kind=0xC0)
    add("C-align-slot20", "C", s, "ok")
    # every slot 0..39 behind 1 MiB of stored filler, length 273 (dictionary 2 MiB)
    for name, dists in (("C-far-low", [xc.slot_range(k)[0] for k in range(40)]),
                        ("C-far-high", [xc.slot_range(k)[1] for k in range(40)]),
                        ("C-far-mid", [sum(xc.slot_range(k)) // 2 for k in range(40)])):
        s = fix_dict(S().stored(1 << 20), 18)
        s.lz([x for d in dists for x in (("match", d + 1, 273 if d > 300 else 2 + d % 9), ("lit", d & 0xFF))], kind=0xC0)
        add(name, "C", s, "ok", D=FAR)
    s = fix_dict(S().stored(1 << 20), 18)
    add("C-far-slot40", "C", s.lz([("match", (1 << 20) + 1, 5)], kind=0xC0), "invalid", D=FAR)
    add("C-eopm", "C", S().lz(lits(10) + [("eopm",)] + lits(3)), "invalid")
    add("C-eopm-last", "C", S().stored(MAIN - 10).lz(lits(10) + [("eopm",)], du=0), "invalid")
    add("C-slot63-not-all-ones", "C", fix_dict(S().lz(lits(10) + [("match", 0xFFFFFFFF, 2)] + lits(3)), 40), "invalid")
    add("C-slot62", "C", fix_dict(S().lz(lits(10) + [("match", 0x80000001, 2)] + lits(3)), 40), "invalid")


def fix_dict(s, prop):
    s.cur["opts"]["dict_prop"] = prop
    return s


# ---- D: dictionary validity --------------------------------------------------------------------
def family_d():
    for over in (0, 1):
        want, tag = ("invalid", "dpos+1") if over else ("ok", "dpos")
        for dpos in (1, 2):
            add("D-first-%s-at-%d" % (tag, dpos), "D", S().lz(lits(dpos) + [("match", dpos + over, 5), ("lit", 7)]), want)
        add("D-first-%s-at-4095" % tag, "D", S().stored(4095).lz([("match", 4095 + over, 5), ("lit", 7)]), want)
        add("D-reset01-" + tag, "D", S().stored(1000).stored(7, ctl=1).lz([("match", 7 + over, 5), ("lit", 7)]), want)
        add("D-resetE0-" + tag, "D", S().stored(1000).lz(lits(3) + [("match", 3 + over, 5), ("lit", 7)], kind=0xE0), want)
        add("D-resetE0-lzma-" + tag, "D", S().lz(lits(30)).lz(lits(3) + [("match", 3 + over, 5), ("lit", 7)], kind=0xE0),
            want)
        # a second block must not see the first one's bytes
        add("D-block2-" + tag, "D", S().stored(1000).block().lz(lits(2) + [("match", 2 + over, 5), ("lit", 7)]), want)
        add("D-block2-stored-" + tag, "D", S().stored(1000).block().stored(9).lz([("match", 9 + over, 5)]), want)
        for prop, dsz in ((0, 4096), (1, 6144), (2, 8192)):
            s = fix_dict(S().stored(10000), prop)
            s.lz([("match", dsz + over, 6), ("lit", 7)]).stored(3000).lz([("rep", 0, 9), ("srep",), ("lit", 1)], kind=0x80)
            add("D-dsz%d-%s" % (dsz, "dsz+1" if over else "dsz"), "D", s, want)
    add("D-prop40", "D", fix_dict(S().stored(9000).lz([("match", 9000, 6)]), 40), "ok")
    add("D-prop41", "D", fix_dict(S().stored(9000).lz([("match", 9000, 6)]), 41), "invalid")
    add("D-prop40-dpos+1", "D", fix_dict(S().stored(9000).lz([("match", 9001, 6)]), 40), "invalid")


# ---- E: the device ring's geometry ----------------------------------------------------------------
def family_e():
    for R in RINGS:
        # sources around the in_ring boundary: lanes of one copy read the ring, HBM or both;
        # the literal behind it is a matched literal whose match byte lies at the boundary too
        for n in E_LENGTHS:
            for back in E_BACK:
                d = R - back
                if R == 4096:                      # positions with every phase of E_PHASES
                    targets = [[(w + 2) * R + ph for w, ph in enumerate(E_PHASES)]]
                else:
                    targets = [[R + ph] for ph in E_PHASES if ph != -273] + [[R - 273, 2 * R - 273 - 2]]
                for tl in targets:
                    s = S()
                    for t in tl:
                        s.to(t).lz([("match", d, n), ("lit", noise(1)[0]), ("lit", 3)])
                    add("E%d-edge-len%d-back%d-at%d" % (R, n, back, tl[0]), "E", s, "ok")
        # the flush trigger pos + len - gfl > R / 2, from either side, with the source in HBM and in the ring
        for delta in (-1, 0, 1):
            for n in (2, 64, 273):
                for d in (1, 100, R - 512, R - 511, R + 7):
                    s = S().stored(R + 600).approach(R, R // 2 - PIECE - 40)
                    s.lz(lits(PIECE + 40 - n + delta) + [("match", d, n), ("lit", 9)], kind=0xC0)
                    add("E%d-trigger%+d-len%d-d%d" % (R, delta, n, d), "E", s, "ok")
        # a literal run and short reps across the trigger
        s = S().stored(R + 600).approach(R, R // 2 - PIECE - 40)
        s.lz(lits(PIECE + 30) + [("match", R - 511, 2)] + [("srep",), ("lit", 1)] * 12 + lits(20), kind=0xC0)
        add("E%d-literals-across-trigger" % R, "E", s, "ok")
        # overlapping copies of 273 across the ring wrap
        for d in E_OVERLAP:
            s = S()
            for w in ((1, 2, 3) if R == 4096 else (1,)):
                s.to(w * R - 100 - w).lz(lits(3) + [("match", d, 273), ("lit", 5), ("rep", 0, 273), ("lit", 6)])
            add("E%d-overlap-d%d" % (R, d), "E", s, "ok")
        # stored chunks around copy_in's pieces: from a gap of R / 2 - 256, 255 and 256 bytes stay
        # below the trigger and the second piece of 257 crosses it; from R / 2 - 257 none does
        for n in (255, 256, 257):
            for g in (R // 2 - 2 * PIECE, R // 2 - PIECE - 1, R // 2 - PIECE):
                s = S().stored(R + 600).approach(R, g)
                s.stored(n).lz([("match", R - 512, 64), ("lit", 1), ("match", R - 511, 64), ("match", n, 273)], kind=0xC0)
                add("E%d-stored%d-gap%d" % (R, n, g), "E", s, "ok")
    # a stored chunk of 65 536 bytes: it fills D on its own, so the chunks before it are short
    for lead in (0, 1, 15, 100):
        s = S()
        if lead:
            s.lz(lits(lead))
        s.stored(65536 - lead).lz([("match", 1, 2)], kind=0xC0)
        add("E-stored65536-lead%d" % lead, "E", s, "ok")


# ---- F: chunk framing -----------------------------------------------------------------------------------
CONTROL_TABLE = {
    # (what came before, this control byte): the kind the LZMA2 rules give
    ("first", 0x01): "ok", ("first", 0x02): "invalid", ("first", 0x80): "invalid", ("first", 0xA0): "invalid",
    ("first", 0xC0): "invalid", ("first", 0xE0): "ok",
    ("lzma", 0x01): "ok", ("lzma", 0x02): "ok", ("lzma", 0x80): "ok", ("lzma", 0xA0): "ok", ("lzma", 0xC0): "ok",
    ("lzma", 0xE0): "ok",
    (0x02, 0x01): "ok", (0x02, 0x02): "ok", (0x02, 0x80): "ok", (0x02, 0xA0): "ok", (0x02, 0xC0): "ok",
    (0x02, 0xE0): "ok",
    (0x01, 0x01): "ok", (0x01, 0x02): "ok", (0x01, 0x80): "invalid", (0x01, 0xA0): "invalid", (0x01, 0xC0): "ok",
    (0x01, 0xE0): "ok",
    ("block2", 0x01): "ok", ("block2", 0x02): "invalid", ("block2", 0x80): "invalid", ("block2", 0xA0): "invalid",
    ("block2", 0xC0): "invalid", ("block2", 0xE0): "ok",
}


def family_f():
    body = lits(6) + [("match", 4, 20), ("lit", 2), ("rep", 0, 4), ("srep",)]
    for (prev, ctl), want in CONTROL_TABLE.items():
        s = S()
        if prev == "lzma":
            s.lz(lits(20) + [("match", 3, 9)])
        elif prev == 0x02:
            s.lz(lits(20) + [("match", 3, 9)]).stored(300, ctl=2)
        elif prev == 0x01:
            s.lz(lits(20) + [("match", 3, 9)]).stored(300, ctl=1)
        elif prev == "block2":
            s.lz(lits(20) + [("match", 3, 9)]).stored(301).block()
        if ctl < 0x80:
            s.stored(50, ctl=ctl)
        else:
            s.lz(body, kind=ctl)
        if want == "ok":  # and the state it leaves must serve the next chunk
            s.lz(lits(3) + [("match", 2, 5)], kind=0xC0 if ctl == 1 or (prev == 0x01 and ctl == 0x02) else 0x80)
        add("F-%s-then-%02X" % (prev if isinstance(prev, str) else "%02X" % prev, ctl), "F", s, want)
    for ctl in range(3, 0x80):
        add("F-control-%02X" % ctl, "F", S().lz(lits(5)).stored(40, ctl=ctl), "invalid")
        add("F-control-%02X-first" % ctl, "F", S().stored(40, ctl=ctl), "invalid")
    # the properties byte: 224 passes the range check (pb 4, lp 4, lc 8) and fails lc + lp <= 4
    # (the reference decoder says invalid: liblzma has no legal byte above 4 * 45 + 4 * 9 + 0)
    add("F-props-224", "F", S().lz(lits(5), props_byte=224), "invalid")
    add("F-props-225", "F", S().lz(lits(5), props_byte=225), "invalid")
    add("F-props-lc4lp1", "F", S().lz(lits(5), props_byte=xc.props_byte(4, 1, 0)), "invalid")
    add("F-props-lc0lp4pb4", "F", S().lz(lits(5) + [("match", 2, 9)], props=(0, 4, 4)), "ok")
    add("F-props-lc4lp0pb4", "F", S().lz(lits(5) + [("match", 2, 9)], props=(4, 0, 4)), "ok")
    add("F-props-mid-lc3lp2", "F", S().lz(lits(5)).lz(lits(5), kind=0xC0, props_byte=xc.props_byte(3, 2, 0)), "invalid")
    syms = lits(30) + [("match", 7, 12), ("lit", 3), ("match", 3, 40)]
    for dc in (-1, 1):
        add("F-csize%+d" % dc, "F", S().lz(syms, dc=dc).stored(100), "invalid")
    add("F-usize-1-match-crosses", "F", S().lz(syms, du=-1).stored(100), "invalid")
    add("F-usize-1-literal-last", "F", S().lz(syms + lits(1), du=-1).stored(100), "invalid")
    add("F-usize+1", "F", S().lz(syms, du=1).stored(100), "invalid")
    add("F-usize+1-last", "F", S().stored(MAIN).lz(syms, du=1, kind=0xC0), "ok")   # D is reached before it
    add("F-stored-size+1", "F", S().lz(syms).stored(100, du=1).lz(lits(4)), "invalid")
    add("F-stored-size-1", "F", S().lz(syms).stored(100, du=-1).lz(lits(4)), "invalid")
    add("F-first-rc-byte-1", "F", S().lz(syms, first_byte=1), "invalid")
    add("F-first-rc-byte-FF", "F", S().lz(lits(4)).lz(syms, first_byte=0xFF), "invalid")
    add("F-one-literal", "F", S().lz(lits(1)).lz(lits(1)).lz(lits(1), kind=0xA0).lz(lits(1), kind=0xE0), "ok")
    add("F-one-literal-only", "F", S().lz(lits(1)), "ok", D=1)
    add("F-no-end-byte", "F", S().lz(syms).block(end=False).lz(syms), "invalid")
    # an LZMA chunk whose compressed size word is at its maximum, 65 536
    add("F-csize-65536", "F", S().lz(full_chunk()), "ok")


@functools.lru_cache(maxsize=None)
def full_chunk():
    """Literals whose range-coded chunk is 65 536 bytes long."""
    data = np.random.default_rng(5).integers(0, 256, 66000, dtype=np.uint8).tobytes()
    lz, rc, syms = xc.Lzma(), xc.RangeEncoder(), []
    while len(rc.out) + rc.cache_size + 4 + (rc.range < 1 << 24) < 65536:  # what finish() will give
        syms.append(("lit", data[len(syms)]))
        lz.encode(rc, syms[-1])
    assert len(rc.finish()) == 65536  # (a seed whose sizes step over 65 536 needs replacing)
    return tuple(syms)


# ---- G: blocks and the container -----------------------------------------------------------------------------
def two_blocks(check=4, n1=1001, n2=777, **kw):
    s = S(check=check).lz(lits(20) + [("match", 5, 30)]).stored(n1 - 50)
    s.block(**kw).lz(lits(9) + [("match", 9, 33), ("rep", 0, 3)], props=(0, 4, 0)).stored(n2 - 45)
    return s


def family_g():
    add("G-two-blocks", "G", two_blocks(), "ok")
    add("G-three-blocks-odd", "G", two_blocks(n1=1001, n2=333).block().stored(17).lz(lits(3), kind=0xC0)
        .block().lz(lits(1)).block().lz(lits(7) + [("match", 7, 200)], props=(1, 1, 1)), "ok")
    add("G-empty-block-first", "G", xc.stream([xc.block([])] + two_blocks().spec(pad_to=MAIN)["blocks"]), "ok")
    add("G-empty-block-last", "G", xc.stream(two_blocks().spec(pad_to=MAIN)["blocks"] + [xc.block([])]), "ok")
    add("G-second-block-one-byte", "G", S().stored(MAIN - 1).block().lz(lits(1)), "ok")
    add("G-second-block-one-stored-byte", "G", S().lz(lits(7)).stored(MAIN - 8).block().stored(1), "ok")
    for check in (0, 1, 4, 10):
        for name, sp, want, f in check_cases(check):
            add(name, "G", sp, want, frame=f)
    # check IDs liblzma does not know are skipped over, not verified
    for check in (2, 3, 5, 9, 15):
        add("G-check%d-unknown" % check, "G", two_blocks(check=check), "ok")
    add("G-delta-first", "G", S().block(filters=(("delta", 3),)).lz(lits(40) + [("match", 7, 60)]).stored(900).block()
        .lz(lits(8) + [("match", 8, 99)]), "ok")
    add("G-delta-second", "G", S().lz(lits(40) + [("match", 7, 60)]).stored(901).block(filters=(("delta", 256),))
        .lz(lits(8) + [("match", 8, 99)]).stored(600), "ok")
    # lc + lp <= 3 first, 4 from a later chunk or block: the second launch decodes the stream again
    add("G-big-model-later-chunk", "G", S().lz(lits(30) + [("match", 9, 99)]).stored(5000)
        .lz(lits(9) + [("match", 4, 50)], kind=0xC0, props=(4, 0, 2)), "ok")
    add("G-big-model-later-block", "G", S().lz(lits(30) + [("match", 9, 99)]).stored(5001).block()
        .lz(lits(9) + [("match", 4, 50)], props=(2, 2, 0)), "ok")
    add("G-big-model-later-block-bad-distance", "G", S().lz(lits(30)).stored(5001).block()
        .lz(lits(9) + [("match", 10, 50)], props=(0, 4, 0)), "invalid")
    add("G-big-model-behind-D", "G", S().stored(MAIN).lz(lits(9), kind=0xC0, props=(4, 0, 0)), "ok")
    # the header's size fields
    for field in ("csize", "usize"):
        add("G-%s-true" % field, "G", two_blocks(**{field: True}), "ok")
        add("G-%s-true-first" % field, "G", S().block(**{field: True}).lz(lits(5) + [("match", 2, 60)]).stored(99).block()
            .stored(5), "ok")
        for dv in (-1, 1):
            s = S().block().lz(lits(5) + [("match", 2, 60)]).stored(99)
            true = len(xc.write_chunks(s.cur["chunks"])[0]) + 1 if field == "csize" else s.pos
            s.cur["opts"][field] = true + dv
            add("G-%s%+d" % (field, dv), "G", s.block().stored(5), "invalid")
    add("G-both-true", "G", two_blocks(csize=True, usize=True), "ok")
    # c_end inside the chunk header, the range coder's five bytes, the symbols, a stored chunk
    for cs in (1, 2, 4, 5, 6, 7, 10, 11, 12, 20):
        add("G-csize-%d-lzma" % cs, "G", S().block(csize=cs).lz(lits(30) + [("match", 3, 10)]), "invalid")
    for cs in (1, 2, 3, 4, 50):
        add("G-csize-%d-stored" % cs, "G", S().block(csize=cs).stored(100), "invalid")
    add("G-csize-0", "G", S().block(csize=0).stored(100), "invalid")
    for us, tag in ((50, "stored"), (100, "stored-end"), (105, "match"), (109, "match-end"), (110, "literal")):
        add("G-usize-%d-inside-%s" % (us, tag), "G",
            S().block(usize=us).stored(100).lz(lits(3) + [("match", 2, 7), ("lit", 1), ("lit", 2)]), "invalid")
    add("G-usize-larger", "G", S().block(usize=MAIN + 1).stored(100), "invalid")
    # index and footer
    sp = two_blocks(n1=100).spec(pad_to=MAIN)
    npad = index_pad(sp)
    assert npad >= 1
    recs = index_records(sp)
    for name, kw in (("count+1", dict(index=dict(count=3))), ("count-1", dict(index=dict(count=1))),
                     ("unpadded+1", dict(index=dict(records=[(recs[0][0] + 1, recs[0][1]), recs[1]]))),
                     ("usize+1", dict(index=dict(records=[recs[0], (recs[1][0], recs[1][1] + 1)]))),
                     ("usize-moved", dict(index=dict(records=[(recs[0][0], recs[0][1] + 1), (recs[1][0], recs[1][1] - 1)]))),
                     ("swapped", dict(index=dict(records=[recs[1], recs[0]]))),
                     ("padding-nonzero", dict(index=dict(pad=bytes(npad - 1) + b"\x01"))),
                     ("padding-nonzero-last", dict(index=dict(pad=b"\x80" + bytes(npad - 1)))),
                     ("backward+1", dict(footer=dict(backward=index_size(sp) // 4))),
                     ("backward-1", dict(footer=dict(backward=index_size(sp) // 4 - 2))),
                     ("footer-check-1", dict(footer=dict(check=1))),
                     ("footer-check-0", dict(footer=dict(check=0)))):
        add("G-index-" + name, "G", dict(sp, **kw), "invalid")
    add("G-trailing-bytes", "G", dict(sp, trailing=b"\x01\x02\x03\x04garbage"), "ok")
    add("G-trailing-zeros", "G", dict(sp, trailing=bytes(8)), "ok")
    for n1 in (1001, 1002, 1003):  # one, two and three bytes of padding
        sp = two_blocks(n1=n1).spec(pad_to=MAIN)
        pad = pad_of(sp["blocks"][0])
        sp["blocks"][0]["pad"] = pad[:-1] + b"\x01"
        add("G-block-padding-nonzero-%d" % len(pad), "G", sp, "invalid")
    # everything behind D in the same 32 KiB input window is still validated; behind the window nothing is
    n = 2 * 32768 - (12 + 12 + 3)  # the stored chunk's last byte is the last of an input window
    sp = S().stored(n).spec()
    add("G-index-wrong-behind-window", "G", dict(sp, index=dict(count=2)), "ok", D=n)
    add("G-end-byte-wrong-behind-window", "G", S().stored(n).raw(b"\x03").spec(), "ok", D=n)
    sp = S().stored(100).spec()
    add("G-index-wrong-in-window", "G", dict(sp, index=dict(count=2)), "invalid", D=100)
    add("G-footer-wrong-in-window", "G", dict(sp, footer=dict(check=1)), "invalid", D=100)
    add("G-trailing-in-window", "G", dict(sp, trailing=b"\x07"), "ok", D=100)


def check_cases(check):
    """(name, spec, want, frame or None) of the two-block streams with this check ID: a
    valid one and, where there is a check, one whose first block's check field is wrong."""
    out = [("G-check%d-two-blocks" % check, two_blocks(check=check).spec(pad_to=MAIN), "ok", None)]
    if check:
        sp = two_blocks(check=check).spec(pad_to=MAIN)
        lay = []
        f = bytearray(xc.write(sp, layout=lay))
        f[lay[0]["check"]] ^= 1
        out.append(("G-check%d-first-block-wrong" % check, sp, "invalid", bytes(f)))
    return out


def pad_of(b):
    return bytes(-(len(xc.write_chunks(b["chunks"])[0]) + 1) % 4)


def index_records(sp):
    lay = []
    xc.write(sp, layout=lay)
    return [(b["pad"] - b["header"] + xc.check_size(sp["check"]), b["usize"]) for b in lay]


def index_size(sp):
    n = 1 + len(xc.vli(len(sp["blocks"]))) + sum(len(xc.vli(a)) + len(xc.vli(b)) for a, b in index_records(sp))
    return (n + 3) // 4 * 4 + 4


def index_pad(sp):
    n = 1 + len(xc.vli(len(sp["blocks"]))) + sum(len(xc.vli(a)) + len(xc.vli(b)) for a, b in index_records(sp))
    return -n % 4


# ---- H: where reading stops --------------------------------------------------------------------------------
def sweep_spec():
    """A compact stream with two blocks, all chunk kinds and both size fields."""
    s = S().block(csize=True, usize=True)
    s.lz(lits(6) + [("match", 3, 9), ("lit", 1), ("rep", 0, 3), ("srep",)]).stored(noise(11), ctl=2)
    s.lz([("lit", 5), ("match", 11, 12)], kind=0x80).lz(lits(2) + [("match", 2, 4)], kind=0xA0)
    s.stored(noise(9), ctl=1).lz(lits(3) + [("match", 9, 30)], kind=0xC0, props=(0, 2, 1))
    s.block(usize=True).lz(lits(5) + [("match", 5, 40), ("lit", 0), ("rep", 0, 7)], props=(1, 0, 0)).stored(noise(6))
    s.lz(lits(2), kind=0xE0, props=(2, 0, 3))
    return s


def family_h():
    D = SMALL
    # D one below, at and one above a chunk end, a block end and a dictionary reset in mid-block
    for off in (-1, 0, 1):
        e = D + off
        add("H-lzma-chunk-end%+d" % off, "H", S().stored(e - 40).lz(lits(5) + [("match", 5, 35)]).lz(lits(9)).stored(50),
            "ok", D=D)
        add("H-stored-chunk-end%+d" % off, "H", S().stored(e).lz(lits(9)).stored(50), "ok", D=D)
        add("H-block-end%+d" % off, "H", S().stored(e - 40).lz(lits(5) + [("match", 5, 35)]).block().lz(lits(9)).stored(50),
            "ok", D=D)
        add("H-block-end-stored%+d" % off, "H", S().stored(e).block().stored(50), "ok", D=D)
        add("H-dict-reset-01%+d" % off, "H", S().stored(e).stored(40, ctl=1).lz(lits(3)), "ok", D=D)
        add("H-dict-reset-E0%+d" % off, "H", S().stored(e).lz(lits(9), kind=0xE0).stored(50), "ok", D=D)
        # what lies at D is wrong: seen only when decoding gets there
        add("H-bad-control-at-end%+d" % off, "H", S().stored(e).raw(b"\x03"), "invalid" if off <= 0 else "ok", D=D)
        # (a chunk that goes on at D is left before its next symbol is read)
        add("H-bad-distance-at-end%+d" % off, "H", S().stored(e - 2).lz(lits(2) + [("match", e + 1, 2)]),
            "invalid" if off < 0 else "ok", D=D)
    # D inside a match of 273: every split
    for k in range(1, 273):
        add("H-split-%d" % k, "H", S().stored(D - k - 3).lz(lits(3) + [("match", 1 + k % 97, 273), ("lit", 1)]).stored(20),
            "ok", D=D)
    add("H-inside-stored", "H", S().stored(D - 100).stored(300).lz(lits(2)), "ok", D=D)
    add("H-one-above-content", "H", S().stored(D - 100).lz(lits(5) + [("match", 5, 94)]), "eof", D=D)
    add("H-one-above-content-stored", "H", S().lz(lits(5)).stored(D - 6), "eof", D=D)
    add("H-at-content", "H", S().stored(D - 100).lz(lits(5) + [("match", 5, 95)]), "ok", D=D)
    # the 32 KiB input window: a chunk ends where D is reached, and the byte behind it, at input
    # offset x, is no control byte.  It is read if it lies in the window that holds the
    # chunk's last byte: x = 32 768 alone is behind a window's end.
    W = 20000
    for x in range(32760, 32776):
        s = S().stored(W)
        ip = 12 + 12 + 3 + W            # stream header, block header, the first chunk
        n = x - ip - 3
        s.stored(n).raw(b"\x03")
        add("H-window-bad-control-at-%d" % x, "H", s, "ok" if x == 32768 else "invalid", D=W + n)
        # D reached inside the chunk: nothing behind it is read
    for x in range(32760, 32776):
        s = S().stored(W)
        n = x - (12 + 12 + 3 + W) - 3
        add("H-window-inside-chunk-%d" % x, "H", s.stored(n).raw(b"\x03"), "ok", D=W + n - 1)
    # one compact stream cut at every byte, and with one bit flipped at every byte
    sw = sweep_spec()
    sp = sw.spec()
    f = xc.write(sp)
    full = len(xc.model(sp))
    for cut in range(len(f)):
        add("H-cut-%d" % cut, "H", sp, sweep_want("cut", cut, len(f)), D=full, frame=f[:cut])
    for i in range(len(f)):
        add("H-flip-%d" % i, "H", sp, sweep_want("flip", i, len(f)), D=full, frame=f[:i] + bytes([f[i] ^ (1 << (i % 8))]) + f[i + 1:])


# The sweeps' kinds are the reference decoder's, pinned as runs over the byte
# offset.  A cut stream is eof until the last byte of D has its input (offset
# 179: what follows lies in the same input window, but a window that ends
# early is no error once D bytes exist).  A flipped bit is invalid but for four
# that only make one of the last two chunks longer (offsets 158, 159: the size
# word of the last stored chunk; 167: of the last LZMA chunk), so that D is
# reached inside it, or turn the index indicator into the size byte of a block
# header that the input is too short for (188).
CUT_RUNS = [("eof", 179), ("ok", 33)]
FLIP_RUNS = [("invalid", 158), ("ok", 2), ("invalid", 7), ("ok", 1), ("invalid", 20), ("ok", 1), ("invalid", 23)]


def sweep_want(kind, i, n):
    runs = CUT_RUNS if kind == "cut" else FLIP_RUNS
    assert sum(k for _, k in runs) == n
    for want, k in runs:
        if i < k:
            return want
        i -= k


@functools.lru_cache(maxsize=None)
def all_cases():
    del _cases[:]
    _cur[0] = 0
    for fam in (family_a, family_b, family_c, family_d, family_e, family_f, family_g, family_h):
        fam()
    names = [c.name for c in _cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    return tuple(_cases)


@functools.lru_cache(maxsize=None)
def batches():
    """{name: (D, cases)}: one D and one family per batch, at most 64 streams."""
    groups = defaultdict(list)
    for c in all_cases():
        groups[c.family, c.D].append(c)
    out = {}
    for (fam, D), cs in groups.items():
        for i in range(0, len(cs), 64):
            out["%s@%d#%d" % (fam, D, i // 64)] = (D, cs[i:i + 64])
    return out


def ring_census(R):
    """What the device ring of size R does over every valid case (at the case's D)."""
    cen = defaultdict(int)
    for c in all_cases():
        if c.want != "ok" or not c.exact:
            continue
        r = Ring(R, c.D)
        for t in c.trace:
            if r.pos >= c.D:
                break
            k = t["kind"]
            if k == "stored":
                r.copy_in(min(t["len"], c.D - r.pos))
            elif k == "lit":
                if t["state"] >= 7:
                    r.back(t["rep0"] + 1)
                r.put()
            elif k == "srep":
                r.back(t["rep0"] + 1)
                r.put()
            elif k in ("match", "rep"):
                r.copy(t["dist"] + 1, min(t["len"], c.D - r.pos))
        for e in r.log:
            if e[0] == "copy":
                _, pos, d, n, where, trig, wrap, safe = e
                cen["copy-" + where] += 1
                if -1 <= trig <= 1:
                    cen["trigger%+d" % trig] += 1
                cen["wrap-in-copy"] += wrap
                cen["wrap-in-copy-" + where] += wrap
                cen["unsafe"] += not safe
                if d < n:
                    cen["overlap"] += 1
            elif e[0] == "back":
                cen["back-" + e[3]] += 1
                cen["unsafe"] += not e[4]
            else:
                cen[e[0]] += 1
    return dict(cen)


@functools.lru_cache(maxsize=None)
def census():
    cen = dict(cases=defaultdict(int), want=defaultdict(int), pairs=set(), slots=set(), match_len=set(), rep_len=set(),
               first_diff=set(), props=set(), lit_ctx=set(), len_ctx=set(), rep_k=set(), controls=set())
    for c in all_cases():
        cen["cases"][c.family] += 1
        cen["want"][c.family, c.want] += 1
        for t in c.trace:
            k = t["kind"]
            if k in ("stored", "lzma"):
                continue
            cen["pairs"].add((t["state"], k))
            cen["props"].add(t["props"])
            if k in ("match", "eopm"):
                cen["slots"].add(t["slot"])
                cen["match_len"].add((t["len"], t["dpos"] & ((1 << t["props"][2]) - 1), t["props"][2]))
                cen["len_ctx"].add(min(t["len"] - 2, 3))
            elif k == "rep":
                cen["rep_len"].add((t["len"], t["dpos"] & ((1 << t["props"][2]) - 1), t["props"][2]))
                cen["rep_k"].add(t["k"])
            elif k == "lit":
                cen["lit_ctx"].add((t["dpos"] & ((1 << t["props"][1]) - 1), t["props"][1], t["props"][0]))
                if "first_diff" in t:
                    cen["first_diff"].add(t["first_diff"])
    cen["cases"], cen["want"] = dict(cen["cases"]), dict(cen["want"])
    return cen
