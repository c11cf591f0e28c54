"""The directed bzip2 encoder payloads.  TEST INFRASTRUCTURE ONLY.

The encoder (zarr_amd/csrc/zcg_bz2_enc.hip) decides by thresholds: how many
prefix bytes the first sort sees, which prefix groups fit the LDS sort and
which of its two sorts they get, how deep a tie may be before the global
prefix doubling takes it, when a block of equal rotations leaves the
doubling, where a 64-byte RLE1 step finds its block cut, how many Huffman
tables a block gets.  Generic payloads meet most of these by accident or not
at all.  Each case here is a batch of chunks of one length built to reach one
of them, and a witness: a statement about the CPU model of the batch
(tests/bz2_craft.py) which says that it does.  The witness is asserted in
tests/test_bz2_enc_cases_host.py; tests/test_gpu_bzip2_enc_craft.py encodes
the same batches on the GPU and takes the streams apart (tests/bz2_read.py).

A batch has one D, so blocks of different lengths in one sort come from RLE1
shrinkage and from the last blocks of chunks that have several.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from bz2_cases import norun_bytes
from bz2_craft import (adjacent_lcp, bwt, crc32_msb, crc_combine, huffman_lengths, mtf_rle2, mtf_rle2_serial,
                       orig_range, prefix_group_sizes, rle1_encode, rotation_ranks, symbol_count)
from bz2_read import read_stream

SUB_BYTES = 128 << 20   # input bytes per sort sub-batch (BZE_SUB_BYTES)
SUB_CHUNKS = 4096       # and chunks
LDS_TILE, LDS_MAX, ISORT = 1024, 2048, 64  # BZE_LC, BZE_LN, BZE_ISORT
LDS_DEPTH = 3 + 4 * 8   # bytes the LDS sort has compared after BZE_LROUNDS rounds behind a 3-byte prefix


def bmax(level: int) -> int:
    """RLE1 bytes a block may hold."""
    return 100000 * level - 19


# ---- the model of the block cuts --------------------------------------------------
def pieces(content: bytes) -> Tuple[np.ndarray, np.ndarray]:
    """RLE1 pieces of the content: (input bytes, RLE1 bytes) of each.  A run
    is cut into pieces of at most 255; a piece of four or more is four bytes
    and a count, a shorter one stands as it is."""
    a = np.frombuffer(content, np.uint8)
    if not len(a):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    lens = np.diff(np.r_[starts, len(a)])
    cnt = (lens + 254) // 255
    pin = np.full(int(cnt.sum()), 255, np.int64)
    last = np.cumsum(cnt) - 1
    pin[last] = lens - 255 * (cnt - 1)
    return pin, np.where(pin >= 4, 5, pin)


def rle1(content: bytes) -> bytes:
    """bz2_craft.rle1_encode, piece by piece in numpy (the block texts here
    are long and mostly without runs)."""
    pin, pout = pieces(content)
    if not len(pin):
        return b""
    first = np.frombuffer(content, np.uint8)[np.cumsum(pin) - pin]
    out = np.repeat(first, pout)
    counted = pin >= 4
    out[(np.cumsum(pout) - 1)[counted]] = pin[counted] - 4
    return out.tobytes()


def model_cuts(content: bytes, level: int) -> List[Tuple[int, int]]:
    """The blocks of a chunk as input ranges: each block takes whole pieces
    while its RLE1 bytes stay within bmax."""
    pin, pout = pieces(content)
    cin, cout = np.cumsum(pin), np.cumsum(pout)
    out = []
    s, base, at = 0, 0, 0
    while s < len(pin):
        e = int(np.searchsorted(cout, base + bmax(level), side="right"))
        assert e > s
        out.append((at, int(cin[e - 1])))
        s, base, at = e, int(cout[e - 1]), int(cin[e - 1])
    return out


def model_blocks(content: bytes, level: int) -> List[bytes]:
    """The block contents of a chunk."""
    return [content[a:b] for a, b in model_cuts(content, level)]


def cut_paths(content: bytes, level: int) -> List[str]:
    """How bze_rle1 finds each cut of the chunk: it walks the input 64 bytes
    at a step and cuts in the first step whose RLE1 bytes pass the block's
    limit, at the last piece start within the limit: "step" when that piece
    starts inside this step, "lastb" when it started in an earlier one."""
    a = np.frombuffer(content, np.uint8)
    D = len(a)
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    k = np.arange(D) - np.repeat(starts, np.diff(np.r_[starts, D]))
    q = k % 255
    ends = np.r_[a[1:] != a[:-1], True] | (q == 254)
    emitted = np.cumsum((q < 4).astype(np.int64) + (ends & (q >= 3)))
    step_end = emitted[np.minimum(np.arange(0, D, 64) + 64, D) - 1]
    cuts = model_cuts(content, level)
    out = []
    for (s, e) in cuts[:-1]:
        base = int(emitted[s - 1]) if s else 0
        w = 64 * int(np.searchsorted(step_end, base + bmax(level), side="right"))
        out.append("step" if e >= w else "lastb")
    return out


def sub_batches(D: int, n: int) -> List[int]:
    """Chunks per sort sub-batch (make_layout's m)."""
    m = max(1, min(SUB_BYTES // D if D else n, n, SUB_CHUNKS))
    return [min(m, n - c) for c in range(0, n, m)]


def prefix_bytes(nblocks: int) -> int:
    """dpre: prefix bytes of the first sort's 32-bit key beside the block index."""
    nb = 0
    while (1 << nb) < nblocks:
        nb += 1
    return min((32 - nb) // 8, 3)


def ngroups_rule(nmtf: int) -> int:
    """libbz2's number of coding tables for nMTF symbols (EOB included)."""
    return 2 if nmtf < 200 else 3 if nmtf < 600 else 4 if nmtf < 1200 else 5 if nmtf < 2400 else 6


# ---- cases ------------------------------------------------------------------------
@dataclass
class EncCase:
    """One encode call: chunks of one length (their serialised bytes, the
    content of the streams) and the witness.  `src` holds the bytes the
    device is given where they differ: the array's native layout for a
    byte-swapped dtype, the raw bytes of a bool array."""
    name: str
    level: int
    chunks: List[bytes]
    witness: Callable[["EncCase"], Dict]
    dt: str = "u1"
    src: Optional[List[bytes]] = None
    shifts: Sequence[int] = ()   # of a cut_phase case

    @property
    def D(self) -> int:
        return len(self.chunks[0])

    def texts(self) -> List[List[bytes]]:
        """The model's block texts (after RLE1) per chunk."""
        key = "_texts"
        if key not in self.__dict__:
            self.__dict__[key] = [[rle1(b) for b in model_blocks(c, self.level)] for c in self.chunks]
        return self.__dict__[key]

    def blocks_per_sub_batch(self) -> List[int]:
        out, c = [], 0
        per = [len(t) for t in self.texts()]
        for m in sub_batches(self.D, len(self.chunks)):
            out.append(sum(per[c:c + m]))
            c += m
        return out


@functools.lru_cache(maxsize=64)
def sort_stats(T: bytes, dpre: int = 3) -> Dict:
    """What the rotation sort meets in the block text T."""
    n = len(T)
    g = prefix_group_sizes(T, dpre)
    levels = rotation_ranks(T)
    lcp = adjacent_lcp(T, levels=levels) if n > 1 else np.zeros(0, np.int64)
    deepest = int(lcp[lcp < n].max()) if (lcp < n).any() else 0
    rounds = 0  # global rounds: h = dpre, 2 dpre, ... until 2h passes the deepest tie (or the block's length)
    if (lcp >= LDS_DEPTH).any() or (g > LDS_MAX).any():
        need = n if (lcp >= n).any() else deepest + 1
        while (dpre << rounds) < need and (dpre << rounds) < n:
            rounds += 1
        rounds = max(rounds, 1)
    return dict(n=n, groups=len(g), gmax=int(g.max()), g_le_isort=int((g <= ISORT).sum()),
                g_mid=int(((g > ISORT) & (g <= LDS_MAX)).sum()),
                g_tile_to_max=int(((g > LDS_TILE) & (g <= LDS_MAX)).sum()),
                g_gt_max=int((g > LDS_MAX).sum()), ties=int((lcp >= dpre).sum()), ties_gt35=int((lcp > 35).sum()),
                deepest=deepest, distinct=int(levels[-1][1].max()) + 1, rounds=rounds)


def _iid(n, k, seed):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint8).tobytes()


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _one_block_stats(case) -> List[Dict]:
    out = []
    for t in case.texts():
        assert len(t) == 1, case.name
        out.append(sort_stats(t[0]))
    assert prefix_bytes(sum(case.blocks_per_sub_batch())) == 3
    return out


# ---- sort cases ---------------------------------------------------------------------
def _w_insertion(case):
    st = _one_block_stats(case)
    for s in st:
        assert s["g_gt_max"] == 0 and s["groups"] - s["g_le_isort"] <= 1 and s["gmax"] <= 80, s
        assert s["deepest"] < LDS_DEPTH and s["rounds"] == 0, s
    return st


def _w_bitonic(case):
    st = _one_block_stats(case)
    for s in st:
        assert s["g_mid"] == s["groups"] and s["deepest"] < LDS_DEPTH and s["rounds"] == 0, s
    return st


def _w_straddle(case):
    st = _one_block_stats(case)
    for s in st:
        assert s["g_tile_to_max"] >= 1 and s["g_gt_max"] >= 1 and s["deepest"] < LDS_DEPTH, s
    return st


def _w_all_global(case):
    st = _one_block_stats(case)
    for s in st:
        assert s["g_gt_max"] >= 4 and s["deepest"] < LDS_DEPTH and s["rounds"] >= 1, s
    return st


def _w_deep(case):
    st = _one_block_stats(case)
    for s in st:
        assert 2 * s["ties_gt35"] > s["n"] - 1 and s["distinct"] == s["n"], s
    return st


def _w_two_halves(case):
    st = _one_block_stats(case)
    for s in st:
        assert s["distinct"] == s["n"] and s["deepest"] >= 29000 and s["rounds"] >= 13, s
        assert abs(2 * s["ties_gt35"] - s["n"]) < s["n"] // 50, s
    return st


def _w_periodic(distinct):
    def w(case):
        st = _one_block_stats(case)
        for s in st:
            assert s["distinct"] == distinct and s["n"] % distinct == 0, s
        return st
    return w


def _w_tiny(case):
    st = _one_block_stats(case)
    assert [s["distinct"] for s in st] == [2, 3, 3], st
    for s, c in zip(st, case.chunks):
        assert s["n"] == len(c) and orig_range(c)[1] == len(c) // s["distinct"]
    return st


def deep_ties_content(D=60000, seed=41):
    rng = np.random.default_rng(seed)
    motif = rng.integers(0, 256, 300, dtype=np.uint8)
    a = np.tile(motif, D // 300)
    at = np.arange(D // 300) * 300 + rng.integers(0, 300, D // 300)
    a[at] ^= rng.integers(1, 256, D // 300, dtype=np.uint8)
    return a.tobytes()


def _tiled(motif: bytes, D: int) -> bytes:
    assert D % len(motif) == 0
    return motif * (D // len(motif))


@functools.lru_cache(maxsize=None)
def sort_cases() -> List[EncCase]:
    half = _uniform(29999, 43)
    out = [
        EncCase("groups_insertion", 1, [_iid(52000, 11, s) for s in (1, 2)], _w_insertion),
        EncCase("groups_bitonic", 1, [_iid(60000, 8, s) for s in (3, 4)], _w_bitonic),
        EncCase("groups_straddle_2048", 1, [_iid(54000, 3, s) for s in (5, 6)], _w_straddle),
        EncCase("groups_all_global", 1, [_iid(60000, 2, s) for s in (7, 8)], _w_all_global),
        EncCase("deep_ties", 1, [deep_ties_content()], _w_deep),
        EncCase("two_halves", 1, [half + half + b"\x01\x02"], _w_two_halves),
        EncCase("periodic_1000x60", 1, [_tiled(_uniform(1000, 44), 60000)], _w_periodic(1000)),
        EncCase("periodic_ab", 1, [b"ab" * 30000], _w_periodic(2)),
    ]
    for D in (6, 12, 96):
        out.append(EncCase(f"tiny_periodic_D{D}", 1, [_tiled(b"ab", D), _tiled(b"abc", D), _tiled(b"aab", D)], _w_tiny))
    return out


def _w_mixed(case):
    """Short and long, periodic and aperiodic blocks in one sort: the
    blocks leave the doubling at different h."""
    st = [[sort_stats(t) for t in ts] for ts in case.texts()]
    flat = [s for ts in st for s in ts]
    assert prefix_bytes(len(flat)) == 3
    assert len({s["rounds"] for s in flat}) >= 4, [s["rounds"] for s in flat]
    assert any(s["distinct"] < s["n"] for s in flat) and any(s["distinct"] == s["n"] for s in flat)
    assert min(s["n"] for s in flat) < 3000 and max(s["n"] for s in flat) > 50000
    if case.D > bmax(case.level):
        assert any(len(ts) == 2 and ts[1]["n"] < ts[0]["n"] for ts in st)
    return st


def _mixed_chunks(D: int) -> List[bytes]:
    deep = deep_ties_content(60000)
    return [_tiled(b"ab", D), _tiled(b"abc", D), _uniform(D, 45), bytes(D - 10) + bytes(range(1, 11)), b"\xfb" * D,
            (deep * (D // len(deep) + 1))[:D]]


def _w_many_small(case):
    nb = case.blocks_per_sub_batch()
    assert len(nb) == 1 and nb[0] > 256 and prefix_bytes(nb[0]) == 2
    return dict(blocks_per_sub_batch=nb, dpre=2)


def _w_many_split(case):
    assert sub_batches(case.D, len(case.chunks)) == [4096, 904]
    nb = case.blocks_per_sub_batch()
    assert nb == [4096, 904] and prefix_bytes(nb[0]) == 2 and prefix_bytes(nb[1]) == 2
    return dict(blocks_per_sub_batch=nb, dpre=2)


def _small_kind(i: int, n: int) -> bytes:
    """Chunk i of a batch of many small chunks: eight kinds in turn."""
    k = i % 8
    if k == 0:
        return _iid(n, 4, 1000 + i)
    if k == 1:
        return norun_bytes(n, seed=i, k=5)
    if k == 2:
        return _tiled(b"ab", n)
    if k == 3:
        return np.random.default_rng(i).integers(0, 3, (n + 6) // 7).astype(np.uint8).repeat(7)[:n].tobytes()
    if k == 4:
        return bytes([i & 0xFF]) * n
    if k == 5:
        return _iid(n, 16, 2000 + i)
    if k == 6:
        return (norun_bytes(n // 4, seed=i, k=3) * 4 + bytes(n))[:n]
    return np.cumsum(np.random.default_rng(i).integers(-1, 2, n)).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def batch_cases() -> List[EncCase]:
    return [
        EncCase("mixed_lengths_D60000", 1, _mixed_chunks(60000), _w_mixed),
        EncCase("mixed_lengths_D150000", 1, _mixed_chunks(150000), _w_mixed),
        EncCase("many_blocks_small", 1, [_small_kind(i, 2000) for i in range(300)], _w_many_small),
        EncCase("many_chunks_split", 1, [_small_kind(i, 64) for i in range(5000)], _w_many_split),
    ]


# ---- RLE1 / cut cases -------------------------------------------------------------------
CUT_OFFSETS = tuple(range(-6, 2))
CUT_SHIFTS = (0, 1, 31, 63)
# the first block's RLE1 bytes when a run of 300 (pieces of 255 and 45, five
# RLE1 bytes each) starts at RLE1 offset bmax + o: o = -6 cuts between the two
# pieces, -5 behind the first, which ends exactly at bmax; -4..-1 in front of
# the run, whose first piece would straddle bmax; at 0 the run starts the
# next block, at +1 the byte in front of it does
CUT_FIRST_LEN = {-6: -1, -5: 0, -4: -4, -3: -3, -2: -2, -1: -1, 0: 0, 1: 0}


def cut_phase_chunk(level: int, o: int, shift: int, D: int) -> bytes:
    """A run of 4 + shift bytes (five RLE1 bytes whatever the shift, so the
    shift moves the input against the 64-byte steps and leaves the RLE1
    offsets alone), filler without runs up to RLE1 offset bmax + o, a run of
    300, filler."""
    head = b"\xc8" * (4 + shift)
    fill = norun_bytes(bmax(level) + o - 5, seed=level * 100 + o + 6, k=12)
    c = head + fill + b"\xd7" * 300
    return c + norun_bytes(D - len(c), seed=7, k=12, base=0x60)


def _w_cut_phase(case):
    res = []
    phases = set()
    i = 0
    assert len(case.chunks) == len(CUT_OFFSETS) * len(case.shifts)
    for o in CUT_OFFSETS:
        for shift in case.shifts:
            c = case.chunks[i]
            i += 1
            cuts = model_cuts(c, case.level)
            assert len(cuts) == 2
            t0 = rle1_encode(c[:cuts[0][1]])
            assert len(t0) == bmax(case.level) + CUT_FIRST_LEN[o], (o, shift, len(t0))
            run_at = c.index(b"\xd7" * 300)
            assert len(rle1_encode(c[:run_at])) == bmax(case.level) + o
            phases.add((o, run_at % 64))
            res.append(dict(o=o, shift=shift, first_len=len(t0), run_phase=run_at % 64,
                            path=cut_paths(c, case.level)[0]))
    assert len(phases) == len(case.chunks)
    assert {r["path"] for r in res} == {"step", "lastb"}, res
    return res


def long_run_chunk(level: int, start: int, D: int, shift: int = 0) -> bytes:
    """A run of 12 000 from RLE1 offset `start` on (a piece boundary every 255
    input bytes, every 5 RLE1 bytes), behind a run of 4 + shift as above."""
    head = b"\xc8" * (4 + shift)
    c = head + norun_bytes(start - 5, seed=start, k=12) + b"\xd7" * 12000
    return c + norun_bytes(D - len(c), seed=9, k=12, base=0x60)


LONG_RUN_STARTS = tuple(range(-104, -99))  # against bmax: 20 pieces end at bmax - 4 .. bmax
LONG_RUN_COUNT_LANES = (63, 0, 62)


def _w_long_run(case):
    """With 0..3 bytes left the next piece's four bytes pass the limit in the
    step where it starts ("step"); with 4 left they fit, and the step of its
    count byte, 254 bytes on, finds no piece start within the limit and falls
    back on the one it remembered ("lastb")."""
    res = []
    for c in case.chunks:
        cuts = model_cuts(c, case.level)
        assert len(cuts) == 2
        e = cuts[0][1]
        assert c[e - 1] == 0xD7 and c[e] == 0xD7, "the cut is not inside the run"
        res.append(dict(first_len=len(rle1_encode(c[:e])), cut_at=e, count_lane=(e + 254) % 64,
                        path=cut_paths(c, case.level)[0]))
    assert [r["path"] for r in res] == ["lastb"] + ["step"] * 4 + ["lastb"] * 3, res
    assert [r["first_len"] for r in res] == [bmax(case.level) - 4 + i for i in range(5)] + [bmax(case.level) - 4] * 3
    assert tuple(r["count_lane"] for r in res[5:]) == LONG_RUN_COUNT_LANES, res
    return res


RUN_LENGTHS = (3, 4, 5, 254, 255, 256, 259, 509, 510, 511, 765)
RUN_PHASES = (0, 1, 62, 63)


def run_phases_chunk(seed: int) -> bytes:
    out = bytearray()
    rng = np.random.default_rng(seed)
    k = 0
    for ph in RUN_PHASES:
        for ln in RUN_LENGTHS:
            pad = (ph - len(out) - 1) % 64 + 1  # at least one byte between two runs
            out += norun_bytes(pad, seed=int(rng.integers(1 << 30)), k=9, base=0x40 + 16 * (k & 1))
            out += bytes([0x10 + (k % 3) + seed]) * ln
            k += 1
    return bytes(out)


def _runs(content: bytes) -> List[Tuple[int, int]]:
    a = np.frombuffer(content, np.uint8)
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    lens = np.diff(np.r_[starts, len(a)])
    return [(int(s), int(l)) for s, l in zip(starts, lens) if l >= 3]


def _w_run_phases(case):
    for c in case.chunks:
        got = {(l, s % 64) for s, l in _runs(c)}
        assert got == {(l, p) for l in RUN_LENGTHS for p in RUN_PHASES}, sorted(got)
    return dict(runs=len(RUN_LENGTHS) * len(RUN_PHASES), D=case.D)


TAIL_RUNS = (1, 3, 4, 5, 255, 256)
TAIL_D = (1024, 1025, 1087)


def _w_tail_runs(case):
    assert case.D % 64 in (0, 1, 63)
    tails = []
    for c in case.chunks:
        s, l = ([(len(c) - 1, 1)] + [r for r in _runs(c) if r[0] + r[1] == len(c)])[-1]
        tails.append(l)
    assert tuple(tails) == TAIL_RUNS, tails
    return dict(D=case.D, tails=tails)


def _swapped(dt: str, values: np.ndarray) -> Tuple[bytes, bytes]:
    """(serialised bytes, native bytes as the device gets them)."""
    return values.astype(np.dtype(dt)).tobytes(), values.astype(np.dtype(dt).newbyteorder("=")).tobytes()


def _w_swapped(case):
    res = []
    for c, s in zip(case.chunks, case.src):
        long_runs = [l for _, l in _runs(c) if l >= 4]
        assert len(long_runs) >= 3 and max(long_runs) > 255, long_runs
        assert c != s
        res.append(dict(runs=len(long_runs), longest=max(long_runs)))
    return res


@functools.lru_cache(maxsize=None)
def rle1_cases() -> List[EncCase]:
    out = []
    D1 = bmax(1) + 700
    for sh in CUT_SHIFTS:
        out.append(EncCase(f"cut_phase_level1_shift{sh}", 1, [cut_phase_chunk(1, o, sh, D1) for o in CUT_OFFSETS],
                           _w_cut_phase, shifts=(sh,)))
    D2 = bmax(2) + 700
    out.append(EncCase("cut_phase_level2", 2, [cut_phase_chunk(2, o, 0, D2) for o in CUT_OFFSETS], _w_cut_phase,
                       shifts=(0,)))
    DL = bmax(1) + 13000
    chunks = [long_run_chunk(1, bmax(1) + s, DL) for s in LONG_RUN_STARTS]
    # the count byte that passes the limit in the last lane of a step (the next
    # piece starts in the step after it), in the first and in lane 62
    last = chunks[0].index(b"\xd7" * 12000) + 21 * 255 - 1
    for lane in LONG_RUN_COUNT_LANES:
        chunks.append(long_run_chunk(1, bmax(1) + LONG_RUN_STARTS[0], DL, shift=(lane - last) % 64))
    out.append(EncCase("cut_in_long_run", 1, chunks, _w_long_run))
    rp = [run_phases_chunk(0), run_phases_chunk(1)]
    Dr = max(len(c) for c in rp) + 3
    out.append(EncCase("run_phases", 1, [c + norun_bytes(Dr - len(c), seed=3, k=5, base=0x80) for c in rp],
                       _w_run_phases))
    for D in TAIL_D:
        out.append(EncCase(f"tail_runs_D{D}", 1,
                           [norun_bytes(D - r, seed=D + r, k=9) + b"\xee" * r for r in TAIL_RUNS], _w_tail_runs))
    # byte-swapped dtypes: constant stretches between ramps
    n = 6000
    ramp = np.arange(n, dtype=np.int64)
    v4 = np.where((ramp // 700) % 2 == 0, 0x01010101, ramp * 0x01000193 % (1 << 32))
    c, s = _swapped(">u4", v4)
    out.append(EncCase("swapped_runs_u4", 1, [c], _w_swapped, dt=">u4", src=[s]))
    v2 = np.where((ramp // 900) % 2 == 0, 0x0202, np.where(ramp % 5 == 0, 0x0100, ramp % 30000)).astype(np.int64)
    c, s = _swapped(">i2", v2)
    out.append(EncCase("swapped_runs_i2", 1, [c], _w_swapped, dt=">i2", src=[s]))
    raw = np.array([0, 1, 2, 255], np.uint8)[np.random.default_rng(46).integers(0, 4, n // 3)].repeat(3)
    raw[1000:1400] = 0
    raw[2000:2300] = np.array([1, 2, 255], np.uint8)[np.arange(300) % 3]  # one run of 300 once normalised
    raw[3000:3004] = (2, 255, 1, 2)
    out.append(EncCase("swapped_runs_bool", 1, [(raw != 0).astype(np.uint8).tobytes()], _w_swapped, dt="bool",
                       src=[raw.tobytes()]))
    return out


# ---- table cases -------------------------------------------------------------------------
NGROUPS_NMTF = (199, 200, 599, 600, 1199, 1200, 2399, 2400)
NGROUPS_D = 4000


def _nmtf_chunk(n: int, seed: int) -> bytes:
    """n bytes without runs, then one long run up to NGROUPS_D (a few RLE1
    bytes whatever its length): the block's symbol count follows n."""
    return norun_bytes(n, seed=seed, k=4) + b"\xf0" * (NGROUPS_D - n)


def _nmtf(content: bytes) -> int:
    return symbol_count(bwt(rle1_encode(content))[0])


@functools.lru_cache(maxsize=None)
def chunk_with_nmtf(target: int) -> bytes:
    """A chunk of NGROUPS_D bytes whose one block has exactly `target`
    symbols (EOB included): bisect on n, then look around it."""
    for seed in range(16):
        lo, hi = 1, NGROUPS_D - 8
        while lo < hi:
            mid = (lo + hi) // 2
            if _nmtf(_nmtf_chunk(mid, seed)) < target:
                lo = mid + 1
            else:
                hi = mid
        for n in range(max(1, lo - 24), min(NGROUPS_D - 8, lo + 24)):
            c = _nmtf_chunk(n, seed)
            if _nmtf(c) == target:
                return c
    raise ValueError(target)


def _w_ngroups(case):
    nm = [_nmtf(c) for c in case.chunks]
    assert tuple(nm) == NGROUPS_NMTF
    assert [ngroups_rule(x) for x in nm] == [2, 3, 3, 4, 4, 5, 5, 6]
    return dict(nmtf=nm, ngroups=[ngroups_rule(x) for x in nm])


def deep_counts(k: int = 18, margin: float = 1.1) -> List[int]:
    """Counts of the MTF ranks 1..k for a code deeper than 17 bits: beside
    RUNA, RUNB and EOB (weight 1 each in the encoder) every count passes the
    sum of all counts but the one before it by the margin, so the Huffman
    tree is a chain, k + 2 deep, and stays one when a few counts move by
    one or two.  (Fibonacci counts are the limit of this rule without a
    margin: any tie flattens their tree.)"""
    w = [1, 1, 1, 4]
    while len(w) < k + 3:
        w.append(max(int(margin * (sum(w) - w[-1])) + 2, w[-1] + 2))
    return w[3:]


def _walk(L: np.ndarray):
    """The cycles of L's inverse-BWT links: (count, cycle of each row, the
    rows of the walk from row 0 in text order, the links)."""
    link = np.argsort(L, kind="stable")
    ll = link.tolist()
    cyc = [-1] * len(L)
    ncyc, rows0 = 0, None
    for s in range(len(L)):
        if cyc[s] >= 0:
            continue
        p, rows = s, []
        while cyc[p] < 0:
            cyc[p] = ncyc
            rows.append(p)
            p = ll[p]
        if s == 0:
            rows0 = rows
        ncyc += 1
    return ncyc, np.array(cyc), np.array(rows0), link


@functools.lru_cache(maxsize=None)
def deep_codes_content(k: int = 18, margin: float = 1.1) -> bytes:
    """A block whose symbols have deep_counts: the ranks, no zero among
    them, each spread evenly over the block (so that every group of 50
    prefers the same table and one table codes them all); L by undoing the
    move-to-front; then adjacent unequal bytes of L are swapped, which moves
    a few ranks by one, until L's links are one cycle (a swap between two
    cycles joins them) and the text has no run of four (a swap at the row
    that starts inside the run; it may split the cycle again).  The text of
    a one-cycle L from row 0 has L as its last column and origPtr 0."""
    c = deep_counts(k, margin)
    n = sum(c)
    keys = np.concatenate([(np.arange(x) + 0.37 + 0.01 * r) / x for r, x in enumerate(c)])
    ranks = np.repeat(np.arange(1, k + 1), c)[np.argsort(keys, kind="stable")]
    mtf = [0x41 + i for i in range(k + 1)]
    L = bytearray()
    for r in ranks.tolist():
        b = mtf.pop(r)
        mtf.insert(0, b)
        L.append(b)
    L = np.frombuffer(bytes(L), np.uint8).copy()
    for _ in range(2000):
        ncyc, cyc, rows, link = _walk(L)
        if ncyc > 1:
            inv = np.empty(n, np.int64)
            inv[link] = np.arange(n)
            cand = np.flatnonzero((L[:-1] != L[1:]) & (cyc[inv[:-1]] != cyc[inv[1:]]))
            i = int(cand[len(cand) // 2])
            L[i], L[i + 1] = L[i + 1], L[i]
            continue
        T = L[link[rows]]
        t = np.concatenate((T, T[:3]))
        runs = np.flatnonzero((t[:-3] == t[1:-2]) & (t[:-3] == t[2:-1]) & (t[:-3] == t[3:]))
        if not len(runs):
            return T.tobytes()
        r = int(rows[(runs[0] + 1) % n])  # the row of the rotation from the run's second byte: its L is the first
        o = r + 1 if r + 1 < n and L[r + 1] != L[r] else r - 1
        L[r], L[o] = L[o], L[r]
    raise ValueError("no text found")


def table_depths(stream: bytes) -> List[Tuple[int, int, int]]:
    """Per table of the stream's first block: (symbols it coded, its longest
    code, the longest code of an unrestricted Huffman tree over the counts
    of those symbols, 0 for a table that coded none)."""
    b = read_stream(stream)[1][0]
    sy = np.array(b.symbols)
    sel = np.array(b.selectors)[np.arange(len(sy)) // 50]
    out = []
    for t in range(b.ngroups):
        cnt = np.bincount(sy[sel == t], minlength=len(b.used) + 2)
        out.append((int(cnt.sum()), max(b.lengths[t]), max(huffman_lengths(cnt, limit=10**9)) if cnt.sum() else 0))
    return out


def _w_deep_codes(case):
    """Under the model: the block is its own RLE1 text, and a Huffman tree
    over its symbol counts is deeper than 17.  That a table of the encoder
    meets these counts is asserted on its stream (table_depths)."""
    T = case.chunks[0]
    assert rle1(T) == T and len(T) <= bmax(case.level)
    L, orig = bwt(T)
    used = sorted(set(T))
    cnt = np.bincount(mtf_rle2(L, used), minlength=len(used) + 2)
    depth = max(huffman_lengths(cnt, limit=10**9))
    assert orig == 0 and cnt[0] + cnt[1] <= 8 and depth >= 19, (orig, cnt.tolist(), depth)
    assert np.abs(cnt[2:-1] - np.array(deep_counts())).max() <= 4
    return dict(n=len(T), counts=cnt.tolist(), unrestricted_depth=depth)


@functools.lru_cache(maxsize=None)
def table_cases() -> List[EncCase]:
    return [EncCase("ngroups_each", 1, [chunk_with_nmtf(t) for t in NGROUPS_NMTF], _w_ngroups),
            EncCase("deep_codes", 1, [deep_codes_content()], _w_deep_codes)]


# ---- what a stream of the encoder must be ----------------------------------------------------
def _first_piece(content: bytes) -> int:
    """RLE1 bytes of the first piece of a block's content."""
    a = np.frombuffer(content[:255], np.uint8)
    d = np.flatnonzero(a != a[0])
    p = int(d[0]) if len(d) else len(a)
    return 5 if p >= 4 else p


def check_stream(stream: bytes, content: bytes, level: int, ours: bool = True, at=None):
    """Takes the stream apart and compares every stage with the model, all
    by equality: the cuts (those of model_cuts: whole RLE1 pieces, within
    bmax, and as late as bze_rle1 cuts, the next block's first piece would
    not have fitted; for
    a stream of libbz2's, `ours` unset, which closes a block a few bytes
    past bmax when a run ends there, within the level's 100 000 L
    instead), the block and stream CRCs, L, origPtr (among
    the sorted positions of the rotations equal to the text, one position
    unless the text is periodic), the symbol map, the symbols, libbz2's
    table count and the selector count, selectors and lengths in range.
    Returns the blocks."""
    lv, blocks, comb, pad = read_stream(stream)
    assert lv == level and pad < 8, (at, "level or padding", lv, pad)
    assert b"".join(b.content for b in blocks) == content, (at, "content")
    if ours:
        want = [e - s for s, e in model_cuts(content, level)]
        assert [len(b.content) for b in blocks] == want, (at, "cuts", [len(b.content) for b in blocks], want)
    c = 0
    for i, b in enumerate(blocks):
        where = (at, "block", i)
        assert b.randomised == 0, where + ("randomised",)
        assert rle1(b.content) == b.T, where + ("cut inside a piece",)
        assert len(b.T) <= (bmax(level) if ours else 100000 * level), where + ("too long", len(b.T))
        if ours and i + 1 < len(blocks):
            assert len(b.T) + _first_piece(blocks[i + 1].content) > bmax(level), where + ("cut early", len(b.T))
        assert b.crc == crc32_msb(b.content), where + ("crc",)
        c = crc_combine(c, b.crc)
        n = len(b.T)
        a = np.frombuffer(b.T, np.uint8)
        rank = rotation_ranks(b.T)[-1][1]
        sa = np.argsort(rank, kind="stable")
        L = a[(sa - 1) % n].tobytes()
        assert b.L == L, where + ("L",)
        first, count = int((rank < rank[0]).sum()), int((rank == rank[0]).sum())
        assert first <= b.orig < first + count, where + ("origPtr", b.orig, first, count)
        used = sorted(set(b.T))
        assert b.used == used, where + ("symbol map",)
        syms = mtf_rle2_serial(L, used) if n < 512 else mtf_rle2(L, used).tolist()
        assert b.symbols == syms, where + ("symbols",)
        assert b.ngroups == ngroups_rule(len(syms)), where + ("nGroups", b.ngroups, len(syms))
        assert b.nselectors == -(-len(syms) // 50), where + ("nSelectors", b.nselectors, len(syms))
        assert all(0 <= t < b.ngroups for t in b.selectors), where + ("selectors",)
        assert len(b.lengths) == b.ngroups and all(1 <= l <= 17 for tab in b.lengths for l in tab), where + ("lengths",)
    assert comb == c, (at, "combined crc")
    return blocks


SORT_NAMES = ("groups_insertion", "groups_bitonic", "groups_straddle_2048", "groups_all_global", "deep_ties",
              "two_halves", "periodic_1000x60", "periodic_ab", "tiny_periodic_D6", "tiny_periodic_D12",
              "tiny_periodic_D96")
BATCH_NAMES = ("mixed_lengths_D60000", "mixed_lengths_D150000", "many_blocks_small", "many_chunks_split")
RLE1_NAMES = ("cut_phase_level1_shift0", "cut_phase_level1_shift1", "cut_phase_level1_shift31",
              "cut_phase_level1_shift63", "cut_phase_level2", "cut_in_long_run", "run_phases", "tail_runs_D1024",
              "tail_runs_D1025", "tail_runs_D1087", "swapped_runs_u4", "swapped_runs_i2", "swapped_runs_bool")
TABLE_NAMES = ("ngroups_each", "deep_codes")
_GROUPS = ((SORT_NAMES, sort_cases), (BATCH_NAMES, batch_cases), (RLE1_NAMES, rle1_cases), (TABLE_NAMES, table_cases))
CASE_NAMES = SORT_NAMES + BATCH_NAMES + RLE1_NAMES + TABLE_NAMES  # (the tests are collected without building a payload)


def all_cases() -> List[EncCase]:
    return [c for _, build in _GROUPS for c in build()]


def case(name: str) -> EncCase:
    """The case of that name; builds its group only."""
    build, = [b for names, b in _GROUPS if name in names]
    return {c.name: c for c in build()}[name]
