"""The crafted bzip2 cases.  TEST INFRASTRUCTURE ONLY.

Content generators and the case matrices built with the block-level writer
(tests/bz2_craft.py): the nblock ladder in content and raw form, `tail4`
blocks, the group / code length / selector knobs, zero runs, stream shapes,
sampling edges, and the multi-block streams of the whole-stream and
randomised GPU tests.  tests/test_bz2_craft_host.py runs them through the
host core, tests/test_gpu_bzip2_craft.py through the kernels.
"""
import functools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from bz2_craft import (BLOCK_MAGIC, Block, bwt, chain_bytes, is_one_cycle, rle1_decode, rle1_state, symbol_count,
                       write_stream, write_stream_info)

# ---- content generators -------------------------------------------------------
def norun_bytes(n: int, seed: int = 0, k: int = 7, base: int = 0x40) -> bytes:
    """n bytes over k symbols, no two neighbours equal (RLE1 leaves them as
    they are, so block and content are the same bytes)."""
    if n == 0:
        return b""
    r = np.random.default_rng(seed).integers(1, k, n)
    return (base + np.cumsum(r) % k).astype(np.uint8).tobytes()


def closed(T: bytes) -> bytes:
    """T with its last byte changed, if need be, so that it does not end
    right after a run of four."""
    if rle1_state(T) != 4:
        return T
    return T[:-1] + bytes([T[-1] ^ 0x10])


ALPHABETS = ("two", "five_doubled", "all256", "three_runs6")


def alphabet_T(kind: str, n: int, seed: int) -> bytes:
    """A block of exactly n bytes (after RLE1) in one of the ladder's alphabets."""
    rng = np.random.default_rng(seed)
    if kind == "two":
        t = np.array([3, 5], np.uint8)[rng.integers(0, 2, n)]
    elif kind == "five_doubled":
        t = np.array([1, 2, 6, 9, 200], np.uint8)[rng.integers(0, 5, (n + 1) // 2)].repeat(2)[:n]
    elif kind == "all256":
        t = rng.integers(0, 256, n).astype(np.uint8)
        if n >= 256:
            t[:256] = rng.permutation(256)
    elif kind == "three_runs6":
        t = np.array([2, 5, 9], np.uint8)[rng.integers(0, 3, (n + 5) // 6)].repeat(6)[:n]
    else:
        raise ValueError(kind)
    return closed(t.tobytes())


@functools.lru_cache(maxsize=None)
def filler(n: int) -> Block:
    return Block(T=norun_bytes(n, seed=n), plain=True)


# ---- cases --------------------------------------------------------------------
@dataclass
class Case:
    """A stream of `blocks` (plus `suffix` bytes) to be decoded to D bytes.
    at(Dbatch) is the same case behind a filler block, so that the decode
    ends at the same place of the same blocks with D = Dbatch (a batch of
    cases shares one D).  A `bare` case goes into a batch as it is (the
    empty stream has to stay empty)."""
    name: str
    blocks: Sequence[Block]
    D: int
    level: int = 1
    suffix: bytes = b""
    bare: bool = False
    _cache: dict = field(default_factory=dict)

    def stream(self) -> bytes:
        if "s" not in self._cache:
            self._cache["s"] = write_stream(self.blocks, self.level)
        return self._cache["s"][0] + self.suffix

    def expected(self) -> Optional[bytes]:
        self.stream()
        return self._cache["s"][1]

    def at(self, Dbatch: int) -> bytes:
        if self.bare:
            return self.stream()
        assert self.D <= Dbatch
        pre = [filler(Dbatch - self.D)] if Dbatch > self.D else []
        return write_stream(pre + list(self.blocks), self.level)[0] + self.suffix


LADDER_NBLOCK = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4097)


@functools.lru_cache(maxsize=None)
def ladder_content_cases() -> List[Case]:
    out = []
    for n in LADDER_NBLOCK:
        for rnd in (0, 1):
            for ai, kind in enumerate(ALPHABETS):
                blk = Block(T=alphabet_T(kind, n, seed=n * 8 + ai), randomised=rnd)
                ln = len(rle1_decode(blk.T))
                for D in (ln, ln + 1, ln - 1, ln // 2):
                    out.append(Case(f"content-n{n}-r{rnd}-{kind}-D{D}", [blk], D))
    return out


@functools.lru_cache(maxsize=None)
def ladder_raw_cases() -> List[Case]:
    """L drawn at random (hardly ever one cycle), origPtr in and out of range."""
    out = []
    for n in LADDER_NBLOCK:
        for rnd in (0, 1):
            for ai, kind in enumerate(ALPHABETS):
                L = alphabet_T(kind, n, seed=1000 + n * 8 + rnd * 4 + ai)
                for orig in (0, n - 1, n // 2, n, n + 5):
                    for D in (1, n // 2 + 1, n, 5 * n):
                        out.append(Case(f"raw-n{n}-r{rnd}-{kind}-o{orig}-D{D}",
                                        [Block(L=L, orig=orig, crc=0x12345678, randomised=rnd)], D))
    return out


TAIL4_NBLOCK = (4, 5, 100, 260, 616, 617, 618, 1337)


@functools.lru_cache(maxsize=None)
def tail4_cases() -> List[Case]:
    """Blocks that end in a run of four without its count byte.  The count
    libbz2 reads instead is the block's first byte (XOR the schedule's mask
    of position nblock when randomised); D sweeps from one below the block's
    regular output to 12 past it, across both candidate run ends."""
    out = []
    for n in TAIL4_NBLOCK:
        for rnd in (0, 1):
            for first in (2, 3, 7):
                if n == 4:
                    T = bytes([first]) * 4
                else:
                    T = bytes([first]) + norun_bytes(n - 5, seed=n, k=5, base=0x60) + b"\x11" * 4
                assert len(T) == n and rle1_state(T) == 4
                blk = Block(T=T, randomised=rnd)
                ln = len(rle1_decode(T))
                for D in range(ln - 1, ln + 13):
                    out.append(Case(f"tail4-n{n}-r{rnd}-f{first}-D{D}", [blk], D))
    return out


@functools.lru_cache(maxsize=None)
def walk_tail4_cases() -> List[Case]:
    """`tail4` on a chain that is not one cycle: the walk's block ends in a
    run of four, and the count byte, chain position nblock, is not the
    block's first byte, because the cycle walked is shorter than the block
    and does not divide it.  Found by drawing L at random."""
    out = []
    rng = np.random.default_rng(2024)
    for n in (23, 37, 617):
        for rnd in (0, 1):
            while True:
                L = np.array([2, 3, 7], np.uint8)[rng.integers(0, 3, n)].tobytes()
                orig = int(rng.integers(0, n))
                T = chain_bytes(L, orig, n + 1)
                if rle1_state(T[:n]) == 4 and T[n] != T[0] and not is_one_cycle(L, orig):
                    break
            ln = len(rle1_decode(T[:n]))
            for D in range(ln - 1, ln + 10):
                out.append(Case(f"walk-tail4-n{n}-r{rnd}-D{D}", [Block(L=L, orig=orig, crc=0, randomised=rnd)], D))
    return out


@functools.lru_cache(maxsize=None)
def block_with_symbols(nsyms: int) -> bytes:
    """A block without runs whose Huffman stage has exactly nsyms symbols
    (EOB included), found by trying lengths and seeds."""
    for n in range(1, 4 * nsyms):
        for seed in range(8):
            T = norun_bytes(n, seed=seed, k=3)
            if symbol_count(bwt(T)[0]) == nsyms:
                return T
    raise ValueError(nsyms)


def _knob_T(n=700, seed=77):
    return alphabet_T("five_doubled", n, seed)


@functools.lru_cache(maxsize=None)
def knob_cases() -> List[Case]:
    """The group, code length, table order and selector knobs; the invalid
    group counts; a block whose every used byte sits at MTF depth 255."""
    out = []
    T = _knob_T()
    ln = len(rle1_decode(T))
    T256 = alphabet_T("all256", 3000, 5)
    ln256 = len(rle1_decode(T256))

    def add(name, blk, D):
        out.append(Case("knob-" + name, [blk], D))

    for ng in range(2, 7):
        add(f"ng{ng}-huffman", Block(T=T, ngroups=ng), ln)
        add(f"ng{ng}-reverse", Block(T=T, ngroups=ng, order=list(range(ng))[::-1], randomised=ng & 1), ln)
        add(f"ng{ng}-len9-all256", Block(T=T256, ngroups=ng, lengths=9), ln256)
    for ng in (0, 1, 7):
        add(f"ng{ng}-invalid", Block(T=T, ngroups=ng), ln)
    for eq in (8, 17, 20):
        add(f"len{eq}", Block(T=T, ngroups=3, lengths=eq), ln)
        add(f"len{eq}-6groups", Block(T=T, ngroups=6, lengths=eq, order=[5, 0, 3, 1, 4, 2]), ln)
    for eq in (9, 17, 20):
        add(f"len{eq}-all256", Block(T=T256, ngroups=6, lengths=eq, order=[2, 5, 1]), ln256)
    add("huffman-all256", Block(T=T256, ngroups=6), ln256)
    add("one-table-of-six", Block(T=T, ngroups=6, order=[4]), ln)
    for extra in (1, 7, 300, 18002, 18060):
        add(f"surplus{extra}", Block(T=T, ngroups=4, extra_selectors=extra), ln)
        add(f"surplus{extra}-short", Block(T=T, ngroups=4, extra_selectors=extra), ln // 2)
    # the last selector of a block covers 1..50 symbols: 2, 3, 49, 50, then
    # 1 and 50 again behind full selectors
    for nsyms in (2, 3, 49, 50, 51, 100, 101):
        t = block_with_symbols(nsyms)
        add(f"syms{nsyms}", Block(T=t, ngroups=2), len(t))
        add(f"syms{nsyms}-6groups-len20", Block(T=t, ngroups=6, lengths=20, order=[5, 4, 3, 2, 1, 0]), len(t))
    # one symbol in the only selector: EOB alone, an empty block (invalid: origPtr >= nblock)
    add("eob-only", Block(L=b"", orig=0, crc=0, used_extra=[65]), 1)
    # every byte value used; L cycles through them, so each symbol is taken
    # from MTF depth 255 (raw form: the bytes are compared while D is inside)
    cyc = np.tile(np.arange(256, dtype=np.uint8), 6).tobytes()
    for D in (1, 700, 1535):
        add(f"mtf255-D{D}", Block(L=cyc, orig=3, crc=0, ngroups=6, lengths=9, order=[0, 5]), D)
        add(f"mtf255-huff-D{D}", Block(L=cyc[::-1], orig=1535, crc=0, ngroups=2, randomised=1), D)
    # unused bytes marked as used: all 256 in the symbol map, few in L
    add("map256", Block(T=T, ngroups=2, used_extra=range(256)), ln)
    add("map256-len20", Block(T=T, ngroups=5, lengths=20, used_extra=range(256)), ln)
    return out


@functools.lru_cache(maxsize=None)
def zero_run_cases() -> List[Case]:
    """Zero runs (RUNA/RUNB) of 1..70 and 255..260 in L, starting at every
    residue of 4 and spread over the residues of 64 (raw form; D inside)."""
    out = []
    for off in range(4):
        parts = [bytes([0x41]) * off] if off else []
        for i, r in enumerate(list(range(1, 71)) + list(range(255, 261))):
            # a run of r equal bytes is one MTF symbol and a zero run of r - 1;
            # a run at the start of L of the front byte is a zero run of r
            parts.append(bytes([0x30 + (i % 3)]) * (r + 1))
            parts.append(bytes([0x50 + (i % 5)]) * (1 + (i * 7 + off) % 5))
        L = b"".join(parts)
        for D in (len(L) // 2, 17):
            out.append(Case(f"zrun-off{off}-D{D}", [Block(L=L, orig=off, crc=0, ngroups=2 + off)], D))
        out.append(Case(f"zrun-front-off{off}", [Block(L=bytes([0x30]) * (64 + off) + L, orig=1, crc=0)], 40))
    # and in a valid block: long runs in T survive the BWT as long runs in L
    T = closed(b"".join(bytes([65 + i % 3]) * 3 + bytes([70 + i % 2]) * 2 for i in range(900)))
    out.append(Case("zrun-valid", [Block(T=T, ngroups=3)], len(rle1_decode(T))))
    return out


@functools.lru_cache(maxsize=None)
def stream_shape_cases() -> List[Case]:
    """60 tiny blocks alternating randomised, the empty stream, trailing
    garbage, and a second stream after the first."""
    out = []
    tiny = [Block(T=alphabet_T(ALPHABETS[i % 4], 1 + i % 9, seed=i), randomised=i & 1) for i in range(60)]
    ln = sum(len(rle1_decode(b.T)) for b in tiny)
    for D in (ln, ln - 1, ln + 1, ln // 2):
        out.append(Case(f"tiny60-D{D}", tiny, D))
    # the empty stream as it is: stage A's first call parses the header and
    # meets the end record at once, whatever D the batch has
    out.append(Case("empty-bare", [], 5, bare=True))
    out.append(Case("empty-garbage-bare", [], 5, suffix=b"\x31\x41\x59garbage", bare=True))
    out.append(Case("empty-magic-bare", [], 5, suffix=BLOCK_MAGIC.to_bytes(6, "big") + bytes(9), bare=True))
    for D in (0, 1, 5):
        out.append(Case(f"empty-D{D}", [], D))
        out.append(Case(f"empty-garbage-D{D}", [], D, suffix=b"\x31\x41\x59garbage"))
    T = _knob_T(300, 9)
    one = [Block(T=T, randomised=1)]
    ln = len(rle1_decode(T))
    s = write_stream(one)[0]
    for D in (ln, ln - 1, ln + 1, 2 * ln):
        out.append(Case(f"garbage-D{D}", one, D, suffix=bytes(range(1, 40))))
        out.append(Case(f"garbage-magic-D{D}", one, D, suffix=BLOCK_MAGIC.to_bytes(6, "big") + bytes(20)))
        out.append(Case(f"twice-D{D}", one, D, suffix=s))
    return out


def host_matrix() -> List[Case]:
    return (ladder_content_cases() + ladder_raw_cases() + tail4_cases() + walk_tail4_cases() + knob_cases() + zero_run_cases()
            + stream_shape_cases())


def gpu_batches() -> dict:
    """The matrix as batches that share one D: name -> (cases, D), each case
    to be decoded as case.at(D)."""
    big = f"-n{LADDER_NBLOCK[-1]}-"
    groups = {"content": [c for c in ladder_content_cases() if big not in c.name],
              "content_big": [c for c in ladder_content_cases() if big in c.name],
              "tail4": tail4_cases() + walk_tail4_cases(),
              "stage_a": knob_cases() + zero_run_cases(), "shapes": stream_shape_cases(),
              "sampling": sampling_cases()}
    for kind in ALPHABETS:
        groups["raw-" + kind] = [c for c in ladder_raw_cases() if f"-{kind}-" in c.name and big not in c.name]
        groups["raw_big-" + kind] = [c for c in ladder_raw_cases() if f"-{kind}-" in c.name and big in c.name]
    return {k: (v, max(c.D for c in v) + 3) for k, v in groups.items()}


SAMPLING_NBLOCK = (1023, 1024, 1025, 2047, 2048, 2049, 131073)


@functools.lru_cache(maxsize=None)
def sampling_cases() -> List[Case]:
    """Valid blocks around the sizes where the sample stride doubles, and
    one of 131 073 bytes (stride 256: the kept bytes per walk are capped by
    the array's level at level 1 and by the stride at level 9)."""
    out = []
    for i, n in enumerate(SAMPLING_NBLOCK):
        for rnd in ((0, 1) if n in (1024, 131073) else (i & 1,)):
            T = alphabet_T(("all256", "five_doubled")[i & 1], n, seed=50 + i)
            out.append(Case(f"sampling-n{n}-r{rnd}", [Block(T=T, randomised=rnd, ngroups=3)],
                            len(rle1_decode(T)), level=9))
    return out


@functools.lru_cache(maxsize=None)
def many_blocks(count: int = 40, seed: int = 3, big_at: int = -1) -> Tuple[Block, ...]:
    """`count` blocks of 64..3 000 bytes, alternately randomised, of even
    total content length; block `big_at` is 3 000 bytes longer."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(64, 3001, count).tolist()
    out = []
    for i, n in enumerate(sizes):
        T = alphabet_T(ALPHABETS[i % 4], n + (3000 if i == big_at else 0), seed=seed * 100 + i)
        out.append(Block(T=T, randomised=i & 1, ngroups=2 + i % 5))
    if sum(len(rle1_decode(b.T)) for b in out) & 1:
        out[-1] = Block(T=out[-1].T + b"\xee", randomised=out[-1].randomised)
    return tuple(out)


def content_len(blocks: Sequence[Block]) -> int:
    return sum(len(rle1_decode(b.T)) for b in blocks)


@functools.lru_cache(maxsize=None)
def fallback_streams() -> Tuple[List[bytes], int, int]:
    """(streams, D, blocks): a stream of 40 small blocks and its variants: a
    wrong CRC in block 21, a cut inside block 26, and block 36 grown so that
    D ends inside a late block."""
    blocks = list(many_blocks())
    D = content_len(blocks)
    s, exp, offs = write_stream_info(blocks)
    assert len(exp) == D
    bad = list(blocks)
    bad[20] = Block(T=blocks[20].T, randomised=blocks[20].randomised, crc_xor=1 << 17)
    grown = list(many_blocks(big_at=35))
    assert content_len(grown) > D + 1000
    return [s, write_stream(bad)[0], s[:offs[25] // 8 + 40], write_stream(grown)[0]], D, len(blocks)


@functools.lru_cache(maxsize=None)
def randomised_streams() -> Tuple[List[bytes], int]:
    """(streams, D): plain and randomised blocks mixed, one randomised block
    of 70 000 bytes (some 140 schedule entries, sample stride 128); D falls
    at the end of the last block, before the last block, and inside it."""
    p0 = Block(T=alphabet_T("all256", 3000, 1))
    big = Block(T=alphabet_T("five_doubled", 70000, 2), randomised=1, ngroups=6)
    p1 = Block(T=alphabet_T("three_runs6", 500, 3))
    r1 = Block(T=alphabet_T("two", 1025, 4), randomised=1)
    base = [p0, big, p1, r1]
    D = content_len(base)
    after = Block(T=alphabet_T("all256", 300, 5), randomised=1)
    after_bad = Block(T=after.T, randomised=1, crc_xor=0x80)
    longer = Block(T=alphabet_T("five_doubled", 5000, 6), randomised=1)
    huge = Block(T=alphabet_T("five_doubled", 99000, 7), randomised=1, ngroups=4)
    streams = [write_stream(b, level=1)[0] for b in
               (base, base + [after], base + [after_bad], [p0, big, p1, longer], [p1, huge], [big, p0, r1, p1, after])]
    assert content_len([p1, huge]) > D and content_len([p0, big, p1, longer]) > D
    return streams, D
