"""Block-level bzip2 writer.  TEST INFRASTRUCTURE ONLY.

libbz2's encoder never sets the randomised bit, never leaves a run of four
without its count byte, always writes an L / origPtr pair that is one cycle
and always fills its blocks.  The decoder accepts all of that and more, so
the tests need streams libbz2 cannot write.  This module writes bzip2
streams block by block, from the format alone (pure Python + numpy):

  stream  = "BZh" level | block* | end-of-stream record (combined CRC)
  block   = magic | CRC | randomised | origPtr | symbol map | selectors |
            code lengths | Huffman(RUNA/RUNB + MTF(L)) | EOB

A block is given in one of two forms:

  content form  Block(T=..., randomised=0/1): T is the block after RLE1
                (any byte string is a valid RLE1 encoding unless it ends
                right after four equal bytes: such a block is a `tail4`
                block, the decoder reads its count byte from the cycle
                start and then reports the stream corrupt).  The writer
                XORs the randomisation schedule into T, computes the BWT,
                origPtr and the CRC of the RLE1-decoded content.
  raw form      Block(L=..., orig=..., crc=...): written as given, for
                L / origPtr pairs that are not one cycle and for origPtr
                out of range.

Per-block knobs: ngroups (2..6 valid, anything 0..7 is written), the code
lengths (an int: every symbol gets that length, the canonical code of
symbol i is then i; or "huffman": real lengths from the symbol counts of
the groups that use a table), the order in which the tables are used
(`order`, cycled over the groups of 50 symbols), and surplus selectors.
The format fixes 50 symbols per selector; only a block's last selector
covers fewer (1..50), which follows from the content: `symbol_count`
reports a block's symbols and tests/bz2_cases.py finds blocks with a given
number of them.
"""
import functools
import heapq
import os
import re
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

_RNUMS_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zarr_amd", "csrc", "zcg_bz2_rnums.h")
G_SIZE = 50
BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090


@functools.lru_cache(maxsize=None)
def rnums() -> Tuple[int, ...]:
    """The 512-entry randomisation schedule (a format constant)."""
    body = open(_RNUMS_H).read().split("{")[-1].split("}")[0]
    t = tuple(int(x) for x in re.findall(r"\d+", body))
    assert len(t) == 512
    return t


def rand_positions(n: int) -> np.ndarray:
    """Chain positions < n whose byte is XORed with 1: F_m - 2, F_m the
    prefix sums of the schedule (used cyclically)."""
    r = np.array(rnums(), np.int64)
    reps = n // int(r.sum()) + 2
    f = np.cumsum(np.tile(r, reps)) - 2
    return f[f < n]


def rand_mask_at(pos: int) -> int:
    """The mask of chain position `pos` alone."""
    p = rand_positions(pos + 1)
    return int(len(p) > 0 and p[-1] == pos)


def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ (0x04C11DB7 if c & 0x80000000 else 0)) & 0xFFFFFFFF
        t.append(c)
    return t


_CRC_T = _crc_table()


def crc32_msb_bytewise(data: bytes) -> int:
    """bzip2's CRC-32: MSB-first, polynomial 0x04C11DB7, init and xorout ~0."""
    c = 0xFFFFFFFF
    t = _CRC_T
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ t[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


_BITREV8 = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)], np.uint8)


def crc32_msb(data: bytes) -> int:
    """The same CRC, quickly: it is zlib's (the reflected form of the same
    polynomial) over the bit-reversed bytes, bit-reversed."""
    c = zlib.crc32(_BITREV8[np.frombuffer(data, np.uint8)].tobytes())
    return int(f"{c:032b}"[::-1], 2)


def crc_combine(comb: int, crc: int) -> int:
    """The stream CRC: rotate left by one, XOR the block CRC in."""
    return (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ crc


def rle1_encode(content: bytes, open_tail: bool = False) -> bytes:
    """RLE1: runs of 4..255 equal bytes become four bytes and a count.  With
    open_tail the content must end in a run of >= 4 and that run's count
    byte is left out (a `tail4` block)."""
    a = np.frombuffer(content, np.uint8)
    out = bytearray()
    if len(a):
        starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
        lens = np.diff(np.r_[starts, len(a)])
        for s, ln in zip(starts.tolist(), lens.tolist()):
            b = bytes([int(a[s])])
            while ln > 0:
                k = min(ln, 255)
                out += b * 4 + bytes([k - 4]) if k >= 4 else b * k
                ln -= k
    if open_tail:
        assert rle1_state(bytes(out[:-1])) == 4, "content does not end in a run of four or more"
        del out[-1]
    return bytes(out)


def rle1_state(T: bytes) -> int:
    """The run machine's state after T: 0 at the start, 1..3 equal bytes
    seen, 4 = four seen and the count byte is due."""
    st, pc = 0, -1
    for c in T:
        st = 0 if st == 4 else (st + 1 if (st and c == pc) else 1)
        pc = c
    return st


def rle1_decode(T: bytes) -> bytes:
    """The content of a block T; a final run of four without its count
    stands as four bytes."""
    out = bytearray()
    st, pc = 0, -1
    for c in T:
        if st == 4:
            out += bytes([pc]) * c
            st = 0
        else:
            out.append(c)
            st = st + 1 if (st and c == pc) else 1
        pc = c
    return bytes(out)


def bwt(t: bytes) -> Tuple[bytes, int]:
    """(L, origPtr) of the cyclic rotations of t, by prefix doubling."""
    a = np.frombuffer(t, np.uint8)
    n = len(a)
    assert n > 0
    rank = a.astype(np.int64)
    idx = np.arange(n)
    k = 1
    while True:
        m = int(rank.max()) + 1
        u, rank = np.unique(rank * m + rank[(idx + k) % n], return_inverse=True)
        rank = rank.reshape(-1)
        if len(u) == n or 2 * k >= n:
            break
        k *= 2
    sa = np.argsort(rank, kind="stable")
    return a[(sa - 1) % n].tobytes(), int(np.flatnonzero(sa == 0)[0])


def rotation_ranks(t: bytes) -> List[Tuple[int, np.ndarray]]:
    """[(k, rank)] for k = 1, 2, 4, ...: rank[i] orders rotation i by its
    first k bytes (cyclic), equal prefixes share a rank.  The list ends once
    all ranks differ or k >= len(t): the last entry is the order of the
    whole rotations, equal rotations still sharing a rank."""
    a = np.frombuffer(t, np.uint8)
    n = len(a)
    assert n > 0
    idx = np.arange(n)
    rank = np.unique(a, return_inverse=True)[1].reshape(-1).astype(np.int64)
    k = 1
    out = [(1, rank)]
    while int(rank.max()) + 1 < n and k < n:
        m = int(rank.max()) + 1
        rank = np.unique(rank * m + rank[(idx + k) % n], return_inverse=True)[1].reshape(-1).astype(np.int64)
        k *= 2
        out.append((k, rank))
    return out


def prefix_group_sizes(t: bytes, dpre: int) -> np.ndarray:
    """Sizes of the groups of rotations of t that share their first dpre
    bytes (cyclic), in sorted order of the prefix."""
    a = np.frombuffer(t, np.uint8).astype(np.int64)
    idx = np.arange(len(a))
    key = np.zeros(len(a), np.int64)
    for d in range(dpre):
        key = key * 256 + a[(idx + d) % len(a)]
    return np.unique(key, return_counts=True)[1]


def adjacent_lcp(t: bytes, cap: Optional[int] = None, levels=None) -> np.ndarray:
    """Common prefix length (cyclic, at most len(t) or cap) of each pair of
    neighbours among the sorted rotations of t: len(t) - 1 values.  `levels`
    is rotation_ranks(t), for a caller that has it."""
    n = len(t)
    levels = rotation_ranks(t) if levels is None else levels
    sa = np.argsort(levels[-1][1], kind="stable")
    x, y = sa[:-1], sa[1:]
    lcp = np.zeros(n - 1, np.int64)
    for k, rank in reversed(levels):
        lcp += k * (rank[(x + lcp) % n] == rank[(y + lcp) % n])
    return np.minimum(lcp, n if cap is None else min(n, cap))


def orig_range(t: bytes) -> Tuple[int, int]:
    """(first, count): the positions, among the sorted rotations of t, of
    the rotations equal to t itself; count is 1 unless t is periodic."""
    rank = rotation_ranks(t)[-1][1]
    return int((rank < rank[0]).sum()), int((rank == rank[0]).sum())


def is_one_cycle(L: bytes, orig: int) -> bool:
    """Whether the inverse-BWT links of L form a single cycle (what a real
    BWT of an aperiodic block gives)."""
    link = np.argsort(np.frombuffer(L, np.uint8), kind="stable").tolist()
    p, k = link[orig], 1
    while p != orig and k <= len(L):
        p = link[p]
        k += 1
    return p == orig and k == len(L)


def chain_bytes(L: bytes, orig: int, count: int) -> bytes:
    """The first `count` bytes a decoder's walk from origPtr fetches (before
    the schedule's masks); past its cycle's length the walk goes round again."""
    link = np.argsort(np.frombuffer(L, np.uint8), kind="stable").tolist()
    p = link[orig]
    out = bytearray()
    for _ in range(count):
        out.append(L[p])
        p = link[p]
    return bytes(out)


_RESOLVED = {}  # (T, randomised) -> (L, origPtr, CRC, content)


@dataclass
class Block:
    T: Optional[bytes] = None          # content form
    randomised: int = 0
    L: Optional[bytes] = None          # raw form
    orig: int = 0
    crc: int = 0
    ngroups: int = 2
    lengths: Union[int, str] = "huffman"
    order: Optional[Sequence[int]] = None   # table of group g = order[g % len(order)]
    extra_selectors: int = 0
    crc_xor: int = 0                   # content form: XORed into the stored CRC
    used_extra: Sequence[int] = field(default_factory=tuple)  # bytes marked used beyond those of L
    plain: bool = False                # T has no run of four: the content is T

    def resolved(self):
        """(L, origPtr, stored CRC, content or None)."""
        if self.L is not None:
            return self.L, self.orig, self.crc, None
        key = (self.T, self.randomised)
        if key not in _RESOLVED:
            content = self.T if self.plain else rle1_decode(self.T)
            t = np.frombuffer(self.T, np.uint8).copy()
            if self.randomised:
                t[rand_positions(len(t))] ^= 1
            _RESOLVED[key] = bwt(t.tobytes()) + (crc32_msb(content), content)
        L, orig, crc, content = _RESOLVED[key]
        return L, orig, crc ^ self.crc_xor, content

    def is_tail4(self):
        return self.T is not None and rle1_state(self.T) == 4


def mtf_rle2_serial(L: bytes, used: Sequence[int]) -> List[int]:
    """Move-to-front over the used bytes, zero runs as RUNA/RUNB (bijective
    base 2, least significant digit first), then EOB: the definition."""
    mtf = list(used)
    out = []
    zrun = 0
    for b in L:
        if mtf[0] == b:
            zrun += 1
            continue
        while zrun > 0:
            out.append(0 if zrun & 1 else 1)
            zrun = (zrun - 1) >> 1
        j = mtf.index(b)
        out.append(j + 1)
        del mtf[j]
        mtf.insert(0, b)
    while zrun > 0:
        out.append(0 if zrun & 1 else 1)
        zrun = (zrun - 1) >> 1
    out.append(len(used) + 1)
    return out


def mtf_rle2(L: bytes, used: Sequence[int]) -> np.ndarray:
    """The same symbols, vectorised.  A byte's MTF index is the number of
    other bytes seen since its own last occurrence (the initial list counts
    as occurrences before the block); the digits of a zero run of z are the
    bits of z + 1 below its leading one, lowest first."""
    a = np.frombuffer(L, np.uint8)
    n = len(a)
    idx = np.arange(n, dtype=np.int32)

    def last_before(j, c):  # last occurrence of byte c strictly before each position
        inc = np.maximum.accumulate(np.where(a == c, idx, np.int32(-1 - j)))
        return np.concatenate(([np.int32(-1 - j)], inc[:-1]))

    prev = np.zeros(n, np.int32)
    for j, c in enumerate(used):
        m = a == c
        if m.any():
            prev[m] = last_before(j, c)[m]
    r = np.zeros(n, np.int64)
    for j, c in enumerate(used):
        r += last_before(j, c) > prev
    z = np.concatenate(([0], (r == 0).astype(np.int8), [0]))
    d = np.diff(z)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    zl = (ends - starts).astype(np.int64)
    nd = np.frexp(zl + 1)[1].astype(np.int64) - 1
    cnt = (r != 0).astype(np.int64)
    cnt[starts] = nd
    offs = np.cumsum(cnt) - cnt
    out = np.empty(int(cnt.sum()) + 1, np.int64)
    nz = r != 0
    out[offs[nz]] = r[nz] + 1
    jj = np.arange(int(nd.sum())) - np.repeat(np.cumsum(nd) - nd, nd)
    out[np.repeat(offs[starts], nd) + jj] = (np.repeat(zl + 1, nd) >> jj) & 1
    out[-1] = len(used) + 1
    return out


def symbol_count(L: bytes) -> int:
    """Number of Huffman symbols of a block with last column L (EOB included)."""
    return len(mtf_rle2(L, sorted(set(L))))


def huffman_lengths(counts: Sequence[int], limit: int = 20) -> List[int]:
    """Code lengths of a Huffman tree over counts (every symbol gets a code);
    the weights are flattened until no length exceeds the limit."""
    w = [max(1, int(c)) for c in counts]
    while True:
        heap = [(x, i, (i,)) for i, x in enumerate(w)]
        heapq.heapify(heap)
        lens = [0] * len(w)
        tie = len(w)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for i in a[2] + b[2]:
                lens[i] += 1
            heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
            tie += 1
        if max(lens) <= limit:
            return lens
        w = [x // 2 + 1 for x in w]


def canonical_codes(lens: Sequence[int]) -> List[int]:
    """Codes in the order the format assigns them: by length, then by symbol."""
    codes = [0] * len(lens)
    vec = 0
    for n in range(min(lens), max(lens) + 1):
        for i, l in enumerate(lens):
            if l == n:
                codes[i] = vec
                vec += 1
        vec <<= 1
    return codes


class BitWriter:
    def __init__(self):
        self.parts = []
        self.cur = []

    def put(self, v: int, n: int):
        self.cur.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def put_bits(self, bits: np.ndarray):
        self._flush()
        self.parts.append(bits.astype(np.uint8))

    def _flush(self):
        if self.cur:
            self.parts.append(np.array(self.cur, np.uint8))
            self.cur = []

    def nbits(self) -> int:
        self._flush()
        return int(sum(len(p) for p in self.parts))

    def tobytes(self) -> bytes:
        self._flush()
        bits = np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8)
        return np.packbits(bits).tobytes()  # zero-padded to a byte


_BLOCK_BITS = {}  # a block's bits do not depend on where it stands


def write_block(w: BitWriter, blk: Block) -> Tuple[int, Optional[bytes]]:
    """Append one block; returns (the stored CRC, its content or None)."""
    L, orig, crc, content = blk.resolved()
    key = (L, orig, crc, blk.randomised, blk.ngroups, blk.lengths, tuple(blk.order or ()), blk.extra_selectors,
           tuple(blk.used_extra))
    if key not in _BLOCK_BITS:
        bw = BitWriter()
        _write_block(bw, blk, L, orig, crc)
        _BLOCK_BITS[key] = np.concatenate(bw.parts) if bw.nbits() else np.zeros(0, np.uint8)
    w.put_bits(_BLOCK_BITS[key])
    return crc, content


def _write_block(w: BitWriter, blk: Block, L: bytes, orig: int, crc: int):
    w.put(BLOCK_MAGIC, 48)
    w.put(crc, 32)
    w.put(blk.randomised, 1)
    w.put(orig, 24)
    used = sorted(set(L) | set(blk.used_extra))
    rows = [0] * 16
    for b in used:
        rows[b >> 4] |= 0x8000 >> (b & 15)
    w.put(sum((0x8000 >> i) for i in range(16) if rows[i]), 16)
    for r in rows:
        if r:
            w.put(r, 16)
    syms = mtf_rle2(L, used)
    alpha = len(used) + 2
    ng = blk.ngroups
    ntab = max(ng, 1)
    order = list(blk.order) if blk.order is not None else list(range(ntab))
    assert all(0 <= t < ntab for t in order)
    need = (len(syms) + G_SIZE - 1) // G_SIZE
    nsel = need + blk.extra_selectors
    assert 1 <= nsel < 32768
    sel = np.array([order[g % len(order)] for g in range(nsel)], np.int64)
    w.put(ng, 3)
    w.put(nsel, 15)
    pos = list(range(max(ntab, 6)))
    for t in sel.tolist():
        j = pos.index(t)
        w.put(((1 << j) - 1) << 1, j + 1)  # j ones and a zero
        del pos[j]
        pos.insert(0, t)
    tsel = sel[np.arange(len(syms)) // G_SIZE]
    lens2 = np.zeros((ntab, alpha), np.int64)
    codes2 = np.zeros((ntab, alpha), np.int64)
    for t in range(ntab):
        if blk.lengths == "huffman":
            lens = huffman_lengths(np.bincount(syms[tsel == t], minlength=alpha))
        else:
            assert alpha <= (1 << int(blk.lengths)) and 1 <= int(blk.lengths) <= 20
            lens = [int(blk.lengths)] * alpha
        lens2[t] = lens
        codes2[t] = canonical_codes(lens)
        cur = lens[0]
        w.put(cur, 5)
        for l in lens:
            while cur < l:
                w.put(2, 2)
                cur += 1
            while cur > l:
                w.put(3, 2)
                cur -= 1
            w.put(0, 1)
    ln = lens2[tsel, syms]
    cd = codes2[tsel, syms]
    j = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    w.put_bits((np.repeat(cd, ln) >> (np.repeat(ln, ln) - 1 - j)) & 1)


def write_stream_info(blocks: Sequence[Block], level: int = 1):
    """(stream, content or None, bit offset of each block and of the end
    record).  The content is None when a block is in raw form."""
    w = BitWriter()
    for c in b"BZh" + bytes([0x30 + level]):
        w.put(c, 8)
    comb = 0
    parts = []
    offs = []
    for blk in blocks:
        offs.append(w.nbits())
        crc, content = write_block(w, blk)
        comb = crc_combine(comb, crc)
        parts.append(content)
    offs.append(w.nbits())
    w.put(END_MAGIC, 48)
    w.put(comb, 32)
    expected = None if any(p is None for p in parts) else b"".join(parts)
    return w.tobytes(), expected, offs


def write_stream(blocks: Sequence[Block], level: int = 1) -> Tuple[bytes, Optional[bytes]]:
    """(stream_bytes, expected_content); no blocks gives the empty stream."""
    s, expected, _ = write_stream_info(blocks, level)
    return s, expected


def count_blocks(stream: bytes) -> int:
    """Blocks of a stream: occurrences of the block magic at any bit offset."""
    a = np.frombuffer(stream + b"\0", np.uint8).astype(np.uint16)
    magic = BLOCK_MAGIC.to_bytes(6, "big")
    n = 0
    for s in range(8):
        b = (((a[:-1] << s) | (a[1:] >> (8 - s))) & 0xFF).astype(np.uint8).tobytes()
        n += b.count(magic)
    return n


def decode_rounds(D: int, level: int) -> int:
    """Blocks the decoder's per-block rounds cover for a chunk of D bytes at
    the array's block-size level (launch_bzip2_decode); any further block is
    decoded by the whole-stream kernel."""
    return -(-D // (80000 * level)) + 2
