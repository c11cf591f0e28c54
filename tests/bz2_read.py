"""Block-level bzip2 reader.  TEST INFRASTRUCTURE ONLY.

The counterpart of tests/bz2_craft.py: it takes a bzip2 stream apart, from the
format alone (pure Python + numpy), and keeps every field a decoder throws
away, so that a test can say which stage of an encoder went wrong:

  stream  = "BZh" level | block* | end-of-stream record (combined CRC) | pad
  block   = magic | CRC | randomised | origPtr | symbol map | selectors |
            code lengths | Huffman(RUNA/RUNB + MTF(L)) | EOB

read_stream returns, per block, the header fields, the selectors after their
MTF decode, the code length tables, the symbol list, the last column L, the
block text T (the inverse BWT from origPtr, the randomisation schedule
undone) and its content rle1_decode(T).  It checks no CRC: the caller compares
the stored values with bz2_craft.crc32_msb of the contents.  write_back
writes the parsed fields out again; a stream read correctly comes back bit
for bit.
"""
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from bz2_craft import (BLOCK_MAGIC, END_MAGIC, G_SIZE, BitWriter, canonical_codes, chain_bytes, rand_positions,
                       rle1_decode)

RUNA, RUNB = 0, 1
_WIN = 20  # the longest code a decoder accepts


class FormatError(ValueError):
    pass


@dataclass
class BlockInfo:
    bit_off: int            # of the block magic
    crc: int                # stored
    randomised: int
    orig: int
    used: List[int]         # byte values of the symbol map, ascending
    ngroups: int
    nselectors: int
    selectors: List[int]    # after the MTF decode, all nselectors of them
    lengths: List[List[int]]  # ngroups tables of len(used) + 2 lengths
    symbols: List[int]      # RUNA / RUNB / MTF index + 1 / EOB (= len(used) + 1, last)
    L: bytes
    T: bytes
    content: bytes
    end_bit: int            # first bit behind the block's EOB code


class _Bits:
    def __init__(self, data: bytes):
        self.a = np.unpackbits(np.frombuffer(data, np.uint8))
        self.n = len(self.a)
        self.b = self.a.tolist()
        self._win = None

    def get(self, pos: int, n: int) -> int:
        if pos + n > self.n:
            raise FormatError("stream ends inside a field")
        v = 0
        for x in self.b[pos:pos + n]:
            v = (v << 1) | x
        return v

    def windows(self) -> list:
        """The _WIN bits from every position on (zeros behind the end)."""
        if self._win is None:
            p = np.concatenate((self.a, np.zeros(_WIN, np.uint8))).astype(np.int32)
            w = np.zeros(self.n, np.int32)
            for k in range(_WIN):
                w |= p[k:k + self.n] << (_WIN - 1 - k)
            self._win = w.tolist()
        return self._win


def _decode_tables(lengths: List[List[int]]) -> Tuple[int, list, list]:
    """(W, symbol per W-bit window, code length per window) for each table;
    a window no code starts gets length 0."""
    W = max(max(t) for t in lengths)
    syms, lens = [], []
    for t in lengths:
        s = np.full(1 << W, -1, np.int32)
        ln = np.zeros(1 << W, np.int32)
        for v, (code, l) in enumerate(zip(canonical_codes(t), t)):
            if code >> l:
                raise FormatError("code lengths oversubscribed")
            s[code << (W - l):(code + 1) << (W - l)] = v
            ln[code << (W - l):(code + 1) << (W - l)] = l
        syms.append(s.tolist())
        lens.append(ln.tolist())
    return W, syms, lens


def _read_block(bits: _Bits, pos: int) -> BlockInfo:
    start = pos
    pos += 48
    crc = bits.get(pos, 32)
    randomised = bits.get(pos + 32, 1)
    orig = bits.get(pos + 33, 24)
    pos += 57
    rows = bits.get(pos, 16)
    pos += 16
    used = []
    for i in range(16):
        if rows & (0x8000 >> i):
            r = bits.get(pos, 16)
            pos += 16
            used += [16 * i + j for j in range(16) if r & (0x8000 >> j)]
    if not used:
        raise FormatError("empty symbol map")
    alpha = len(used) + 2
    ngroups = bits.get(pos, 3)
    nsel = bits.get(pos + 3, 15)
    pos += 18
    if not 2 <= ngroups <= 6 or nsel < 1:
        raise FormatError(f"nGroups {ngroups}, nSelectors {nsel}")
    order = list(range(ngroups))
    selectors = []
    b = bits.b
    for _ in range(nsel):
        j = 0
        while bits.get(pos, 1):
            pos += 1
            j += 1
            if j >= ngroups:
                raise FormatError("selector past nGroups")
        pos += 1
        t = order.pop(j)
        order.insert(0, t)
        selectors.append(t)
    lengths = []
    for _ in range(ngroups):
        cur = bits.get(pos, 5)
        pos += 5
        tab = []
        for _ in range(alpha):
            while True:
                if not 1 <= cur <= _WIN:
                    raise FormatError(f"code length {cur}")
                if pos >= bits.n:
                    raise FormatError("stream ends inside the code lengths")
                if not b[pos]:
                    pos += 1
                    break
                cur += -1 if b[pos + 1] else 1
                pos += 2
            tab.append(cur)
        lengths.append(tab)
    W, tsym, tlen = _decode_tables(lengths)
    sh = _WIN - W
    win = bits.windows()
    eob = alpha - 1
    symbols = []
    g = 0
    done = False
    while not done:
        if g >= nsel:
            raise FormatError("symbols past the last selector")
        ts, tl = tsym[selectors[g]], tlen[selectors[g]]
        g += 1
        for _ in range(G_SIZE):
            if pos >= bits.n:
                raise FormatError("stream ends inside the symbols")
            w = win[pos] >> sh
            s = ts[w]
            if s < 0:
                raise FormatError("no code starts here")
            pos += tl[w]
            symbols.append(s)
            if s == eob:
                done = True
                break
    if pos > bits.n:
        raise FormatError("stream ends inside the symbols")
    # undo RUNA/RUNB and the move-to-front
    mtf = list(used)
    L = bytearray()
    run, weight = 0, 1
    for s in symbols:
        if s <= RUNB:
            run += weight << s
            weight <<= 1
            continue
        if run:
            L += bytes([mtf[0]]) * run
            run, weight = 0, 1
        if s == eob:
            break
        c = mtf.pop(s - 1)
        mtf.insert(0, c)
        L.append(c)
    L = bytes(L)
    if not L or orig >= len(L):
        raise FormatError(f"origPtr {orig} of {len(L)}")
    t = np.frombuffer(chain_bytes(L, orig, len(L)), np.uint8).copy()
    if randomised:
        t[rand_positions(len(t))] ^= 1
    T = t.tobytes()
    return BlockInfo(start, crc, randomised, orig, used, ngroups, nsel, selectors, lengths, symbols, L, T,
                     rle1_decode(T), pos)


def read_stream(stream: bytes) -> Tuple[int, List[BlockInfo], int, int]:
    """(level, blocks, stored combined CRC, zero pad bits behind the end
    record).  Raises FormatError for anything that is not one whole stream
    followed by zero bits alone."""
    if len(stream) < 14 or stream[:3] != b"BZh" or not 0x31 <= stream[3] <= 0x39:
        raise FormatError("no stream header")
    bits = _Bits(stream)
    pos = 32
    blocks = []
    while True:
        magic = bits.get(pos, 48)
        if magic == END_MAGIC:
            comb = bits.get(pos + 48, 32)
            pos += 80
            break
        if magic != BLOCK_MAGIC:
            raise FormatError(f"no block at bit {pos}")
        blocks.append(_read_block(bits, pos))
        pos = blocks[-1].end_bit
    if any(bits.b[pos:]):
        raise FormatError("bits set behind the end record")
    return stream[3] - 0x30, blocks, comb, bits.n - pos


def write_back(level: int, blocks: List[BlockInfo], comb: int) -> bytes:
    """The stream of the parsed fields: symbol map, selectors, lengths and
    symbols written again with the format's canonical codes."""
    w = BitWriter()
    for c in b"BZh" + bytes([0x30 + level]):
        w.put(c, 8)
    for blk in blocks:
        w.put(BLOCK_MAGIC, 48)
        w.put(blk.crc, 32)
        w.put(blk.randomised, 1)
        w.put(blk.orig, 24)
        rows = [0] * 16
        for c in blk.used:
            rows[c >> 4] |= 0x8000 >> (c & 15)
        w.put(sum((0x8000 >> i) for i in range(16) if rows[i]), 16)
        for r in rows:
            if r:
                w.put(r, 16)
        w.put(blk.ngroups, 3)
        w.put(blk.nselectors, 15)
        order = list(range(blk.ngroups))
        for t in blk.selectors:
            j = order.index(t)
            w.put(((1 << j) - 1) << 1, j + 1)
            order.pop(j)
            order.insert(0, t)
        for tab in blk.lengths:
            cur = tab[0]
            w.put(cur, 5)
            for l in tab:
                while cur < l:
                    w.put(2, 2)
                    cur += 1
                while cur > l:
                    w.put(3, 2)
                    cur -= 1
                w.put(0, 1)
        syms = np.array(blk.symbols, np.int64)
        tsel = np.array(blk.selectors, np.int64)[np.arange(len(syms)) // G_SIZE]
        ln = np.array(blk.lengths, np.int64)[tsel, syms]
        cd = np.array([canonical_codes(tab) for tab in blk.lengths], np.int64)[tsel, syms]
        j = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        w.put_bits((np.repeat(cd, ln) >> (np.repeat(ln, ln) - 1 - j)) & 1)
    w.put(END_MAGIC, 48)
    w.put(comb, 32)
    return w.tobytes()
