"""gzip / deflate streams for the GPU inflate tests: builders over the system
zlib, and a small reader that gives a stream's structure back (code lengths,
token positions), so that a case can check that it has the property it is
there for."""
import struct
import zlib

import numpy as np

# ---- builders -------------------------------------------------------------------------------------
PLAIN_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255])


def trailer(payload):
    return struct.pack("<II", zlib.crc32(payload), len(payload) & 0xFFFFFFFF)


def member(raw, payload, header=PLAIN_HEADER):
    return header + raw + trailer(payload)


def gzip_wrap(raw_deflate: bytes, payload: bytes, flags=0, extra=b"", name=b"", comment=b"",
              hcrc=False):
    """A member with the header fields of `flags` (PLAIN_HEADER by default)."""
    h = bytearray([0x1f, 0x8b, 8, flags | (2 if hcrc else 0), 0, 0, 0, 0, 0, 255])
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    return member(raw_deflate, payload, bytes(h))


def stored(data, last=False):
    """One stored block (byte aligned: the header's 3 bits and 5 bits of padding)."""
    return bytes([1 if last else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, wbits=-15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(payload) + c.flush()


def flip(b, i, bit=1):
    return b[:i] + bytes([b[i] ^ bit]) + b[i + 1:]


def text(n, seed, spare=0):
    """n bytes of n // 4 + spare words drawn from 300 (the draw count is part
    of the stream: the same seed gives other bytes with another `spare`)."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 10))).astype(np.uint8)) for _ in range(300)]
    p = 1.0 / (np.arange(300) + 1.0)
    out = b" ".join(words[i] for i in rng.choice(300, size=n // 4 + spare, p=p / p.sum()))
    assert len(out) >= n
    return out[:n]


def noise(n, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n).astype(np.uint8).tobytes()


def _skewed_with_copies():
    """128 KiB, p(i) ~ 1 / (i + 1)^1.3, ~2 000 copies of 3-40 bytes from up to 32 K back."""
    rng = np.random.default_rng(1307)
    p = 1.0 / (np.arange(256) + 1.0) ** 1.3
    a = rng.choice(256, size=128 << 10, p=p / p.sum()).astype(np.uint8)
    for _ in range(2000):
        n = int(rng.integers(3, 41))
        at = int(rng.integers(64, a.size - n))
        d = int(rng.integers(1, min(at, 32768) + 1))
        for k in range(n):  # (byte by byte: a copy may overlap itself, as in LZ77)
            a[at + k] = a[at + k - d]
    return a.tobytes()


def _three_symbols():
    rng = np.random.default_rng(2207)
    return rng.choice(np.array([0, 7, 255], np.uint8), size=64 << 10, p=[0.9, 0.08, 0.02]).tobytes()


# ---- a small deflate reader -------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    """A raw deflate stream as a list of bits (64 zero bits behind it) and a read position p."""

    def __init__(self, raw):
        self.b = np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little").tolist() + [0] * 64
        self.p = 0

    def bits(self, n):
        x = 0
        for i in range(n):
            x |= self.b[self.p + i] << i
        self.p += n
        return x


def canon(lens):
    """{(length, code): symbol} of the canonical Huffman code with these lengths."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def sym(br, table):
    """The symbol whose code stands at br.p, br moved behind it; None, br not
    moved, for a bit pattern that is no code."""
    c = 0
    for l in range(1, 16):
        c = (c << 1) | br.b[br.p + l - 1]
        if (l, c) in table:
            br.p += l
            return table[(l, c)]
    return None


def block_header(br):
    """The fixed or dynamic block header at br.p: (last, literal/length code
    lengths, distance code lengths); br is left at the first body bit."""
    last, ty = br.bits(1), br.bits(2)
    assert ty in (1, 2), ty
    if ty == 1:
        return last, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
    hl, hd, hc = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    cl = [0] * 19
    for i in range(hc):
        cl[CLEN_ORDER[i]] = br.bits(3)
    ct, ls = canon(cl), []
    while len(ls) < hl + hd:
        s = sym(br, ct)
        if s < 16:
            ls.append(s)
        else:
            n = br.bits((2, 3, 7)[s - 16])
            ls += [ls[-1]] * (3 + n) if s == 16 else [0] * ((3, 11)[s - 17] + n)
    return last, ls[:hl], ls[hl:]
