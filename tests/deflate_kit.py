"""gzip / deflate streams for the GPU inflate tests: builders over the system
zlib, and a small reader that gives a stream's structure back (code lengths,
token positions), so that a case can check that it has the property it is
there for; the gzip encoder's tests read zlib's streams and the GPU's with it."""
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


def code_lengths(br):
    """The code lengths of a dynamic block's header at br.p (behind the 3
    type bits): (literal/length lengths, distance lengths, [(symbol, run)] of
    the code-length alphabet as sent: run is 1 for a plain length, the repeat
    count for 16 / 17 / 18)."""
    hl, hd, hc = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    cl = [0] * 19
    for i in range(hc):
        cl[CLEN_ORDER[i]] = br.bits(3)
    ct, ls, sent = canon(cl), [], []
    while len(ls) < hl + hd:
        s = sym(br, ct)
        if s < 16:
            ls.append(s)
            sent.append((s, 1))
        else:
            n = br.bits((2, 3, 7)[s - 16]) + (3, 3, 11)[s - 16]
            ls += [ls[-1]] * n if s == 16 else [0] * n
            sent.append((s, n))
    return ls[:hl], ls[hl:], sent


def block_header(br):
    """The fixed or dynamic block header at br.p: (last, literal/length code
    lengths, distance code lengths); br is left at the first body bit."""
    last, ty = br.bits(1), br.bits(2)
    assert ty in (1, 2), ty
    if ty == 1:
        return last, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
    return (last,) + code_lengths(br)[:2]


def read_header(br):
    """Block header at br.p: (last, literal/length table, distance table); br at the first body bit."""
    last, ll, dl = block_header(br)
    return last, canon(ll), canon(dl)


def token(br, lt, dt):
    """One token from br.p, as a decoder that believes a token starts there
    takes it: its symbol, br behind the token; None, br not moved, where the
    bits are no code."""
    p = br.p
    s = sym(br, lt)
    if s is None or s <= 256:
        return s
    if s <= 285:
        br.p += LEN_EXTRA[s - 257]
        d = sym(br, dt)
        if d is not None and d <= 29:
            br.p += DIST_EXTRA[d]
            return s
    br.p = p
    return None


def block_tokens(br, lt, dt):
    """Reads a block's body to its end-of-block code: (token count, bit of that code)."""
    n = 0
    while True:
        p = br.p
        s = token(br, lt, dt)
        assert s is not None
        if s == 256:
            return n, p
        n += 1


DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]


def _lut(lens):
    """(table, mask): table[the next max(lens) bits of the stream, first bit lowest] = (symbol, code length)."""
    top = max(max(lens), 1)
    table = [None] * (1 << top)
    for (l, c), s in canon(lens).items():
        r = int(format(c, "0%db" % l)[::-1], 2)
        for k in range(r, 1 << top, 1 << l):
            table[k] = (s, l)
    return table, (1 << top) - 1


class Block:
    """One block of a raw deflate stream: type (0 stored, 1 fixed, 2 dynamic),
    last, the bit its header starts at, both code-length arrays and the
    code-length symbols as sent (dynamic), the input range [b0, b1) and the
    tokens (input position, length, distance), a literal as (position, 0, byte)."""
    __slots__ = ("type", "last", "bit", "ll", "dl", "sent", "b0", "b1", "tokens")


def read_blocks(raw):
    """Every block of a whole raw deflate stream (nothing may follow it but the last byte's padding)."""
    br, out, pos, pad = Bits(raw), [], 0, raw + bytes(8)
    while True:
        b = Block()
        b.bit, b.last, b.type, b.b0, b.tokens, b.ll, b.dl, b.sent = br.p, br.bits(1), br.bits(2), pos, [], None, None, None
        assert b.type != 3, "reserved block type"
        if b.type == 0:
            br.p = (br.p + 7) & ~7
            n = br.bits(16)
            assert br.bits(16) == n ^ 0xFFFF
            assert br.p + 8 * n <= 8 * len(raw), "stored block runs past the stream"
            br.p += 8 * n
            pos += n
        else:
            if b.type == 1:
                b.ll, b.dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                b.ll, b.dl, b.sent = code_lengths(br)
            (lt, lm), (dt, dm) = _lut(b.ll), _lut(b.dl)
            p, toks = br.p, b.tokens
            while True:   # (the hot loop: table lookups on the bytes, not Bits)
                q = p >> 3
                v = int.from_bytes(pad[q:q + 8], "little") >> (p & 7)
                e = lt[v & lm]
                assert e is not None and p <= 8 * len(raw), (len(out), len(toks), pos)
                s, n = e
                p += n
                if s < 256:
                    toks.append((pos, 0, s))
                    pos += 1
                    continue
                if s == 256:
                    break
                assert s <= 285, (len(out), len(toks), pos)
                v >>= n
                x = LEN_EXTRA[s - 257]
                n = LEN_BASE[s - 257] + (v & ((1 << x) - 1))
                v >>= x
                p += x
                e = dt[v & dm]
                assert e is not None and e[0] <= 29, (len(out), len(toks), pos)
                d, x = e
                v >>= x
                p += x + DIST_EXTRA[d]
                d = DIST_BASE[d] + (v & ((1 << DIST_EXTRA[d]) - 1))
                assert d <= pos
                toks.append((pos, n, d))
                pos += n
            br.p = p
        b.b1 = pos
        out.append(b)
        if b.last:
            assert (br.p + 7) // 8 == len(raw), (br.p, len(raw))
            return out


def first_difference(got, want):
    """Where two raw deflate streams of one input first part, in the terms of
    their structure: block, symbol index and input position."""
    try:
        a = read_blocks(got)
    except (AssertionError, IndexError, TypeError) as e:
        return f"the stream does not parse: {e!r}"
    for k, y in enumerate(read_blocks(want)):
        if k >= len(a):
            return f"block {k} missing ({len(a)} blocks)"
        x = a[k]
        if (x.type, x.last, x.b0) != (y.type, y.last, y.b0):
            return f"block {k}: type/last/start {(x.type, x.last, x.b0)} for {(y.type, y.last, y.b0)}"
        for i, (s, t) in enumerate(zip(x.tokens, y.tokens)):
            if s != t:
                return f"block {k} symbol {i} at input {t[0]}: (pos, len, dist) {s} for {t}"
        if len(x.tokens) != len(y.tokens) or x.b1 != y.b1:
            return f"block {k}: {len(x.tokens)} symbols to {x.b1} for {len(y.tokens)} to {y.b1}"
        if (x.ll, x.dl) != (y.ll, y.dl):
            return f"block {k} (input {y.b0}-{y.b1}): same symbols, other code lengths"
        if x.sent != y.sent:
            return f"block {k} (input {y.b0}-{y.b1}): same code lengths, sent otherwise"
        if x.bit != y.bit:
            return f"block {k} starts at bit {x.bit} for {y.bit}"
    return "same structure (padding or trailing bits differ)"
