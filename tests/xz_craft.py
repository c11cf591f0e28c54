"""A symbol-level .xz / LZMA2 writer, parser and model.  TEST INFRASTRUCTURE ONLY.

Written from the format (xz-file-format-1.0.4, the LZMA2 chunk layer and the
LZMA symbol coder), so that tests can hold streams no encoder produces:
chosen symbols, distances and lengths, chunks that continue without a reset,
several blocks, size fields, wrong indexes.

  symbol   ("lit", b) | ("match", dist, len) | ("rep", k, len) | ("srep",) | ("eopm",)
           dist is the distance in bytes (1 = the previous byte); the end
           marker is the match whose coded distance is 0xFFFFFFFF.
  chunk    ("lzma", kind, symbols[, opts])   kind 0x80 | 0xA0 | 0xC0 | 0xE0;
                                             opts: props=(lc, lp, pb) with 0xC0 / 0xE0,
                                             props_byte, du / dc (added to the size words)
           ("stored", ctl, data[, opts])     opts: du
           ("raw", data)                     bytes as they are
  block    block(chunks, ...)                see block()
  stream   stream(blocks, ...)               see stream()

write(spec) gives the bytes, parse(bytes) the spec again (a plain LZMA decoder
that returns symbols), model(spec) the decoded bytes by slice arithmetic, or
None where a distance reaches before the dictionary.  The writer carries the
whole coder state (probabilities, state, reps, dictionary start, output) from
chunk to chunk and applies the resets a control byte implies, so a chunk that
continues without a reset is coded the way a decoder reads it.
"""
import hashlib
import struct
import zlib

P_IS_MATCH, P_IS_REP, P_G0, P_G1, P_G2, P_REP0_LONG = 0, 192, 204, 216, 228, 240
P_POS_SLOT, P_SPEC_POS, P_ALIGN, P_LEN, P_REP_LEN, P_LITERAL = 432, 688, 802, 818, 1332, 1846
L_CHOICE, L_CHOICE2, L_LOW, L_MID, L_HIGH = 0, 1, 2, 130, 258
EOPM = 0xFFFFFFFF

_CRC64 = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0xC96C5795D7870F42 if _c & 1 else 0)
    _CRC64.append(_c)


def crc64(data):
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _CRC64[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def check_bytes(check, data):
    if check == 1:
        return struct.pack("<I", zlib.crc32(data))
    if check == 4:
        return struct.pack("<Q", crc64(data))
    if check == 10:
        return hashlib.sha256(data).digest()
    return bytes(check_size(check))


def check_size(check):
    return 0 if check == 0 else 4 << ((check - 1) // 3)


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def dist_slot(d):
    """Slot of the coded distance d (the distance in bytes less one)."""
    if d < 4:
        return d
    n = d.bit_length()
    return 2 * (n - 1) + ((d >> (n - 2)) & 1)


def slot_range(slot):
    """Lowest and highest coded distance of a slot."""
    if slot < 4:
        return slot, slot
    nd = (slot >> 1) - 1
    base = (2 | (slot & 1)) << nd
    return base, base + (1 << nd) - 1


def len_class(n):
    return "low" if n < 10 else "mid" if n < 18 else "high"


# ---- the range coder ---------------------------------------------------------
class RangeEncoder:
    """liblzma's: normalise before each decision and before the flush of five bytes."""

    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry, temp = self.low >> 32, self.cache
            while True:
                self.out.append((temp + carry) & 0xFF)
                temp = 0xFF
                self.cache_size -= 1
                if self.cache_size == 0:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, probs, i, b):
        if self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()
        p = probs[i]
        bound = (self.range >> 11) * p
        if b == 0:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        else:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)

    def direct(self, v, nbits):
        for k in range(nbits - 1, -1, -1):
            if self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self.shift_low()
            self.range >>= 1
            if (v >> k) & 1:
                self.low += self.range

    def finish(self):
        if self.range < 1 << 24:  # the flush is a symbol too: the decoder's last normalisation reads this byte
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()
        for _ in range(5):
            self.shift_low()
        return bytes(self.out)


class RangeDecoder:
    def __init__(self, data):
        self.d, self.ip, self.range = data, 5, 0xFFFFFFFF
        self.code = int.from_bytes(data[1:5], "big")

    def norm(self):
        if self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.code = ((self.code << 8) | self.d[self.ip]) & 0xFFFFFFFF
            self.ip += 1

    def bit(self, probs, i):
        self.norm()
        p = probs[i]
        bound = (self.range >> 11) * p
        if self.code < bound:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
            return 0
        self.range -= bound
        self.code -= bound
        probs[i] = p - (p >> 5)
        return 1

    def direct(self, nbits):
        v = 0
        for _ in range(nbits):
            self.norm()
            self.range >>= 1
            b = 1 if self.code >= self.range else 0
            if b:
                self.code -= self.range
            v = (v << 1) | b
        return v


# ---- the LZMA coder state, shared by the writer and the parser -----------------
class Lzma:
    """Coder state of one block: model, state, reps, dictionary start and the
    block's output so far.  `base` is the stream position of the block's
    first byte; `trace` gets one record per coded symbol."""

    def __init__(self, base=0, trace=None):
        self.out, self.dict_start, self.base, self.trace = bytearray(), 0, base, trace
        self.valid = True
        self.set_props(3, 0, 2)

    def set_props(self, lc, lp, pb):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.reset_state()

    def reset_state(self):
        self.probs = [1024] * (P_LITERAL + (0x300 << min(self.lc + self.lp, 8)))
        self.state, self.reps = 0, [0, 0, 0, 0]

    def byte_back(self, d):
        """The byte d + 1 back, 0 where there is none (an invalid stream)."""
        i = len(self.out) - 1 - d
        if i < self.dict_start:
            self.valid = False
        return self.out[i] if 0 <= i < len(self.out) else 0

    def append_match(self, d, n):
        if d + 1 > len(self.out) - self.dict_start:
            self.valid = False
        for _ in range(n):
            self.out.append(self.byte_back(d))

    def note(self, kind, **kw):
        if self.trace is not None:
            pos = self.base + len(self.out)
            self.trace.append(dict(kind=kind, state=self.state, pos=pos, dpos=len(self.out) - self.dict_start,
                                   props=(self.lc, self.lp, self.pb), rep0=self.reps[0], **kw))

    # -- literal probabilities' base
    def lit_base(self):
        dpos = len(self.out) - self.dict_start
        prev = self.out[-1] if dpos else 0
        return P_LITERAL + 0x300 * (((dpos & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))

    def pos_state(self):
        return (len(self.out) - self.dict_start) & ((1 << self.pb) - 1)

    # -- encode
    def encode(self, rc, sym):
        pr, st, ps = self.probs, self.state, self.pos_state()
        kind = sym[0]
        if kind == "lit":
            b = sym[1]
            tb = self.lit_base()
            rc.bit(pr, P_IS_MATCH + (st << 4) + ps, 0)
            m = 1
            if st < 7:
                self.note("lit")
                for i in range(7, -1, -1):
                    bit = (b >> i) & 1
                    rc.bit(pr, tb + m, bit)
                    m = (m << 1) | bit
            else:
                mb, off = self.byte_back(self.reps[0]), 0x100
                diff = mb ^ b
                self.note("lit", first_diff=None if diff == 0 else diff.bit_length() - 1)
                for i in range(7, -1, -1):
                    mb <<= 1
                    mbit = mb & off
                    bit = (b >> i) & 1
                    rc.bit(pr, tb + off + mbit + m, bit)
                    m = (m << 1) | bit
                    if (mbit != 0) != (bit == 1):
                        off = 0
            self.out.append(b)
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            return
        rc.bit(pr, P_IS_MATCH + (st << 4) + ps, 1)
        if kind in ("match", "eopm"):
            d, n = (EOPM, sym[1] if len(sym) > 1 else 2) if kind == "eopm" else (sym[1] - 1, sym[2])
            slot = dist_slot(d)
            self.note(kind, slot=slot, dist=d, len=n)
            rc.bit(pr, P_IS_REP + st, 0)
            self.enc_len(rc, P_LEN, n, ps)
            self.enc_tree(rc, P_POS_SLOT + (min(n - 2, 3) << 6), 6, slot)
            if slot >= 4:
                nd = (slot >> 1) - 1
                base = (2 | (slot & 1)) << nd
                rem = d - base
                if slot < 14:
                    self.enc_rev(rc, P_SPEC_POS + base - slot - 1, nd, rem)
                else:
                    rc.direct(rem >> 4, nd - 4)
                    self.enc_rev(rc, P_ALIGN, 4, rem & 15)
            self.reps = [d] + self.reps[:3]
            self.state = 7 if st < 7 else 10
            if kind == "eopm":
                self.valid = False
                return
            self.append_match(d, n)
            return
        rc.bit(pr, P_IS_REP + st, 1)
        if kind == "srep":
            self.note("srep")
            rc.bit(pr, P_G0 + st, 0)
            rc.bit(pr, P_REP0_LONG + (st << 4) + ps, 0)
            self.state = 9 if st < 7 else 11
            self.append_match(self.reps[0], 1)
            return
        assert kind == "rep"
        k, n = sym[1], sym[2]
        self.note("rep", k=k, len=n, dist=self.reps[k])
        if k == 0:
            rc.bit(pr, P_G0 + st, 0)
            rc.bit(pr, P_REP0_LONG + (st << 4) + ps, 1)
        else:
            rc.bit(pr, P_G0 + st, 1)
            rc.bit(pr, P_G1 + st, 0 if k == 1 else 1)
            if k > 1:
                rc.bit(pr, P_G2 + st, 0 if k == 2 else 1)
            d = self.reps.pop(k)
            self.reps.insert(0, d)
        self.enc_len(rc, P_REP_LEN, n, ps)
        self.state = 8 if st < 7 else 11
        self.append_match(self.reps[0], n)

    def enc_tree(self, rc, base, nbits, v):
        m = 1
        for i in range(nbits - 1, -1, -1):
            bit = (v >> i) & 1
            rc.bit(self.probs, base + m, bit)
            m = (m << 1) | bit

    def enc_rev(self, rc, base, nbits, v):
        m = 1
        for k in range(nbits):
            bit = (v >> k) & 1
            rc.bit(self.probs, base + m, bit)
            m = (m << 1) | bit

    def enc_len(self, rc, lb, n, ps):
        v = n - 2
        assert 0 <= v < 272
        if v < 8:
            rc.bit(self.probs, lb + L_CHOICE, 0)
            self.enc_tree(rc, lb + L_LOW + (ps << 3), 3, v)
        elif v < 16:
            rc.bit(self.probs, lb + L_CHOICE, 1)
            rc.bit(self.probs, lb + L_CHOICE2, 0)
            self.enc_tree(rc, lb + L_MID + (ps << 3), 3, v - 8)
        else:
            rc.bit(self.probs, lb + L_CHOICE, 1)
            rc.bit(self.probs, lb + L_CHOICE2, 1)
            self.enc_tree(rc, lb + L_HIGH, 8, v - 16)

    # -- decode one symbol (a valid stream)
    def dec_tree(self, rd, base, nbits):
        m = 1
        for _ in range(nbits):
            m = (m << 1) | rd.bit(self.probs, base + m)
        return m - (1 << nbits)

    def dec_rev(self, rd, base, nbits):
        m, v = 1, 0
        for k in range(nbits):
            bit = rd.bit(self.probs, base + m)
            m = (m << 1) | bit
            v |= bit << k
        return v

    def dec_len(self, rd, lb, ps):
        if rd.bit(self.probs, lb + L_CHOICE) == 0:
            return 2 + self.dec_tree(rd, lb + L_LOW + (ps << 3), 3)
        if rd.bit(self.probs, lb + L_CHOICE2) == 0:
            return 10 + self.dec_tree(rd, lb + L_MID + (ps << 3), 3)
        return 18 + self.dec_tree(rd, lb + L_HIGH, 8)

    def decode(self, rd):
        pr, st, ps = self.probs, self.state, self.pos_state()
        if rd.bit(pr, P_IS_MATCH + (st << 4) + ps) == 0:
            tb, m = self.lit_base(), 1
            if st < 7:
                while m < 0x100:
                    m = (m << 1) | rd.bit(pr, tb + m)
            else:
                mb, off = self.byte_back(self.reps[0]), 0x100
                while m < 0x100:
                    mb <<= 1
                    mbit = mb & off
                    bit = rd.bit(pr, tb + off + mbit + m)
                    m = (m << 1) | bit
                    if (mbit != 0) != (bit == 1):
                        off = 0
            self.out.append(m & 0xFF)
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            return ("lit", m & 0xFF)
        if rd.bit(pr, P_IS_REP + st) == 0:
            n = self.dec_len(rd, P_LEN, ps)
            slot = self.dec_tree(rd, P_POS_SLOT + (min(n - 2, 3) << 6), 6)
            d = slot
            if slot >= 4:
                nd = (slot >> 1) - 1
                d = (2 | (slot & 1)) << nd
                if slot < 14:
                    d += self.dec_rev(rd, P_SPEC_POS + d - slot - 1, nd)
                else:
                    d += rd.direct(nd - 4) << 4
                    d += self.dec_rev(rd, P_ALIGN, 4)
            self.reps = [d] + self.reps[:3]
            self.state = 7 if st < 7 else 10
            if d == EOPM:
                return ("eopm",)
            self.append_match(d, n)
            return ("match", d + 1, n)
        if rd.bit(pr, P_G0 + st) == 0:
            if rd.bit(pr, P_REP0_LONG + (st << 4) + ps) == 0:
                self.state = 9 if st < 7 else 11
                self.append_match(self.reps[0], 1)
                return ("srep",)
            k = 0
        else:
            k = 1 if rd.bit(pr, P_G1 + st) == 0 else 2 if rd.bit(pr, P_G2 + st) == 0 else 3
            self.reps.insert(0, self.reps.pop(k))
        n = self.dec_len(rd, P_REP_LEN, ps)
        self.state = 8 if st < 7 else 11
        self.append_match(self.reps[0], n)
        return ("rep", k, n)


# ---- the spec's constructors -----------------------------------------------------
def lzma(kind, symbols, **opts):
    return ("lzma", kind, list(symbols), opts)


def stored(ctl, data, **opts):
    return ("stored", ctl, bytes(data), opts)


def raw(data):
    return ("raw", bytes(data))


def block(chunks, dict_prop=0, csize=None, usize=None, filters=(), pad=None, end=True):
    """csize / usize: None (field absent), True (the true value) or a number.
    filters: (("delta", dist),) in front of LZMA2.  pad: the block padding's
    bytes (None: the zeros the format asks for).  end: write the 0x00 that
    ends the LZMA2 data."""
    return dict(chunks=list(chunks), dict_prop=dict_prop, csize=csize, usize=usize, filters=tuple(filters), pad=pad,
                end=end)


def stream(blocks, check=4, index=None, footer=None, trailing=b""):
    """index: None (rebuilt from the blocks) or dict(count=, records=[(unpadded,
    uncompressed)], pad=bytes), each optional.  footer: dict(backward=, check=)."""
    return dict(blocks=list(blocks), check=check, index=index, footer=footer, trailing=bytes(trailing))


def props_byte(lc, lp, pb):
    return (pb * 5 + lp) * 9 + lc


# ---- the writer ------------------------------------------------------------------------
def write_chunks(chunks, base=0, trace=None):
    """(bytes of the chunks, the coder with the block's output)."""
    lz, out = Lzma(base, trace), bytearray()
    for ch in chunks:
        if ch[0] == "raw":
            out += ch[1]
        elif ch[0] == "stored":
            ctl, data, opts = ch[1], ch[2], ch[3] if len(ch) > 3 else {}
            if ctl == 1:
                lz.dict_start = len(lz.out)
            if trace is not None:
                trace.append(dict(kind="stored", ctl=ctl, pos=base + len(lz.out), len=len(data)))
            out += bytes([ctl]) + struct.pack(">H", (len(data) - 1 + opts.get("du", 0)) & 0xFFFF) + data
            lz.out += data
        else:
            kind, syms, opts = ch[1], ch[2], ch[3] if len(ch) > 3 else {}
            if kind == 0xE0:
                lz.dict_start = len(lz.out)
            if kind >= 0xC0:
                lz.set_props(*opts.get("props", (3, 0, 2)))
            elif kind == 0xA0:
                lz.reset_state()
            if trace is not None:
                trace.append(dict(kind="lzma", ctl=kind, pos=base + len(lz.out)))
            rc, start = RangeEncoder(), len(lz.out)
            for s in syms:
                lz.encode(rc, s)
            data = rc.finish()
            if "first_byte" in opts:
                data = bytes([opts["first_byte"]]) + data[1:]
            usz = len(lz.out) - start - 1 + opts.get("du", 0)
            csz = len(data) - 1 + opts.get("dc", 0)
            assert 0 <= usz < 1 << 21 and 0 <= csz < 1 << 16, (usz, csz)
            out += bytes([kind | (usz >> 16)]) + struct.pack(">HH", usz & 0xFFFF, csz)
            if kind >= 0xC0:
                out.append(opts.get("props_byte", props_byte(lz.lc, lz.lp, lz.pb)))
            out += data
    return bytes(out), lz


def delta_encode(data, dist):
    return bytes((data[i] - (data[i - dist] if i >= dist else 0)) & 0xFF for i in range(len(data)))


def delta_decode(data, dist):
    out = bytearray(data)
    for i in range(dist, len(out)):
        out[i] = (out[i] + out[i - dist]) & 0xFF
    return bytes(out)


def write(spec, trace=None, layout=None):
    """The stream's bytes.  layout (a list) gets one dict per block: where its
    header, data, padding and check start, and the positions of its chunks."""
    check = spec["check"]
    out = bytearray(b"\xfd7zXZ\x00")
    flags = bytes([0, check])
    out += flags + struct.pack("<I", zlib.crc32(flags))
    records, upos = [], 0
    for b in spec["blocks"]:
        data, lz = write_chunks(b["chunks"], upos, trace)
        if b["end"]:
            data += b"\x00"
        content = bytes(lz.out)
        for name, dist in reversed(b["filters"]):
            content = delta_decode(content, dist)
        cs, us = b["csize"], b["usize"]
        hdr = bytearray([0, (len(b["filters"])) | (0x40 if cs is not None else 0) | (0x80 if us is not None else 0)])
        if cs is not None:
            hdr += vli(len(data) if cs is True else cs)
        if us is not None:
            hdr += vli(len(content) if us is True else us)
        for name, dist in b["filters"]:
            hdr += bytes([0x03, 1, dist - 1])
        hdr += bytes([0x21, 1, b["dict_prop"]])
        hdr += bytes(-len(hdr) % 4)
        hdr[0] = len(hdr) // 4
        hdr += struct.pack("<I", zlib.crc32(bytes(hdr)))
        pad = bytes(-len(data) % 4) if b["pad"] is None else b["pad"]
        if layout is not None:
            layout.append(dict(header=len(out), data=len(out) + len(hdr), pad=len(out) + len(hdr) + len(data),
                               check=len(out) + len(hdr) + len(data) + len(pad), ustart=upos, usize=len(content)))
        out += hdr + data + pad + check_bytes(check, content)
        records.append((len(hdr) + len(data) + check_size(check), len(content)))
        upos += len(content)
    ix = spec["index"] or {}
    recs = ix.get("records", records)
    index = bytearray(b"\x00" + vli(ix.get("count", len(recs))))
    for unp, usz in recs:
        index += vli(unp) + vli(usz)
    index += ix.get("pad", bytes(-len(index) % 4))
    index += struct.pack("<I", zlib.crc32(bytes(index)))
    out += index
    ft = spec["footer"] or {}
    tail = struct.pack("<I", ft.get("backward", len(index) // 4 - 1)) + bytes([0, ft.get("check", check)])
    out += struct.pack("<I", zlib.crc32(tail)) + tail + b"YZ" + spec["trailing"]
    return bytes(out)


# ---- the parser (valid streams) ---------------------------------------------------------
def read_vli(s, p):
    v, k = 0, 0
    while True:
        b = s[p]
        p += 1
        v |= (b & 0x7F) << (7 * k)
        k += 1
        if not b & 0x80:
            return v, p


def parse_chunks(s, p):
    """The chunks from s[p] up to the 0x00 that ends them: (chunks, position behind the 0x00)."""
    lz, chunks = Lzma(), []
    while s[p] != 0:
        ctl = s[p]
        if ctl < 0x80:
            n = struct.unpack(">H", s[p + 1:p + 3])[0] + 1
            if ctl == 1:
                lz.dict_start = len(lz.out)
            chunks.append(stored(ctl, s[p + 3:p + 3 + n]))
            lz.out += s[p + 3:p + 3 + n]
            p += 3 + n
            continue
        kind = ctl & 0xE0
        usz = ((ctl & 0x1F) << 16) + struct.unpack(">H", s[p + 1:p + 3])[0] + 1
        csz = struct.unpack(">H", s[p + 3:p + 5])[0] + 1
        p += 5
        opts = {}
        if kind == 0xE0:
            lz.dict_start = len(lz.out)
        if kind >= 0xC0:
            pr = s[p]
            p += 1
            opts["props"] = (pr % 9, pr // 9 % 5, pr // 45)
            lz.set_props(*opts["props"])
        elif kind == 0xA0:
            lz.reset_state()
        rd, end, syms = RangeDecoder(s[p:p + csz]), len(lz.out) + usz, []
        while len(lz.out) < end:
            syms.append(lz.decode(rd))
        assert len(lz.out) == end
        chunks.append(lzma(kind, syms, **opts))
        p += csz
    return chunks, p + 1


def parse(s):
    assert s[:6] == b"\xfd7zXZ\x00"
    check, p, blocks = s[7], 12, []
    while s[p] != 0:
        h0, hsize, bflags = p, s[p] * 4 + 4, s[p + 1]
        p += 2
        cs = us = None
        if bflags & 0x40:
            cs, p = read_vli(s, p)
        if bflags & 0x80:
            us, p = read_vli(s, p)
        filters, dict_prop = [], 0
        for _ in range((bflags & 3) + 1):
            fid, p = read_vli(s, p)
            psz, p = read_vli(s, p)
            if fid == 0x03:
                filters.append(("delta", s[p] + 1))
            else:
                assert fid == 0x21
                dict_prop = s[p]
            p += psz
        p = h0 + hsize
        chunks, q = parse_chunks(s, p)
        if cs is not None:
            assert cs == q - p
            cs = True
        if us is not None:
            us = True
        blocks.append(block(chunks, dict_prop, cs, us, filters))
        p = q + (-(q - p) % 4) + check_size(check)
    i0 = p
    n, p = read_vli(s, p + 1)
    for _ in range(2 * n):
        _, p = read_vli(s, p)
    p += -(p - i0) % 4 + 4 + 12
    return stream(blocks, check, trailing=s[p:])


# ---- the model --------------------------------------------------------------------------
def model_block(chunks, limit=None):
    """A block's LZMA2 output by slice arithmetic, None where a distance
    reaches before the dictionary start (what lies behind `limit` bytes of
    output is not looked at)."""
    out, dict_start, reps = bytearray(), 0, [0, 0, 0, 0]
    for ch in chunks:
        if limit is not None and len(out) >= limit:
            break
        if ch[0] == "raw":
            return None
        if ch[0] == "stored":
            if ch[1] == 1:
                dict_start = len(out)
            out += ch[2]
            continue
        if ch[1] == 0xE0:
            dict_start = len(out)
        if ch[1] >= 0xA0:
            reps = [0, 0, 0, 0]
        for s in ch[2]:
            if limit is not None and len(out) >= limit:
                break
            if s[0] == "lit":
                out.append(s[1])
                continue
            if s[0] == "eopm":
                return None
            if s[0] == "match":
                reps = [s[1] - 1] + reps[:3]
                n = s[2]
            elif s[0] == "rep":
                reps.insert(0, reps.pop(s[1]))
                n = s[2]
            else:
                n = 1
            d = reps[0] + 1
            if d > len(out) - dict_start:
                return None
            src = out[len(out) - d:]
            out += (src * (n // d + 1))[:n]
    return bytes(out)


def model(spec, D=None):
    """The stream's decoded bytes (the first D), None where it has none."""
    out = b""
    for b in spec["blocks"]:
        if D is not None and len(out) >= D:
            break
        m = model_block(b["chunks"], None if D is None else D - len(out))
        if m is None:
            return None
        for name, dist in reversed(b["filters"]):
            m = delta_decode(m, dist)
        out += m
    return out if D is None else out[:D]
