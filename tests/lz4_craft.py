"""Sequence-level LZ4 frame writer and a plain model.  TEST INFRASTRUCTURE ONLY.

liblz4's encoder never writes offset 0, never ends a match at the last legal
byte of a full block, stores incompressible blocks raw and picks its offsets
and lengths by what the data offers.  The decoders accept far more, so the
tests need streams the encoder cannot write.  This module writes LZ4 frames
sequence by sequence, from the format alone (pure Python):

  frame    = magic | FLG BD [content size] HC | block* | end mark [content checksum]
  block    = size word (bit 31: stored) | data [block checksum]
  data     = sequence*                       (a compressed block)
  sequence = token | literal length bytes | literals | offset | match length bytes
             (the last sequence of a block ends after its literals)

A sequence is the tuple (lit: bytes, off, ml); (lit, None, None) is the final
literal-only sequence.  A block is a list of sequences, ("stored", bytes), or
("sized", word, data): `data` written behind an explicit block-size word.
`model` decodes a list of blocks with slice arithmetic; `parse_frame` reads a
frame back into blocks, so the writer can be pinned against liblz4's encoder.
"""
import struct

MAGIC = 0x184D2204
STORED = 0x80000000


def xxh32(data, seed=0):
    """XXH32, as the LZ4 frame format uses it (header, block and content checksums)."""
    P1, P2, P3, P4, P5, M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M  # noqa: E731
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while i + 16 <= n:
            for k, w in enumerate(struct.unpack_from("<4I", data, i)):
                v[k] = rotl((v[k] + w * P2) & M, 13) * P1 & M
            i += 16
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 4 <= n:
        h = rotl((h + struct.unpack_from("<I", data, i)[0] * P3) & M, 17) * P4 & M
        i += 4
    while i < n:
        h = rotl((h + data[i] * P5) & M, 11) * P1 & M
        i += 1
    h ^= h >> 15
    h = h * P2 & M
    h ^= h >> 13
    h = h * P3 & M
    return h ^ (h >> 16)


# ---- the writer ---------------------------------------------------------------------------------
def _ext(n):
    """Length bytes of a field whose nibble is 15: 255s, then the remainder
    (the remainder-0 byte included, at 15, 270, ...)."""
    r = n - 15
    return b"\xff" * (r // 255) + bytes([r % 255])


def ext_len(n):
    return 0 if n < 15 else (n - 15) // 255 + 1


def seq(lit, off=None, ml=None):
    """The bytes of one sequence; ml=None makes it the final literal-only one."""
    ll = len(lit)
    mn = 0 if ml is None else ml - 4
    assert mn >= 0 and (ml is None) == (off is None)
    out = bytes([(min(ll, 15) << 4) | min(mn, 15)]) + (_ext(ll) if ll >= 15 else b"") + lit
    if ml is not None:
        assert 0 <= off <= 0xFFFF
        out += struct.pack("<H", off) + (_ext(mn) if mn >= 15 else b"")
    return out


def seq_len(nlit, ml=None):
    """len(seq(...)) of a sequence with nlit literals, without building it."""
    return 1 + ext_len(nlit) + nlit + (0 if ml is None else 2 + ext_len(ml - 4))


def block(seqs):
    return b"".join(seq(*s) for s in seqs)


def _is_stored(b):
    return isinstance(b, tuple) and b[0] == "stored"


def _is_sized(b):
    return isinstance(b, tuple) and b[0] == "sized"


def frame(blocks, linked=False, block_max_id=4, block_checksum=False, content_checksum=False, content_size=None,
          end_mark=True, content=None):
    """An LZ4 frame.  The content checksum is that of `content`, or of
    model(blocks, linked) when no content is given."""
    flg = 0x40 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | (0x08 if content_size is not None else 0) \
        | (0x04 if content_checksum else 0)
    desc = bytes([flg, block_max_id << 4]) + (struct.pack("<Q", content_size) if content_size is not None else b"")
    out = [struct.pack("<I", MAGIC), desc, bytes([(xxh32(desc) >> 8) & 0xFF])]
    for b in blocks:
        if _is_stored(b):
            word, data = len(b[1]) | STORED, b[1]
        elif _is_sized(b):
            word, data = b[1], b[2]
        else:
            data = b if isinstance(b, bytes) else block(b)
            word = len(data)
        out += [struct.pack("<I", word), data]
        if block_checksum:
            out.append(struct.pack("<I", xxh32(data)))
    if end_mark:
        out.append(struct.pack("<I", 0))
        if content_checksum:
            if content is None:
                content = model(blocks, linked)
            out.append(struct.pack("<I", xxh32(content)))
    return b"".join(out)


# ---- the model ----------------------------------------------------------------------------------
def decoded_len(blocks):
    """Decoded bytes of a case, from the sequence list alone."""
    n = 0
    for b in blocks:
        n += len(b[1]) if _is_stored(b) else sum(len(lit) + (ml or 0) for lit, _, ml in b)
    return n


def model(blocks, linked=False):
    """The decoded bytes of a valid case; None when an offset reaches before
    `low` (the block start, or the frame start when linked)."""
    out = bytearray()
    for b in blocks:
        if _is_stored(b):
            out += b[1]
            continue
        low = 0 if linked else len(out)
        for lit, off, ml in b:
            out += lit
            if ml is None:
                continue
            if off == 0:
                out += bytes(ml)  # lz4 1.9.3 decodes offset 0 to zeros
                continue
            n = len(out)
            if n - low < off:
                return None
            if ml <= off:
                out += out[n - off:n - off + ml]
            else:
                out += (bytes(out[n - off:]) * (-(-ml // off)))[:ml]
    return bytes(out)


# ---- the parser ---------------------------------------------------------------------------------
def parse_block(data):
    """The sequences of a compressed block as its encoder wrote them."""
    seqs, ip, n = [], 0, len(data)
    while True:
        tok = data[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                s = data[ip]
                ip += 1
                ll += s
                if s != 255:
                    break
        lit = data[ip:ip + ll]
        ip += ll
        if ip == n:
            seqs.append((lit, None, None))
            return seqs
        off = data[ip] | (data[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                s = data[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        seqs.append((lit, off, ml + 4))


def parse_frame(f):
    """(blocks, the preferences frame() takes) of a complete frame."""
    assert struct.unpack_from("<I", f, 0)[0] == MAGIC
    flg, bd = f[4], f[5]
    prefs = dict(linked=not flg & 0x20, block_max_id=bd >> 4, block_checksum=bool(flg & 0x10),
                 content_checksum=bool(flg & 0x04), content_size=None)
    pos = 6
    if flg & 0x08:
        prefs["content_size"] = struct.unpack_from("<Q", f, pos)[0]
        pos += 8
    pos += 1
    blocks = []
    while True:
        word = struct.unpack_from("<I", f, pos)[0]
        pos += 4
        if word == 0:
            break
        n = word & ~STORED
        data = f[pos:pos + n]
        pos += n + (4 if prefs["block_checksum"] else 0)
        blocks.append(("stored", data) if word & STORED else parse_block(data))
    assert pos + (4 if prefs["content_checksum"] else 0) == len(f)
    return blocks, prefs
