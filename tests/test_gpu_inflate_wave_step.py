"""The one-wave-per-chunk inflate kernel's decode step: steady / edge bodies of
pass 1 and the token-ready Huffman tables.

Every stream is decoded through the default dispatch and through
FLAG_INFLATE_WAVE, each with and without FLAG_DEBUG_INFLATE_LONG_SEG, in one
batch launch per flag set; status and bytes must equal the oracle's, and the
bytes after N in the caller's buffer must stay untouched.  Streams come from
the system zlib; their structure (code lengths, token positions) is read back
with a small deflate parser so that each case checks that it has the property
it is there for.
"""
import struct
import zlib

import numpy as np
import pytest

import zref
from golden_util import CODEC_IDS, dtype_info
from zarr_amd import ArrayMetadata, Gzip, _native

pytestmark = pytest.mark.gpu

KIND = {zref.OK: "Ok", zref.EOF: "UnexpectedEof", zref.INVALID_DATA: "InvalidData"}
FLAG_SETS = (0, _native.FLAG_INFLATE_WAVE, _native.FLAG_DEBUG_INFLATE_LONG_SEG,
             _native.FLAG_INFLATE_WAVE | _native.FLAG_DEBUG_INFLATE_LONG_SEG)
GUARD = 4096


def gzip_wrap(raw_deflate, payload):
    h = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255])
    return h + raw_deflate + struct.pack("<II", zlib.crc32(payload), len(payload) & 0xFFFFFFFF)


def deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(payload) + c.flush()


def check_batch(streams, dt, n):
    """One launch per flag set: oracle parity of status and bytes, guard intact."""
    import torch
    from zarr_amd.batch import BatchCodec, PackedStreams
    es, be, isb, _ = dtype_info(dt)
    D = n * es
    st_ref, out_ref = zref.decode_batch(CODEC_IDS["gzip"], [np.frombuffer(s, np.uint8) for s in streams],
                                        D, elem_size=es, big_endian=be, is_bool=isb)
    meta = ArrayMetadata.new([n], [n], dt, Gzip(-1))
    for flags in FLAG_SETS:
        dst = torch.full((len(streams) * (D + GUARD),), 0xAB, dtype=torch.uint8, device="cuda:0")
        packed = PackedStreams(streams, D + GUARD, "cuda:0", dst=dst)
        BatchCodec(0).decode(meta, packed, flags=flags)
        torch.cuda.synchronize()
        st = packed.status.cpu().numpy()
        out = dst.cpu().numpy().reshape(len(streams), D + GUARD)
        for i in range(len(streams)):
            assert KIND[int(st[i])] == KIND[int(st_ref[i])], (i, flags, int(st[i]), int(st_ref[i]))
            if st_ref[i] == zref.OK:
                assert out[i, :D].tobytes() == out_ref[i].tobytes(), (i, flags)
            assert (out[i, D:] == 0xAB).all(), (i, flags)
    return st_ref


# ---- a small deflate parser: code lengths and token positions of the first blocks ----
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    def __init__(self, b):
        self.b = b
        self.p = 0

    def bits(self, n):  # n <= 16
        p = self.p
        x = (int.from_bytes(self.b[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)
        self.p = p + n
        return x


def canon(lens):
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
    c = l = 0
    while True:
        c = (c << 1) | br.bits(1)
        l += 1
        if (l, c) in table:
            return table[(l, c)]


def parse_blocks(raw, nblocks):
    """The first `nblocks` blocks of a raw deflate stream (fixed or dynamic blocks):
    [{lmax, dmax, tokens: [(stream bit after the token, output bytes after it, length)]}]."""
    br, out, produced = Bits(raw), [], 0
    for _ in range(nblocks):
        last, ty = br.bits(1), br.bits(2)
        assert ty in (1, 2), ty
        if ty == 1:
            hl, ls = 288, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 30
        else:
            hl, hd, hc = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            cl = [0] * 19
            for i in range(hc):
                cl[CLEN_ORDER[i]] = br.bits(3)
            ct, ls = canon(cl), []
            while len(ls) < hl + hd:
                s = sym(br, ct)
                if s < 16:
                    ls.append(s)
                elif s == 16:
                    ls += [ls[-1]] * (3 + br.bits(2))
                elif s == 17:
                    ls += [0] * (3 + br.bits(3))
                else:
                    ls += [0] * (11 + br.bits(7))
        lt, dt = canon(ls[:hl]), canon(ls[hl:])
        toks = []
        while True:
            s = sym(br, lt)
            if s == 256:
                break
            n = 1
            if s > 256:
                n = LEN_BASE[s - 257] + br.bits(LEN_EXTRA[s - 257])
                br.bits(DIST_EXTRA[sym(br, dt)])
            produced += n
            toks.append((br.p, produced, n))
        out.append({"lmax": max(ls[:hl]), "dmax": max(ls[hl:]), "tokens": toks})
        if last:
            break
    return out


# ---- payloads (built once) ---------------------------------------------------------------
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


@pytest.fixture(scope="module")
def case1():
    payload = _skewed_with_copies()
    raw = deflate(payload, 6)
    return payload, raw, gzip_wrap(raw, payload)


@pytest.fixture(scope="module")
def case2():
    payload = _three_symbols()
    raw = deflate(payload, 6, zlib.Z_HUFFMAN_ONLY)
    return payload, raw, gzip_wrap(raw, payload)


def test_subtable_codes_through_rewritten_tables(case1):
    """Literal/length codes longer than the 9-bit root and distance codes
    longer than the 8-bit root: both tables' subtable links and entries go
    through the in-place rewrite."""
    payload, raw, s = case1
    blocks = parse_blocks(raw, 2)
    assert max(b["lmax"] for b in blocks) > 9 and max(b["dmax"] for b in blocks) > 8
    st = check_batch([s], "u1", len(payload))
    assert st[0] == zref.OK


def test_list_cap_and_steady_to_edge_switch(case2):
    """Three-symbol Huffman-only data: ~1.1 bits per token, so every round's
    token lists fill (IW_TCAP = 768 against > 3 000 tokens in a 4 096-bit
    segment) and pass 1 goes back from the steady to the edge body for the cap."""
    payload, raw, s = case2
    toks = parse_blocks(raw, 1)[0]["tokens"]
    i0 = len(toks) // 2
    span = sum(1 for t in toks[i0:i0 + 4096] if t[0] < toks[i0][0] + 4096)
    assert span > 3000, span
    st = check_batch([s], "u1", len(payload))
    assert st[0] == zref.OK


def test_short_segments_inside_the_mark_zone(case1):
    """Small blocks (memLevel 1: ~127 tokens each, segments at IW_SEGMIN, never
    past the marked IW_MARKW words) next to memLevel 4 and 9 (the switch to
    the steady body inside a segment), at levels 1, 6 and 9."""
    payload = case1[0][: 32 << 10]
    small = parse_blocks(deflate(payload, 6, mem=1), 1000)
    assert len(small) >= 100 and max(len(b["tokens"]) for b in small) <= 128, len(small)
    streams = [gzip_wrap(deflate(payload, lv, mem=mem), payload) for mem in (1, 4, 9) for lv in (1, 6, 9)]
    st = check_batch(streams, "u1", len(payload))
    assert (st == zref.OK).all()


def test_stream_end_in_the_edge_body(case1):
    """Truncated at each of the last 48 byte positions and at 16 positions over
    the middle: the lanes near the stream end run the edge body (the steady
    body needs 8 x 48 bits of slack) and the result is the oracle's."""
    payload, raw, s = case1
    cuts = [len(s) - k for k in range(1, 49)] + [len(s) * k // 18 for k in range(1, 17)]
    st = check_batch([s[:c] for c in cuts], "u1", len(payload))
    assert (st != zref.OK).sum() >= 48 - 8  # (the last cuts fall in the 8-byte gzip trailer)


@pytest.mark.parametrize("which", ["case1", "case2"])
def test_lookahead_on_rewritten_tables(which, request):
    """The output fills inside the second dynamic block, so zlib's look-ahead
    decodes the next token with the tables the H round rewrote (they are
    turned back first).  Nine N per stream: after the block's first tokens, in
    its middle, at its last tokens (the look-ahead then reads the EOB and the
    next header) and inside matches; then the same with the 64 stream bytes
    after that point set to 0xFF."""
    payload, raw, s = request.getfixturevalue(which)
    toks = parse_blocks(raw, 2)[1]["tokens"]
    n = len(toks)
    picks = [(toks[i][0], toks[i][1]) for i in (0, 1, n // 4, n // 2, 3 * n // 4, n - 2, n - 1)]
    matches = [t for t in toks if t[2] > 3]
    if matches:  # the output ends inside a match
        picks += [(m[0], m[1] - 1) for m in (matches[0], matches[-1])]
    else:
        picks += [(toks[i][0], toks[i][1]) for i in (n // 8, 7 * n // 8)]
    assert len(picks) == 9
    for bit, N in picks:
        at = 10 + (bit >> 3) + 1  # the first whole stream byte after the token
        ff = bytearray(s)
        ff[at:at + 64] = b"\xff" * 64
        check_batch([s, bytes(ff)], "u1", N)


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_swapped_and_bool_dtypes(case1, dt):
    """The !wide_ok paths (byte-swapped far sources, bool normalisation)."""
    payload, raw, s = case1
    es = dtype_info(dt)[0]
    st = check_batch([s], dt, len(payload) // es)
    assert st[0] == zref.OK
