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
import zlib

import pytest

from deflate_kit import (DIST_EXTRA, LEN_BASE, LEN_EXTRA, Bits, _skewed_with_copies, _three_symbols, block_header,
                         canon, deflate, gzip_wrap, sym)
from golden_util import dtype_info
from gpu_check import GUARD, check_many
from zarr_amd import _native

pytestmark = pytest.mark.gpu

FLAG_SETS = (0, _native.FLAG_INFLATE_WAVE, _native.FLAG_DEBUG_INFLATE_LONG_SEG,
             _native.FLAG_INFLATE_WAVE | _native.FLAG_DEBUG_INFLATE_LONG_SEG)


def check_batch(streams, dt, n):
    """One launch per flag set: oracle parity of status and bytes, guard intact."""
    return check_many("gzip", streams, dt, n, FLAG_SETS, guard=GUARD)


def parse_blocks(raw, nblocks):
    """The first `nblocks` blocks of a raw deflate stream (fixed or dynamic blocks):
    [{lmax, dmax, tokens: [(stream bit after the token, output bytes after it, length)]}]."""
    br, out, produced = Bits(raw), [], 0
    for _ in range(nblocks):
        last, ll, dl = block_header(br)
        lt, dt = canon(ll), canon(dl)
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
        out.append({"lmax": max(ll), "dmax": max(dl), "tokens": toks})
        if last:
            break
    return out


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
    assert st[0] == "Ok"


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
    assert st[0] == "Ok"


def test_short_segments_inside_the_mark_zone(case1):
    """Small blocks (memLevel 1: ~127 tokens each, segments at IW_SEGMIN, never
    past the marked IW_MARKW words) next to memLevel 4 and 9 (the switch to
    the steady body inside a segment), at levels 1, 6 and 9."""
    payload = case1[0][: 32 << 10]
    small = parse_blocks(deflate(payload, 6, mem=1), 1000)
    assert len(small) >= 100 and max(len(b["tokens"]) for b in small) <= 128, len(small)
    streams = [gzip_wrap(deflate(payload, lv, mem=mem), payload) for mem in (1, 4, 9) for lv in (1, 6, 9)]
    st = check_batch(streams, "u1", len(payload))
    assert set(st) == {"Ok"}


def test_stream_end_in_the_edge_body(case1):
    """Truncated at each of the last 48 byte positions and at 16 positions over
    the middle: the lanes near the stream end run the edge body (the steady
    body needs 8 x 48 bits of slack) and the result is the oracle's."""
    payload, raw, s = case1
    cuts = [len(s) - k for k in range(1, 49)] + [len(s) * k // 18 for k in range(1, 17)]
    st = check_batch([s[:c] for c in cuts], "u1", len(payload))
    assert sum(k != "Ok" for k in st) >= 48 - 8  # (the last cuts fall in the 8-byte gzip trailer)


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
    assert st[0] == "Ok"
