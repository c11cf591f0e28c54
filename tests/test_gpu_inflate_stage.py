"""The wave inflate kernel's L-phase stage (zcg_inflate_wave.hip): a ring of
IW_S = 4 096 entries that lies over the Huffman tables, which are saved to the
workspace per block and loaded back before a further H round and before the
look-ahead.  Near distances that only the larger ring has, the stages that
keep the 2 032-byte capacity and 15-bit distances (byte-swapped dtypes, fewer
than 16 bytes of room), stage edges, both table reloads and the status paths
late in a stage.

Every stream goes through the default dispatch, FLAG_INFLATE_WAVE and
FLAG_SERIAL_INFLATE, one batch launch per flag set, against the oracle, with
guard bytes behind every chunk.  What a case is there for is asserted on the
host first (deflate_kit's reader and a model of the kernel's stage rule), in
test_host_properties, which needs no GPU.
"""
import functools
import zlib

import numpy as np
import pytest

from deflate_kit import (PLAIN_HEADER, Bits, _three_symbols, deflate, flip, gzip_wrap, noise, read_blocks, read_header,
                         stored, text, token, trailer)
from golden_util import dtype_info
from gpu_check import GUARD, check_many, oracle
from zarr_amd import _native

FLAG_SETS = (0, _native.FLAG_INFLATE_WAVE, _native.FLAG_SERIAL_INFLATE)

# the kernel's constants (zcg_inflate_wave.hip)
CAP_WIDE = 4096 - 16    # stage capacity with 16-byte source pieces (IW_S - 16)
CAP_NARROW = 2048 - 16  # byte-swapped dtypes and stages with fewer than 16 bytes of room (IW_SN - 16)
IW_TCAP = 768           # tokens per lane list
IW_SEGMAX = 4096        # bits per lane segment at most
SEG0 = ((64 * 3072 * 108 // 100 // 64) + 31) & ~31  # a chunk's first round: bits per lane segment


def check(streams, dt, n, want=None, ref=None):
    return check_many("gzip", streams, dt, n, FLAG_SETS, guard=GUARD, want=want, ref=ref)


def quant_chunk(idx):
    """bench.py's C2 "quant" chunk: round(64 (100 sin(0.05 (i + 7 idx)) cos(0.03 j) + k)) / 64 as <f4."""
    i = np.arange(256, dtype=np.float64)[:, None, None]
    j = np.arange(256, dtype=np.float64)[None, :, None]
    k = np.arange(4, dtype=np.float64)[None, None, :]
    v = np.round(64 * (100 * np.sin(0.05 * (i + idx * 7)) * np.cos(0.03 * j) + k)) / 64
    return v.astype("<f4").reshape(-1)


# ---- host side: tokens and the stage rule ------------------------------------------------------
def tokens_of(raw):
    """(output position, length (0: a literal), distance or byte) of every token, in stream order."""
    return [t for b in read_blocks(raw) for t in b.tokens]


def stage_starts(raw, D, swap=False, start=0):
    """Output positions at which the kernel starts a stage while it decodes D
    bytes of a stream whose Huffman tokens all come from ONE H round (one
    block, no capped list), after `start` bytes of stored blocks.  The rule:
    groups of 128 tokens; a group that does not fit whole ends a stage that
    has bytes already; the last stage (room <= capacity) clips at D."""
    toks = [max(1, t[1]) for t in tokens_of(raw)]
    i, P, out = 0, start, []
    while P < D and i < len(toks):
        out.append(P)
        room = D - P
        capS = CAP_NARROW if swap or room < 16 else CAP_WIDE
        cap = min(room, capS)
        fin, emitted = cap == room, 0
        while True:
            grp, take, e = toks[i:i + 128], 0, emitted
            for ln in grp:
                if (e < cap) if fin else (e + ln <= cap):
                    take, e = take + 1, e + ln
                else:
                    break
            if not fin and emitted and take < len(grp):
                break  # rejected: the group starts the next stage
            i, emitted = i + take, e
            if (fin and emitted >= cap) or take < 128:
                break
        P += min(emitted, cap)
    return out


def token_bits(raw):
    """[(bit of the token's first code bit, output position)] of the first block, and the bit of its end-of-block code."""
    br = Bits(raw)
    _, lt, dt = read_header(br)
    blk, out = read_blocks(raw)[0], []
    for pos, _, _ in blk.tokens:
        out.append((br.p, pos))
        assert token(br, lt, dt) is not None
    return out, br.p


# ---- payloads and streams (built once per session) ----------------------------------------------
@functools.lru_cache(maxsize=None)
def near_payload():
    """Case 1: 3 000 noise bytes three times over: matches at distance 3 000 from position 3 000 on."""
    a = noise(3000, 11)
    return a + a + a


@functools.lru_cache(maxsize=None)
def far32k():
    """(payload, raw deflate, member) with matches at the largest distance,
    32 768, which zlib's own encoder never sends (its window stops 262 bytes
    short): 32 768 noise bytes in a stored block, then a fixed-code block that
    copies the first 300 of them (258 + 42 bytes)."""
    a = noise(32768, 12)
    bits, n = 0, 0

    def put(x, k):  # k bits, lowest first (header fields, extra bits)
        nonlocal bits, n
        bits, n = bits | (x << n), n + k

    def code(c, k):  # a Huffman code, highest bit first
        for i in range(k - 1, -1, -1):
            put((c >> i) & 1, 1)

    put(1, 1), put(1, 2)                                            # last block, fixed codes
    code(0b11000101, 8), code(29, 5), put(32768 - 24577, 13)        # length 258 (symbol 285), distance code 29
    code(273 - 256, 7), put(42 - 35, 3), code(29, 5), put(32768 - 24577, 13)  # length 42 (symbol 273)
    code(0, 7)                                                      # end of block
    raw = stored(a) + bits.to_bytes((n + 7) // 8, "little")
    p = a + a[:300]
    return p, raw, PLAIN_HEADER + raw + trailer(p)


@functools.lru_cache(maxsize=None)
def gz(payload_fn, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    p = payload_fn()
    raw = deflate(p, level, strategy, mem)
    return p, raw, gzip_wrap(raw, p)


@functools.lru_cache(maxsize=None)
def edge_payloads():
    return text(16384, 31), quant_chunk(0).tobytes()[:16384]


@functools.lru_cache(maxsize=None)
def edge_streams():
    """Each edge payload as one deflate stream, and behind a stored block of its first 5 bytes."""
    out = []
    for p in edge_payloads():
        out.append(gzip_wrap(deflate(p, 6), p))
    for p in edge_payloads():
        out.append(PLAIN_HEADER + stored(p[:5]) + deflate(p[5:], 6) + trailer(p))
    return out


EDGES = [4079, 4080, 4081, 8159, 8160, 8161]
STORED_SIZES = [4079, 1, 4081, 0, 16383, 17, 8160, 0, 7279]


@functools.lru_cache(maxsize=None)
def stored_member():
    payload = noise(40000, 4002)
    assert sum(STORED_SIZES) == len(payload)
    raw, at = b"", 0
    for i, k in enumerate(STORED_SIZES):
        raw += stored(payload[at:at + k], last=i == len(STORED_SIZES) - 1)
        at += k
    return PLAIN_HEADER + raw + trailer(payload)


def c2_256k():
    return quant_chunk(0).tobytes()[: 256 << 10]


SHORT_SEEDS = (15, 16, 17)  # (noise that holds no match of its own)


@functools.lru_cache(maxsize=None)
def short_room_payload():
    """Case 2: a first stage of 4 079 bytes and a match across its end.  A
    stage inside a block is short of room only behind a stage that the rule
    left nearly full (N > 4 080, or the first stage would be the last; a stage
    at a block start behind a stored block is the other way, far32k): 31 groups of 128 tokens
    = 1 500 literals, one match of 112 bytes and 2 467 literals end at 4 079,
    and the group behind them, which starts with a match of 60 bytes at
    distance 3 879, does not fit."""
    a, b = noise(1500, SHORT_SEEDS[0], hi=200), noise(2467, SHORT_SEEDS[1], hi=200)
    return a + a[100:212] + b + a[200:260] + noise(200, SHORT_SEEDS[2], hi=200)


SHORT_ROOM = [4081, 4084, 4086, 4092, 4094]  # 2, 5, 7, 13 and 15 bytes behind 4 079


@functools.lru_cache(maxsize=None)
def lookahead_cases():
    """Case 5: (stream, [N, N - 1]) with N a token boundary inside a Huffman
    block behind at least one full stage: before a match, and before an
    end-of-block code (blocks of 4 095 tokens: memLevel 6)."""
    p = text(40000, 32)
    raw = deflate(p, 6, mem=6)
    blocks = read_blocks(raw)
    assert all(b.type != 0 for b in blocks)
    b = next(b for b in blocks if not b.last and b.b1 > 2 * CAP_WIDE)
    n_eob = b.b1
    n_match = next(pos for pos, ln, _ in b.tokens if ln and pos > b.b0 + CAP_WIDE + 100)
    return gzip_wrap(raw, p), b, n_match, n_eob


@functools.lru_cache(maxsize=None)
def status_cases():
    """Case 6: [(stream, N, expected kind, output position of the fault)].  A
    match whose distance is made larger than its position by flipping the top
    extra bit of its distance code (the token's last bit), and a stream cut
    inside a token; each late in the first stage and late in the second."""
    out = []
    for at, back in ((2100, 2099), (6100, 5100)):
        a = noise(at, 40 + at, hi=128)
        p = a + a[at - back:at - back + 200] + noise(300, 41, hi=128)
        raw = deflate(p, 6)
        tb, _ = token_bits(raw)
        k = next(i for i, (_, pos) in enumerate(tb) if pos == at)
        t = read_blocks(raw)[0].tokens[k]
        assert t[1] >= 3 and t[2] == back, t
        last_bit = tb[k + 1][0] - 1
        bad = flip(raw, last_bit >> 3, 1 << (last_bit & 7))
        out.append((gzip_wrap(bad, p), len(p), "invalid", at, raw))
        cut_bit = next(b for b, pos in tb if pos >= at + 250)
        out.append((PLAIN_HEADER + raw[:cut_bit >> 3], len(p), "eof", at + 250, raw))
    return out


# ---- the properties, on the host --------------------------------------------------------------
def test_host_properties():
    # 1. a near match the 2 048-entry ring could not hold: source inside the first stage, 2 048 or more back
    _, raw, _ = gz(near_payload)
    assert len(read_blocks(raw)) == 1
    assert any(ln and 2048 <= d <= pos and pos + ln <= CAP_WIDE for pos, ln, d in tokens_of(raw))
    # 2. a match at distance 32 768; the short-room sizes end in a stage of 1..15 bytes
    p32, raw32, _ = far32k()
    assert [(ln, d) for _, ln, d in tokens_of(raw32)] == [(258, 32768), (42, 32768)]
    assert zlib.decompress(raw32, -15) == p32
    # ... and behind its stored block the Huffman block's one stage starts at 32 768 with 1..15 bytes of room:
    # no 16-byte pieces, so its first token is a near part whose source lies 32 768 back (all 15 bits of d - 1)
    for k in range(1, 16):
        assert stage_starts(raw32, 32768 + k, start=32768) == [32768]
    assert read_blocks(raw32)[0].type == 0 and read_blocks(raw32)[0].b1 == 32768
    assert tokens_of(raw32)[0][0] == 32768 and tokens_of(raw32)[0][2] > 4096
    _, raws, _ = gz(short_room_payload)
    assert len(read_blocks(raws)) == 1
    for n in SHORT_ROOM:
        ss = stage_starts(raws, n)
        assert ss == [0, 4079] and 1 <= n - ss[-1] <= 15, (n, ss)
    # ... and the short stage starts with a match, whose source lies before it
    assert any(ln >= 15 and pos == 4079 for pos, ln, _ in tokens_of(raws))
    # 3. the edge payloads are one Huffman block each, so that the stage rule alone cuts them
    for p in edge_payloads():
        assert [b.type != 0 for b in read_blocks(deflate(p, 6))] == [True]
        assert [b.type != 0 for b in read_blocks(deflate(p[5:], 6))] == [True]
    # 4. one round cannot cover the block: a body of more than 64 segments of IW_SEGMAX bits ...
    raw = deflate(c2_256k(), 6, mem=9)
    bodies = []
    br = Bits(raw)
    last = 0
    while not last:
        last, lt, dt = read_header(br)
        p0 = br.p
        while token(br, lt, dt) != 256:
            pass
        bodies.append(br.p - p0)
    assert max(bodies) > 64 * IW_SEGMAX, bodies
    # ... and lists that fill (IW_TCAP tokens) well inside the first segment of a block of many more tokens
    raw = deflate(_three_symbols(), 6, zlib.Z_HUFFMAN_ONLY, 9)
    tb, _ = token_bits(raw)
    assert len(tb) > 8 * IW_TCAP and tb[IW_TCAP][0] - tb[0][0] < SEG0 // 2, (len(tb), tb[IW_TCAP][0] - tb[0][0])
    # 5. the look-ahead sizes: token boundaries inside a Huffman block, a full stage behind them
    _, b, n_match, n_eob = lookahead_cases()
    starts = [pos for pos, _, _ in b.tokens]
    assert n_match in starts and n_match - b.b0 > CAP_WIDE and n_eob == b.b1 and n_eob - b.b0 > CAP_WIDE
    # 6. the faults sit more than 2 048 bytes into a stage: the first stage, then the second
    for k, (_, n, kind, at, raw) in enumerate(status_cases()):
        ss = stage_starts(raw, n)
        mine = max(s for s in ss if s <= at)
        assert at - mine >= 2048 and ss.index(mine) == k // 2, (k, at, ss)


# ---- on the GPU ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u1", "<f4"])
def test_near_distances_of_the_larger_ring(dt):
    p, _, s = gz(near_payload)
    check([s], dt, len(p) // dtype_info(dt)[0], want=["ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [">f4", ">i2"])
def test_swapped_stages_keep_wide_distances(dt):
    p, _, s = gz(near_payload)
    check([s], dt, len(p) // dtype_info(dt)[0], want=["ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [">f4", "<f4"])
def test_distance_32768(dt):
    p, _, s = far32k()
    check([s], dt, len(p) // 4, want=["ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 16))
def test_short_room_stage_at_distance_32768(k):
    """N = 32 768 + k: the stage behind the stored block has k < 16 bytes of
    room and reads its match's source 32 768 bytes back, byte by byte: the
    near descriptor needs 15 bits for d - 1 (the 12 / 12 split of a wide stage
    would cut it)."""
    _, _, s = far32k()
    check([s], "u1", 32768 + k, want=["ok"])
    if k % 4 == 0:
        check([s], "<f4", (32768 + k) // 4, want=["ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHORT_ROOM)
def test_short_room_last_stage(n):
    _, _, s = gz(short_room_payload)
    check([s], "u1", n, want=["ok"])
    if n % 4 == 0:
        check([s], "<f4", n // 4, want=["ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_stage_edges(n):
    ss = edge_streams()
    check(ss[:2], "u1", n, want=["ok", "ok"])
    check(ss[2:], "u1", n + 5, want=["ok", "ok"])  # the same offsets from ring entry 5


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4081, 8145, 20000])
def test_stored_blocks_longer_than_a_stage(n):
    check([stored_member()], "u1", n, want=["ok"])


@pytest.mark.gpu
def test_table_reload_before_a_further_round():
    c2, tri = c2_256k(), _three_symbols()
    s1 = gzip_wrap(deflate(c2, 6, mem=9), c2)
    s2 = gzip_wrap(deflate(tri, 6, zlib.Z_HUFFMAN_ONLY, 9), tri)
    check([s1], "<f4", len(c2) // 4, want=["ok"])
    check([s2], "u1", len(tri), want=["ok"])
    # 64 chunks in one launch: every slot saves and reloads its own tables
    kinds, outs = oracle("gzip", [s1], "<f4", len(c2) // 4)
    check([s1] * 64, "<f4", len(c2) // 4, ref=(kinds * 64, outs * 64))
    kinds, outs = oracle("gzip", [s2], "u1", len(tri))
    check([s2] * 64, "u1", len(tri), ref=(kinds * 64, outs * 64))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["match", "eob"])
def test_table_reload_before_the_lookahead(which):
    s, _, n_match, n_eob = lookahead_cases()
    n = n_match if which == "match" else n_eob
    check([s], "u1", n, want=["ok"])
    check([s], "u1", n - 1, want=["ok"])


@pytest.mark.gpu
def test_status_late_in_a_stage():
    for s, n, kind, _, _ in status_cases():
        check([s], "u1", n, want=[kind])
