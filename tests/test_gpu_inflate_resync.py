"""The one-wave-per-chunk inflate kernel's resync: a lane that has left its
segment follows its path until it meets a token start the next lane marked,
and the sync token's rank in that lane's list is counted from the mark words
for all synced lanes at once after the loop.

Every stream is decoded through the default dispatch and through
FLAG_INFLATE_WAVE, each with and without FLAG_DEBUG_INFLATE_LONG_SEG, in one
batch launch per flag set; status and bytes must equal the oracle's, and the
bytes after N in the caller's buffer must stay untouched.  Streams come from
the system zlib.  The property the cases are there for is the resync distance
at the first block's segment boundaries: the kernel's first-round segment rule
is restated here, a small deflate decoder follows the path from each segment
start and the path of its predecessor, and the distance is where the two first
share a token start.
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

# the kernel's first-round rule (zcg_inflate_wave.hip): IW_EST0 = 64 * 3072 bits
# estimated for the first block's body, 108 %, 64 lanes, rounded up to 32 bits
IW_EST0 = 64 * 3072
SEG = ((IW_EST0 * 108 // 100 // 64) + 31) & ~31
MARKED = 32 * 32  # IW_MARKW words of token-start marks are kept per segment
assert SEG == 3328


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


# ---- a small deflate decoder over a list of bits: headers, and token paths from any bit ----
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def bit_list(raw):
    return np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little").tolist() + [0] * 64


def take(bits, p, n):
    x = 0
    for i in range(n):
        x |= bits[p + i] << i
    return x, p + n


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


def sym(bits, p, table):
    """(symbol, bit after its code); None for a bit pattern that is no code."""
    c = 0
    for l in range(1, 16):
        c = (c << 1) | bits[p + l - 1]
        if (l, c) in table:
            return table[(l, c)], p + l
    return None, p


def read_header(bits, p):
    """Block header at bit p: (last, literal/length table, distance table, first body bit)."""
    last, p = take(bits, p, 1)
    ty, p = take(bits, p, 2)
    assert ty in (1, 2), ty
    if ty == 1:
        hl, ls = 288, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 30
    else:
        hl, p = take(bits, p, 5)
        hd, p = take(bits, p, 5)
        hc, p = take(bits, p, 4)
        hl, hd, hc = hl + 257, hd + 1, hc + 4
        cl = [0] * 19
        for i in range(hc):
            cl[CLEN_ORDER[i]], p = take(bits, p, 3)
        ct, ls = canon(cl), []
        while len(ls) < hl + hd:
            s, p = sym(bits, p, ct)
            if s < 16:
                ls.append(s)
            else:
                n, p = take(bits, p, (2, 3, 7)[s - 16])
                ls += [ls[-1]] * (3 + n) if s == 16 else [0] * ((3, 11)[s - 17] + n)
    return last, canon(ls[:hl]), canon(ls[hl:]), p


def token(bits, p, lt, dt):
    """One token from bit p, as a decoder that believes a token starts there
    takes it: (symbol, bit after the token); (None, p) where the bits are no code."""
    s, e = sym(bits, p, lt)
    if s is None or s <= 256:
        return s, e
    if s > 285:
        return None, p
    e += LEN_EXTRA[s - 257]
    d, e = sym(bits, e, dt)
    if d is None or d > 29:
        return None, p
    return s, e + DIST_EXTRA[d]


def first_block(raw):
    """(bits, tables, body start, bit of the end-of-block code, token count) of the first block."""
    bits = bit_list(raw)
    _, lt, dt, body = read_header(bits, 0)
    p, n = body, 0
    while True:
        s, e = token(bits, p, lt, dt)
        assert s is not None
        if s == 256:
            return bits, lt, dt, body, p, n
        p, n = e, n + 1


def resync_distances(raw, limit=MARKED):
    """For every boundary between two first-round segments that lie inside the
    first block: bits from the boundary to the first token start that the path
    from the boundary (a decoder started there) shares with the path of the
    segment before it (a decoder started at that segment's first bit); None
    when they share none within `limit` bits."""
    bits, lt, dt, body, eob, _ = first_block(raw)

    def path(p, stop):
        starts = []
        while p < stop:
            starts.append(p)
            s, e = token(bits, p, lt, dt)
            if s is None:
                break
            p = e
        return starts

    out = []
    k = 1
    while body + (k + 1) * SEG <= eob:
        b = body + k * SEG
        mine = set(path(b, b + limit))
        join = next((x for x in path(b - SEG, b + limit) if x >= b and x in mine), None)
        out.append(None if join is None else join - b)
        k += 1
    return out


# ---- payloads (built once) ---------------------------------------------------------------
def quant_chunk(idx):
    """bench.py's C2 "quant" chunk: round(64 (100 sin(0.05 (i + 7 idx)) cos(0.03 j) + k)) / 64 as <f4."""
    i = np.arange(256, dtype=np.float64)[:, None, None]
    j = np.arange(256, dtype=np.float64)[None, :, None]
    k = np.arange(4, dtype=np.float64)[None, None, :]
    v = np.round(64 * (100 * np.sin(0.05 * (i + idx * 7)) * np.cos(0.03 * j) + k)) / 64
    return v.astype("<f4").reshape(-1)


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


def _randwalk_i2():
    return np.cumsum(np.random.default_rng(0).integers(-3, 4, 64 << 10)).astype("<i2").tobytes()


@pytest.fixture(scope="module")
def quant():
    """[(payload, raw deflate, gzip stream)] of the first 192 KiB of C2 chunks 0 and 1."""
    out = []
    for idx in (0, 1):
        payload = quant_chunk(idx).tobytes()[: 192 << 10]
        raw = deflate(payload, 6)
        out.append((payload, raw, gzip_wrap(raw, payload)))
    return out


def test_sync_in_each_storage_class(quant):
    """Syncs inside the two early mark words (kept in LDS), within the next
    eight words and further on (ranks counted over 1-2, up to 10 and up to 32
    mark words): the first block of each payload has boundaries of all three
    kinds and none beyond the marked zone."""
    for payload, raw, s in quant:
        d = resync_distances(raw)
        assert len(d) >= 32, len(d)
        assert all(x is not None and x < MARKED for x in d), d
        assert any(x < 64 for x in d) and any(64 <= x < 320 for x in d) and any(320 <= x < MARKED for x in d), d
    n = (192 << 10) // 4
    st = check_batch([q[2] for q in quant], "<f4", n)
    assert (st == zref.OK).all()


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_swapped_and_bool_dtypes(quant, dt):
    es = dtype_info(dt)[0]
    st = check_batch([q[2] for q in quant], dt, (192 << 10) // es)
    assert (st == zref.OK).all()


def test_paths_that_cross_whole_segments():
    """Small blocks (memLevel 1: ~127 tokens each, segments at IW_SEGMIN, never
    past the kept zone): pass 2 crosses whole segments, so the synced segment
    is not the lane's neighbour; in one batch with memLevel 4 and 9, at levels
    1, 6 and 9."""
    payload = _skewed_with_copies()[: 32 << 10]
    bits = bit_list(deflate(payload, 6, mem=1))
    p, nblk, most = 0, 0, 0
    while True:
        last, lt, dt, p = read_header(bits, p)
        n = 0
        while True:
            s, p = token(bits, p, lt, dt)
            assert s is not None
            if s == 256:
                break
            n += 1
        nblk, most = nblk + 1, max(most, n)
        if last:
            break
    assert nblk >= 100 and most <= 128, (nblk, most)
    streams = [gzip_wrap(deflate(payload, lv, mem=mem), payload) for mem in (1, 4, 9) for lv in (1, 6, 9)]
    st = check_batch(streams, "u1", len(payload))
    assert (st == zref.OK).all()


def test_full_list_while_resyncing():
    """~1.1 bits per token (three symbols, Huffman only): every list caps, so
    lanes stop on the cap with no sync and no rank; and the all-literal
    random-walk i16 payload whose capped chains halve the segment size."""
    p3 = _three_symbols()
    raw = deflate(p3, 6, zlib.Z_HUFFMAN_ONLY)
    bits, lt, dt, body, eob, ntok = first_block(raw)
    assert (eob - body) / ntok < 1.3 and ntok * 4096 // (eob - body) > 3000, ((eob - body) / ntok)
    st = check_batch([gzip_wrap(raw, p3)], "u1", len(p3))
    assert st[0] == zref.OK
    rwp = _randwalk_i2()
    raw = deflate(rwp, 6, zlib.Z_HUFFMAN_ONLY)
    st = check_batch([gzip_wrap(raw, rwp)], "u1", len(rwp))
    assert st[0] == zref.OK


def test_stream_end_while_resyncing(quant):
    """Cut at each of the last 48 bytes and at 16 interior points: lanes near
    the stream end stop on the input-exhausted marker, in their segment or on
    the way to a sync, and the statuses are the oracle's."""
    payload, raw, s = quant[0]
    cuts = [len(s) - k for k in range(1, 49)] + [len(s) * k // 18 for k in range(1, 17)]
    st = check_batch([s[:c] for c in cuts], "u1", len(payload))
    assert (st != zref.OK).sum() >= 48 - 8  # (the last cuts fall in the 8-byte gzip trailer)


def test_path_passes_the_marked_extent():
    """64 equally likely byte values, Huffman only: every code has 6 bits, so a
    misaligned path never meets the true one.  Lanes run past the 1 024
    marked bits of the next segment and cross whole segments to the round's
    end, or sync several segments on."""
    payload = np.random.default_rng(11).integers(0, 64, 64 << 10, dtype=np.uint8).tobytes()
    raw = deflate(payload, 6, zlib.Z_HUFFMAN_ONLY)
    d = resync_distances(raw)
    assert len(d) >= 16 and any(x is None for x in d), d
    st = check_batch([gzip_wrap(raw, payload)], "u1", len(payload))
    assert st[0] == zref.OK


def test_many_waves_per_cu(quant):
    """64 copies of one stream in one launch: several waves stay resident per
    SIMD, so the resync loops of different chunks interleave there."""
    payload, raw, s = quant[0]
    st = check_batch([s] * 64, "u1", len(payload))
    assert (st == zref.OK).all()
