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
import zlib

import numpy as np
import pytest

from deflate_kit import (Bits, _skewed_with_copies, _three_symbols, block_tokens, deflate, gzip_wrap, read_header,
                         token)
from golden_util import dtype_info
from gpu_check import GUARD, check_many
from zarr_amd import _native

pytestmark = pytest.mark.gpu

FLAG_SETS = (0, _native.FLAG_INFLATE_WAVE, _native.FLAG_DEBUG_INFLATE_LONG_SEG,
             _native.FLAG_INFLATE_WAVE | _native.FLAG_DEBUG_INFLATE_LONG_SEG)

# the kernel's first-round rule (zcg_inflate_wave.hip): IW_EST0 = 64 * 3072 bits
# estimated for the first block's body, 108 %, 64 lanes, rounded up to 32 bits
IW_EST0 = 64 * 3072
SEG = ((IW_EST0 * 108 // 100 // 64) + 31) & ~31
MARKED = 32 * 32  # IW_MARKW words of token-start marks are kept per segment
assert SEG == 3328


def check_batch(streams, dt, n):
    """One launch per flag set: oracle parity of status and bytes, guard intact."""
    return check_many("gzip", streams, dt, n, FLAG_SETS, guard=GUARD)


# ---- token paths from any bit (deflate_kit's reader) ---------------------------------------
def first_block(raw):
    """(reader, tables, body start, bit of the end-of-block code, token count) of the first block."""
    br = Bits(raw)
    _, lt, dt = read_header(br)
    body = br.p
    n, eob = block_tokens(br, lt, dt)
    return br, lt, dt, body, eob, n


def resync_distances(raw, limit=MARKED):
    """For every boundary between two first-round segments that lie inside the
    first block: bits from the boundary to the first token start that the path
    from the boundary (a decoder started there) shares with the path of the
    segment before it (a decoder started at that segment's first bit); None
    when they share none within `limit` bits."""
    br, lt, dt, body, eob, _ = first_block(raw)

    def path(p, stop):
        starts, br.p = [], p
        while br.p < stop:
            starts.append(br.p)
            if token(br, lt, dt) is None:
                break
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
    assert set(st) == {"Ok"}


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_swapped_and_bool_dtypes(quant, dt):
    es = dtype_info(dt)[0]
    st = check_batch([q[2] for q in quant], dt, (192 << 10) // es)
    assert set(st) == {"Ok"}


def test_paths_that_cross_whole_segments():
    """Small blocks (memLevel 1: ~127 tokens each, segments at IW_SEGMIN, never
    past the kept zone): pass 2 crosses whole segments, so the synced segment
    is not the lane's neighbour; in one batch with memLevel 4 and 9, at levels
    1, 6 and 9."""
    payload = _skewed_with_copies()[: 32 << 10]
    br = Bits(deflate(payload, 6, mem=1))
    nblk, most, last = 0, 0, 0
    while not last:
        last, lt, dt = read_header(br)
        nblk, most = nblk + 1, max(most, block_tokens(br, lt, dt)[0])
    assert nblk >= 100 and most <= 128, (nblk, most)
    streams = [gzip_wrap(deflate(payload, lv, mem=mem), payload) for mem in (1, 4, 9) for lv in (1, 6, 9)]
    st = check_batch(streams, "u1", len(payload))
    assert set(st) == {"Ok"}


def test_full_list_while_resyncing():
    """~1.1 bits per token (three symbols, Huffman only): every list caps, so
    lanes stop on the cap with no sync and no rank; and the all-literal
    random-walk i16 payload whose capped chains halve the segment size."""
    p3 = _three_symbols()
    raw = deflate(p3, 6, zlib.Z_HUFFMAN_ONLY)
    _, lt, dt, body, eob, ntok = first_block(raw)
    assert (eob - body) / ntok < 1.3 and ntok * 4096 // (eob - body) > 3000, ((eob - body) / ntok)
    st = check_batch([gzip_wrap(raw, p3)], "u1", len(p3))
    assert st[0] == "Ok"
    rwp = _randwalk_i2()
    raw = deflate(rwp, 6, zlib.Z_HUFFMAN_ONLY)
    st = check_batch([gzip_wrap(raw, rwp)], "u1", len(rwp))
    assert st[0] == "Ok"


def test_stream_end_while_resyncing(quant):
    """Cut at each of the last 48 bytes and at 16 interior points: lanes near
    the stream end stop on the input-exhausted marker, in their segment or on
    the way to a sync, and the statuses are the oracle's."""
    payload, raw, s = quant[0]
    cuts = [len(s) - k for k in range(1, 49)] + [len(s) * k // 18 for k in range(1, 17)]
    st = check_batch([s[:c] for c in cuts], "u1", len(payload))
    assert sum(k != "Ok" for k in st) >= 48 - 8  # (the last cuts fall in the 8-byte gzip trailer)


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
    assert st[0] == "Ok"


def test_many_waves_per_cu(quant):
    """64 copies of one stream in one launch: several waves stay resident per
    SIMD, so the resync loops of different chunks interleave there."""
    payload, raw, s = quant[0]
    st = check_batch([s] * 64, "u1", len(payload))
    assert set(st) == {"Ok"}
