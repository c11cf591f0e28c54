"""The gzip member frame the three inflate kernels share (zcg_inflate_common.h):
open (guards, flate2's header rules), block headers, stored blocks through a
kernel's stage, and close (zlib's post-N look-ahead, result -> status).

Every stream goes through the default dispatch, FLAG_SERIAL_INFLATE,
FLAG_INFLATE_BLOCK_PAR and FLAG_INFLATE_WAVE, one batch launch per flag set
per group of streams; status and bytes must equal the oracle's, and the bytes
after N in the caller's buffer must stay untouched.  Each case first asserts
that the oracle's own answer is the one it is there for.  All streams are
<= 60 KB.
"""
import struct
import zlib

import numpy as np
import pytest

from deflate_kit import PLAIN_HEADER, stored, text, trailer
from golden_util import dtype_info
from gpu_check import GUARD, check_many
from zarr_amd import _native

pytestmark = pytest.mark.gpu

FLAG_SETS = (0, _native.FLAG_SERIAL_INFLATE, _native.FLAG_INFLATE_BLOCK_PAR, _native.FLAG_INFLATE_WAVE)


def check_group(streams, dt, n, want):
    """`want`: the oracle's answer for each stream (checked first).  Then one
    launch per flag set: oracle parity of status and bytes, guard intact."""
    check_many("gzip", streams, dt, n, FLAG_SETS, guard=GUARD, want=want)


# ---- 1. stored blocks ---------------------------------------------------------------------------
STORED_SIZES = [2031, 1, 2033, 0, 16383, 17, 4096, 0, 15439]


@pytest.fixture(scope="module")
def stored_member():
    payload = np.random.default_rng(4001).integers(0, 256, 40000).astype(np.uint8).tobytes()
    assert sum(STORED_SIZES) == len(payload)
    raw, at = b"", 0
    for i, k in enumerate(STORED_SIZES):
        raw += stored(payload[at:at + k], last=i == len(STORED_SIZES) - 1)
        at += k
    return PLAIN_HEADER + raw + trailer(payload)


@pytest.mark.parametrize("n", [1, 2031, 2032, 2033, 4065, 16384, 20448, 20465, 24561, 40000])
def test_stored_blocks(stored_member, n):
    """Blocks around the wave kernel's stage piece (2 032 bytes) and the
    256-lane kernel's stage (16 384), empty blocks, and N at block ends
    (2 031, 2 032, 4 065, 20 448, 20 465, 24 561, 40 000): there the look-ahead
    reads the next stored header."""
    check_group([stored_member], "u1", n, ["Ok"])


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_stored_blocks_swapped_and_bool(stored_member, dt):
    check_group([stored_member], dt, 40000 // dtype_info(dt)[0], ["Ok"])


# ---- 2. look-ahead after a stored block ---------------------------------------------------
def test_lookahead_after_stored_block():
    """N = 3 000 fills the output exactly at the end of a non-final stored
    block, so zlib goes on to the next header: four tails it must reject and
    one it accepts.  At N = 2 999 the output fills inside the block and nothing
    after it is looked at."""
    head = np.random.default_rng(4005).integers(0, 256, 3000).astype(np.uint8).tobytes()
    assert (zlib.crc32(head) >> 1) & 3 == 3  # (the bare trailer's first bits read as BTYPE 3)
    more = text(2000, 4003)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    tails = [
        (bytes([0x06]), b""),                                        # type-3 header
        (bytes([0x00]) + struct.pack("<HH", 5, 5) + b"abcde", b""),  # LEN / NLEN mismatch
        (b"", b""),                                                  # nothing: the trailer is read as a header
        (stored(b"") + bytes([0x06]), b""),                          # empty stored block, then type 3
        (c.compress(more) + c.flush(), more),                        # a valid zlib-6 block
    ]
    streams = [PLAIN_HEADER + stored(head) + raw + trailer(head + pay) for raw, pay in tails]
    check_group(streams, "u1", 3000, ["InvalidData"] * 4 + ["Ok"])
    check_group(streams, "u1", 2999, ["Ok"] * 5)


# ---- 3. sync flushes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sync_member():
    payload = text(60000, 4004)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b""
    for at in range(0, len(payload), 7000):
        raw += c.compress(payload[at:at + 7000]) + c.flush(zlib.Z_SYNC_FLUSH)
    raw += c.flush()
    s = PLAIN_HEADER + raw + trailer(payload)
    assert len(s) <= 60000
    return s


@pytest.mark.parametrize("n", [7000, 7001, 14000, 60000])
def test_sync_flushes(sync_member, n):
    """Every 7 000 bytes a Huffman block ends and an empty stored block
    follows: N at such a seam, one past it, and the whole member."""
    check_group([sync_member], "u1", n, ["Ok"])


# ---- 4. gzip header fields --------------------------------------------------------------------
def test_gzip_header_fields():
    payload = text(5000, 4005)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(payload) + c.flush()
    extra = b"ZA\x04\x00frme"
    h = bytes([0x1f, 0x8b, 8, 0x02 | 0x04 | 0x08 | 0x10, 1, 2, 3, 4, 0, 3])
    h += struct.pack("<H", len(extra)) + extra + b"chunk.bin\x00" + b"a comment\x00"
    crc16 = zlib.crc32(h) & 0xFFFF
    good = h + struct.pack("<H", crc16) + raw + trailer(payload)
    bad_crc = h + struct.pack("<H", (crc16 + 1) & 0xFFFF) + raw + trailer(payload)
    cm7 = bytearray(good)
    cm7[2] = 7
    check_group([good, bad_crc, good[:14], bytes(cm7)], "u1", len(payload),
                ["Ok", "InvalidData", "UnexpectedEof", "InvalidData"])
