"""Directed block-level bzip2 streams on the GPU (zcg_bz2.hip) against the
oracle, bit-exact.

Every stream in tests/test_gpu_bzip2.py comes from libbz2's encoder, which
never sets the randomised bit, never leaves a run of four without its count
byte (`tail4`), always writes a one-cycle L / origPtr pair, fills its blocks
and, written at the metadata's level, never has more blocks than the
launcher has rounds.  tests/bz2_craft.py writes the streams that reach the
rest: the randomised branch, `tail4`, the serial walk of a chain that is not
one cycle, blocks of pinned size, the whole-stream kernel that finishes what
the rounds leave open, and the tables libbz2 never builds for stage A's
device IO.  The writer is pinned against libbz2 on the CPU
(tests/test_bz2_craft_host.py), where the host core decodes the same cases.

A batch has one D, so a case that wants its own D is decoded behind a filler
block (Case.at): the decode then ends at the same place of the same block.
"""
import bz2

import pytest

import bz2_cases as cs
import bz2_craft as bc
from gpu_check import check_many, rw

pytestmark = pytest.mark.gpu


def batch(name, **kw):
    cases, D = cs.gpu_batches()[name]
    check_many("bzip2", [c.at(D) for c in cases], "u1", D, **kw)


def test_ladder_content():
    """nblock 1..4097 across the wave-quarter, sample-stride and per-thread
    segment boundaries, four alphabets, randomised and not, D at, past,
    before and inside the block."""
    batch("content")
    batch("content_big")


@pytest.mark.parametrize("kind", cs.ALPHABETS)
def test_ladder_raw(kind):
    """Chains that are not one cycle (the serial walk; a third of the cases
    reach D before the CRC check, tests/test_bz2_craft_host.py pins the
    count per batch) and origPtr at and past nblock."""
    batch("raw-" + kind)
    batch("raw_big-" + kind)


def test_randomised_blocks():
    streams, D = cs.randomised_streams()
    for level in (1, 9):  # at level 9 there are 3 rounds: the whole-stream kernel decodes the rest
        check_many("bzip2", streams, "u1", D, param=level)


def test_tail4():
    """A block that ends in a run of four: the count is the cycle's first
    byte, XOR the schedule's mask of chain position nblock when the block is
    randomised (nblock 617 and 1337 are such positions)."""
    batch("tail4")


# ---- the whole-stream kernel ---------------------------------------------------
def test_whole_stream_kernel_small_blocks():
    streams, D, blocks = cs.fallback_streams()
    assert blocks > bc.decode_rounds(D, 9)
    check_many("bzip2", streams[:1], "u1", D, param=9)


def test_whole_stream_kernel_level1_stream_under_level9():
    payload = rw(750000, seed=11).tobytes()
    s = bz2.compress(payload, 1)
    assert bc.count_blocks(s) > bc.decode_rounds(len(payload), 9)
    check_many("bzip2", [s], "u1", len(payload), param=9)


def test_whole_stream_kernel_mixed_batch():
    streams, D, blocks = cs.fallback_streams()
    assert blocks > bc.decode_rounds(D, 9)
    one = cs.norun_bytes(D, seed=1)
    short = [bc.write_stream([bc.Block(T=one, randomised=1)], level=2)[0], bz2.compress(one, 2),
             bc.write_stream([bc.Block(T=one[:D // 2]), bc.Block(T=one[D // 2:])])[0]]
    for s in short:
        assert bc.count_blocks(s) + 1 <= bc.decode_rounds(D, 9)
    mixed = []
    for i in range(24):
        mixed.append(streams[0] if i % 3 == 0 else short[i % 3] if i % 2 else short[0])
    check_many("bzip2", mixed, "u1", D, param=9)


def test_whole_stream_kernel_errors_and_short_output():
    """Past the rounds: a wrong block CRC, a cut stream, D inside a block."""
    streams, D, blocks = cs.fallback_streams()
    assert blocks > bc.decode_rounds(D, 9) and 21 > bc.decode_rounds(D, 9)
    check_many("bzip2", streams, "u1", D, param=9)


@pytest.mark.parametrize("dt", [">i2", "bool"])
def test_whole_stream_kernel_transform(dt):
    from golden_util import dtype_info
    streams, D, blocks = cs.fallback_streams()
    es = dtype_info(dt)[0]
    assert blocks > bc.decode_rounds(D, 9) and D % es == 0
    check_many("bzip2", streams, dt, D // es, param=9)


@pytest.mark.parametrize("level", [1, 9])
def test_sampling_edges(level):
    batch("sampling", param=level)


def test_stage_a_device_io():
    """2..6 groups, equal code lengths of 8, 9, 17 and 20, real Huffman
    lengths, every table order, surplus selectors (past 18 002 too), all
    256 bytes in the symbol map, MTF depth 255 on every symbol, zero runs
    of 1..70 and 255..260 across L's 4- and 64-byte offsets, and the
    invalid group counts."""
    batch("stage_a")


def test_empty_garbage_and_doubled_streams():
    """The bare empty stream (header and end record only, with and without
    bytes after it) goes into the batch as it is; the other shapes stand
    behind a filler block."""
    cases, D = cs.gpu_batches()["shapes"]
    empty = bc.write_stream([])[0]
    assert len(empty) == 14 and sum(c.at(D).startswith(empty) for c in cases) == 3
    batch("shapes")
