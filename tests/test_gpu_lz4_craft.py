"""Directed sequence-level LZ4 frames on the GPU (zcg_lz4_dec.hip) against the
oracle, bit-exact.

Every other LZ4 stream of the suite comes from liblz4's encoder, which never
writes offset 0, stops its matches 12 bytes before the end of a full block,
stores incompressible blocks raw and takes the offsets and lengths the data
offers.  tests/lz4_craft.py writes frames sequence by sequence and
tests/lz4_cases.py holds the tables; tests/test_lz4_craft_host.py pins them
against the reference decoder and a plain model on the CPU.  Each batch runs
through the default pick, the wave-per-block kernel (lz4_block_wave,
FLAG_LZ4_WAVE_PER_BLOCK) and the lane-per-block kernel (lz4_lane_block with
LaneRing, FLAG_LZ4_LANE_PER_BLOCK); frames
the block placement cannot serve (linked, short block in mid-frame, early
end) reach the serial lz4_block under every flag.  Per stream: the status
kind is the oracle's, Ok chunks have the oracle's bytes, and the 0xAB guard
behind the D decoded bytes is intact whatever the status.

What each family is there for, by the constant or table it pins (move the
lists in tests/lz4_cases.py when one of them changes):

  A  the input side: literal and match lengths around the nibble (14/15/16),
     one and two length bytes (269/270/271, 525), LZ_ROUND and LZ_RING
     (1023..1025, 2047..2049), with the token at every block offset 0..63
     (LzBuf's 16-byte phases and 64-byte reloads; every lane of the wave
     window), and chains of 14..20 length bytes that leave the 16-byte
     register window: lz4_seq_at's B(), LzWin::byte, LzBuf::at up to d = 48.
  B  the wave window (64 stream bytes, at most 32 sequences a step): 25 and 30
     three-byte sequences back to back, a successor at window offset 63, 64
     and 65, literals across the window end (c >= 64), the final sequence
     first and last in a window, and LZ_LIGHT: totals of 32 stay on the
     byte-parallel path, one total of 33 sends the whole step down the heavy
     path.
  C1 offset 0 (zeros) and every row of c_lz_pat (offsets 1..15), each at match
     lengths around 16 and 32 (append16's pieces; lz4_block's two pattern16
     stores and its d2 loop) and at the LZ_LRB = 128 ring phases around the
     mirror (0, 1, 15, 16, 17), the middle and the wrap (111, 112, 113, 127).
  C2 offsets around 16, 32, 64 and LZ_LRB (123..129), and every offset
     90..100 around LZ_NEAR = 96 at all 128 ring phases: the ring serves the
     nearer ones, the block's own output in HBM the others.
  C3 offsets around LZ_RING = 2048 from a source the step before wrote (HBM
     behind need_visible's fence), every offset 1900..2049 against light and
     heavy steps (`src + LZ_RING >= rb + rn`), 4095, 65535 (a 256 KiB block),
     and offset == position (legal) against position + 1 (invalid) in the
     first and in a later block.
  C4 pointers to pointers in the LDS ring: matches that copy from matches
     within one window, ml >= off and ml < off, and overlapping matches.
  D  heavy rounds of LZ_ROUND = 1024: one sequence of 1024, 1025, 2048, 2049
     and 3073 bytes, as literals, as the final literals and as a match at
     offsets inside and outside a round and the ring.
  E  the block end at capacity (64 KiB and 256 KiB blocks): a match may end at
     cap - 5 and start at cap - 12 and no later; literals may end at cap.
  F  the block size word against the content, and the block cut at every
     byte: iend inside the token, the length bytes, the literals, the offset.
  G  the serial lz4_block (off 0; off < 16 with ml <= 32 and > 32; off >= 16;
     literals of at most 16 in and out of the window) behind a short first
     block (low = out) and in linked frames (low = 0), matches that reach
     the frame's first bytes, frames that end before D (the suffix checks),
     and stored blocks among compressed ones.
  H  D inside a block: lim at the 16- and 32-byte fast-path guards of
     lz4_block (the linked copies), at finish()'s `p + 4 <= lim` and at
     LZ_LPC = 64-byte pieces.

Nothing here is meant to fault: the invalid cases are streams the kernels'
own checks reject with a status.
"""
import numpy as np
import pytest

import lz4_cases as cs
import lz4_craft as lc
from golden_util import dtype_info
from gpu_check import GUARD, check_many, oracle
from zarr_amd import _native

pytestmark = pytest.mark.gpu

WAVE, LANE = _native.FLAG_LZ4_WAVE_PER_BLOCK, _native.FLAG_LZ4_LANE_PER_BLOCK
FLAGS = [0, WAVE, LANE]


def check(streams, D, flags, dt="u1", want=None):
    """One batch under one flag set; want: the kinds the table names (the
    oracle's, asked once per batch, must equal them)."""
    es = dtype_info(dt)[0]
    assert D % es == 0
    check_many("lz4", streams, dt, D // es, flags, guard=GUARD, want=want, cache=True)


def family_batches(family, valid):
    got = [(name, D, cases) for name, (D, cases) in cs.batches().items()
           if cases[0].family == family and (cases[0].want == "ok") == valid]
    assert got, family
    return got


@pytest.mark.parametrize("flags", FLAGS, ids=["default", "wave", "lane"])
@pytest.mark.parametrize("family", ["A", "B", "C1", "C2", "C3", "C4", "D", "E", "F", "G", "H"])
def test_valid_family(family, flags):
    for name, D, cases in family_batches(family, True):
        check([c.frame for c in cases], D, flags, want=[c.want for c in cases])


@pytest.mark.parametrize("flags", FLAGS, ids=["default", "wave", "lane"])
@pytest.mark.parametrize("family", ["C3", "E", "F", "G"])
def test_rejected_family(family, flags):
    """Offsets before the block or frame start, matches and literals past the
    last legal byte of a full block, cut blocks, frames that end early."""
    for name, D, cases in family_batches(family, False):
        check([c.frame for c in cases], D, flags, want=[c.want for c in cases])


@pytest.mark.parametrize("flags", [LANE, WAVE], ids=["lane", "wave"])
def test_all_valid_cases_of_one_size_shuffled(flags):
    """Every valid case of families A to D in one batch, in random order: the
    64 lanes of a wave of the lane kernel hold 64 different blocks on
    different paths."""
    cases = [c for c in cs.all_cases() if c.D == cs.MAIN and c.want == "ok"]
    assert len(cases) == 215
    order = np.random.default_rng(17).permutation(len(cases))
    check([cases[i].frame for i in order], cs.MAIN, flags, want=["ok"] * len(cases))


@pytest.mark.parametrize("want", ["ok", "invalid"])
@pytest.mark.parametrize("dt", [">u2", "bool"])
def test_element_transform(dt, want):
    """Families C and E through the element transform of the finish kernel
    (rejected chunks keep their status and their guard)."""
    for fams, D in (({"C1", "C2", "C3", "C4"}, cs.MAIN), ({"E"}, cs.CAP)):
        cases = [c for c in cs.all_cases() if c.family in fams and c.D == D and c.want == want]
        counts = {("ok", cs.MAIN): 57, ("invalid", cs.MAIN): 6, ("ok", cs.CAP): 6, ("invalid", cs.CAP): 10}
        assert len(cases) == counts[want, D]
        check([c.frame for c in cases], D, 0, dt=dt, want=[want] * len(cases))


def flip_literal(c, frame):
    """`frame` with one bit of one literal flipped (the longest literal run of
    the case: its bytes stand once in the frame)."""
    lits = [s[0] for b in c.blocks if not (isinstance(b, tuple) and b[0] == "stored") for s in b]
    lit = max(lits, key=len)
    assert len(lit) >= 12 and frame.count(lit) == 1
    i = frame.index(lit) + len(lit) // 2
    return frame[:i] + bytes([frame[i] ^ 1]) + frame[i + 1:]


def test_content_checksum_verification():
    """Crafted frames with a content checksum under ZCG_FLAG_VERIFY_LZ4_CONTENT:
    the valid ones stay Ok, a copy with one literal flipped (Ok to the
    oracle, which does not read the checksum) becomes InvalidData."""
    for batch in ("G", "E", "C4"):
        D, cases = cs.batches()[batch]
        good = [lc.frame(c.blocks, linked=c.linked, content_checksum=True) for c in cases]
        bad = [flip_literal(c, f) for c, f in zip(cases, good)]
        streams = good + bad
        ref = oracle("lz4", streams, "u1", D, cache=True)
        assert ref[0] == ["Ok"] * len(streams)
        for c, o in zip(cases, ref[1]):
            assert o == lc.model(c.blocks, c.linked)[:D]
        check_many("lz4", streams, "u1", D, [f | _native.FLAG_VERIFY for f in FLAGS], guard=GUARD, ref=ref,
                   expect=["Ok"] * len(good) + ["InvalidData"] * len(bad),
                   names=[f"{batch}-{i}" for i in range(len(streams))])
