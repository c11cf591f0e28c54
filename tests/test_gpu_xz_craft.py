"""Directed symbol-level LZMA2 / .xz streams on the GPU (zcg_xz.hip) against the
oracle, bit-exact.

Every other xz stream of the suite comes from liblzma's encoder, which writes
one block per stream, never sets a block header's size fields, writes the
LZMA2 control bytes in one pattern, keeps lc/lp/pb for the whole stream and
takes the distances and lengths the data offers.  tests/xz_craft.py writes
streams symbol by symbol and tests/xz_cases.py holds the tables;
tests/test_xz_craft_host.py pins them on the CPU against the reference
decoder, a plain model and the host build of the same decode core, whose
counting IO shows that no case takes the core outside its buffers.  Each
batch runs with the default 4 KiB history ring and with the 32 KiB one
(ZCG_FLAG_XZ_RING_32K).  Per stream: the status kind is the oracle's, Ok
chunks have the oracle's bytes, and the 0xAB guard behind the D decoded bytes
is intact whatever the status (flush() clips at D).

What each family is there for (move the lists in tests/xz_cases.py when a
constant of zcg_xz.hip or a rule of zcg_xz_core.h changes):

  A  the symbol loop's state machine: all 12 states left by a literal, a
     match, a rep and a short rep; matched literals that agree with the match
     byte or first differ at each bit; rep1..3 after a known history; rep and
     short rep at dictionary position 0 (invalid) and 1.
  B  the length coder's low / mid / high trees at every pos_state for pb 0..4,
     the literal coder at every lp context, lc/lp pairs up to lc + lp = 4
     (the second launch with the larger model), the slot context
     min(len - 2, 3), and dictionary resets in mid-block at positions that are
     no multiple of 16: contexts follow pos - dict_start.
  C  every distance slot 0..39 at its ends and middle (reverse trees, direct
     bits, every align value), behind 1 MiB of history in one batch; the end
     marker and slots 40, 62, 63 are rejected.
  D  dict_is_distance_valid: distance == position against position + 1 in a
     first block, after both kinds of reset, in a second block; the
     dictionary sizes of properties 0, 1, 2 and 40, 41.
  E  XzDevIO's ring: sources R - 514 .. R - 510 behind pos (in_ring's margin:
     lanes of one copy on the ring, in HBM or on both), at every ring phase of
     the wrap; pos + len - gfl at R / 2 - 1, R / 2, R / 2 + 1 (the flush
     trigger); overlapping copies of 273 across the wrap; copy_in's 256-byte
     pieces across a flush; literals and short reps across the trigger.
  F  the LZMA2 control table by (previous chunk, control byte), every control
     byte 3..0x7F, the properties byte, chunk size words off by one, the range
     coder's first byte, chunks of one literal, a chunk of 65 536 coded bytes.
  G  two and more blocks, odd block sizes, every check ID, delta on one block,
     lc + lp = 4 from a later chunk or block (the second launch decodes what
     the first had begun), the header's size fields true and wrong, c_end and
     u_end inside every part of a chunk, index and footer errors.
  H  D around chunk ends, block ends and dictionary resets, D at every split of
     a match of 273, the 32 KiB input window, one stream cut at every byte and
     with a bit flipped at every byte.

Nothing here is meant to fault: the invalid cases are streams the decoder's
own checks reject with a status.
"""
import numpy as np
import pytest

import xz_cases as cs
from golden_util import dtype_info
from gpu_check import GUARD, check_many
from zarr_amd._native import FLAG_XZ_RING_32K as RING_32K

pytestmark = pytest.mark.gpu

FLAGS = [0, RING_32K]
FLAG_IDS = ["ring4k", "ring32k"]


def check(cases, D, flags, dt="u1"):
    """One batch under one flag set: statuses, bytes and guards (the oracle is
    asked once per batch and must give the kinds the table names)."""
    es = dtype_info(dt)[0]
    assert D % es == 0 and all(c.D == D for c in cases)
    check_many("xz", [c.frame for c in cases], dt, D // es, flags, guard=GUARD, want=[c.want for c in cases],
               names=[c.name for c in cases], cache=True)


def family_batches(family):
    got = [(name, D, cases) for name, (D, cases) in cs.batches().items() if cases[0].family == family]
    assert got, family
    return got


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("family", "A B C D E F G H".split())
def test_family(family, flags):
    for name, D, cases in family_batches(family):
        check(cases, D, flags)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("seed", [17, 18])
def test_all_families_shuffled(seed, flags):
    """64 cases of every family and status in one batch, in random order:
    neighbouring chunks differ in status and path, and the second launch (the
    larger model) picks only the chunks that asked for it."""
    pool = [c for c in cs.all_cases() if c.D == cs.MAIN]
    big = [c for c in pool if any(sum(t["props"][:2]) == 4 for t in c.trace if "props" in t)]
    assert len(pool) == 771 and len(big) == 71
    rng = np.random.default_rng(seed)
    pick = [pool[i] for i in rng.permutation(len(pool))[:48]] + [big[i] for i in rng.permutation(len(big))[:16]]
    pick = [pick[i] for i in rng.permutation(len(pick))]
    assert len({c.family for c in pick}) >= 6 and len({c.want for c in pick}) == 2
    check(pick, cs.MAIN, flags)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_second_launch_leaves_the_other_chunks_alone(flags):
    """Family G's streams that change to lc + lp = 4 after output was written
    under the small model, between chunks that never ask for the larger one:
    valid, rejected and cut ones.  The second launch decodes its chunks from
    their first byte again and writes nothing elsewhere."""
    by_name = {c.name: c for c in cs.all_cases()}
    retry = [by_name[n] for n in ("G-big-model-later-chunk", "G-big-model-later-block",
                                  "G-big-model-later-block-bad-distance", "G-big-model-behind-D")]
    others = [by_name[n] for n in ("G-two-blocks", "G-csize+1", "A-rep-at-dpos0", "E4096-overlap-d64", "G-usize-larger",
                                   "F-csize-65536", "D-block2-dpos+1", "G-index-swapped")]
    order = [others[0], retry[0], others[1], others[2], retry[1], retry[2], others[3], others[4], retry[3]] + others[5:]
    check(order, cs.MAIN, flags)


@pytest.mark.parametrize("dt", [">u2", "bool"])
@pytest.mark.parametrize("family", ["A", "E"])
def test_element_transform(family, dt):
    """Families A and E through the element transform: it runs after the
    decode, on the output of a ring that keeps raw bytes (far matches read
    the output back), and leaves rejected chunks and the guard alone."""
    for name, D, cases in family_batches(family):
        check(cases, D, 0, dt=dt)
    name, D, cases = family_batches(family)[0]
    check(cases, D, RING_32K, dt=dt)
