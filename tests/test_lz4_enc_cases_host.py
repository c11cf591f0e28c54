"""The directed LZ4-encoder blocks on the CPU.  TEST INFRASTRUCTURE ONLY.

For every case of tests/lz4_enc_cases.py:

  * the model with the path report (tests/hostcore/lz4_fast_ref.c:
    zref_lz4_fast_block_report) writes liblz4's bytes for every block,
    LZ4_compress_fast(.., n - 1, 1), and the same bytes as the plain model;
  * its restatement of le_block's batches finds every match the serial search
    finds, at the same attempt, and leaves the same table (emu_diff == 0);
  * the witness holds: the blocks reach the branch the case is named for;
  * the expected frame, the oracle's liblz4 LZ4F frame, decodes to the content.

So a difference that tests/test_gpu_lz4_enc_craft.py finds on the GPU points
at the kernel, not at the payload or the expectation.
"""
import os
import re

import numpy as np
import pytest

import lz4_enc_cases as ec
import test_hostcore as th

zref = pytest.importorskip("zref")

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zarr_amd", "csrc")


def test_constants_pinned():
    """What the batch restatement copies from the kernel, read out of its text."""
    src = open(os.path.join(CSRC, "zcg_lz4_enc.hip")).read()
    assert f"constexpr u32 LE_MFLIMIT = {ec.MFLIMIT};" in src
    assert f"constexpr u32 LE_LASTLIT = {ec.LASTLIT};" in src
    assert "constexpr u32 LE_64KLIMIT = 65536 + LE_MFLIMIT - 1;" in src and ec.LIMIT64K == 65536 + ec.MFLIMIT - 1
    assert "const u32 st = k == 0 ? 1u : (63u + k) >> 6;" in src
    assert [ec.step(k) for k in (0, 1, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert "__launch_bounds__(64) void lz4_block_exact" in src and "const u32 k = k0 + lane;" in src
    assert "le_wave_min(dup ? (rd < lane ? rd : lane) : 64u)" in src and ec.LANES == 64
    assert "const u32 P = g + 1 < V ? g + 1 : V;" in src and "const bool valid = nxt <= mfl1;" in src
    assert len(re.findall(r"\+ 65535u >= ", src)) == 2 and ec.DIST_MAX == 65535
    ref = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcore", "lz4_fast_ref.c")).read()
    assert "#define ZR_LANES 64" in ref and "st[j] = k == 0 ? 1u : (63u + k) >> 6;" in ref
    assert len(ec.REP_FIELDS) == len(re.search(r"enum \{\s*ZR_MODE,(.*?)ZR_N\s*\}", ref, re.S)
                                                       .group(1).split(","))


def test_case_list():
    cases = ec.all_cases()
    assert tuple(c.name for c in cases) == ec.CASE_NAMES and len(set(ec.CASE_NAMES)) == len(cases)
    for c in cases:
        assert 1 <= len(c.chunks) < 20 and {len(x) for x in c.chunks} == {c.D}, c.name
        assert all(0 <= v < c.D and 0 <= k < len(c.chunks) for k, v in c.short.items())
        assert c.raw is None or [len(x) for x in c.raw] == [c.D] * len(c.chunks)
    assert any(c.is_bits() for c in cases) and any(c.D % 8 == 0 for c in cases)
    # the mandatory classes each have a case
    for prefix in ("stale_u16", "stale_u32", "stale_u16_g0", "cut_batches", "distance_next_65535", "distance_search_65536",
                   "mode_65546_256k", "mode_65547_1024k", "mode_tail_65546", "mode_tail_65547", "catchup_", "exit_ret0_lit",
                   "exit_ret0_ml", "exit_ret0_last", "tiny_12", "tiny_13", "tiny_14", "length_fields",
                   "last_literal_lengths", "count_lanes", "rematch_chains", "frame_mixed", "xxh_1", "xxh_batch_17",
                   "xxh_refused_5"):
        assert any(n.startswith(prefix) for n in ec.CASE_NAMES), prefix


def test_report_against_known_blocks():
    """The report on blocks whose path is known otherwise."""
    r = ec.report(bytes(1000))           # one match from position 1 to matchlimit
    assert (r.nseq, r.seq[0][:4], r.exit, r.at_matchlimit, r.last_lit) == (1, (1, 1, 990, 1), ec.MATCH_END, 1, 5), r
    r = ec.report(ec.noise(65536, 1))    # noise: one search, liblz4 returns 0
    assert r.stored and r.exit == ec.RET0_LAST and r.searches == 1 and r.nseq == 0 and r.stale == 0 and r.emu_diff == 0
    assert r.batches > r.cut > 0 and r.vshort == 1
    assert ec.report(b"").stored and ec.report(ec.noise(12, 2)).searches == 0


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_case(name):
    c = ec.case(name)
    for i, chunk in enumerate(c.chunks):
        for k, blk in enumerate(ec.blocks_of(chunk, c.B)):
            (r1, o1), (r2, o2) = th.lz4_pair(blk)
            rep = ec.report(blk)
            assert (rep.ret, rep.out) == (r1, o1) == (r2, o2), (name, i, k, r1, r2, rep.ret)
            assert rep.emu_diff == 0, (name, i, k, rep)
        if i in c.short:
            continue
        st, frame = zref.encode(zref.LZ4, c.B, np.frombuffer(chunk, np.uint8))
        assert st == zref.OK
        st, back = zref.decode(zref.LZ4, frame, c.D, 1, False, False)
        assert st == zref.OK and back == chunk, (name, i)
    assert c.witness(c), name


def test_serialised_sources():
    """What the device gets for the bool run: any non-zero byte where the stream holds 1."""
    for c in ec.all_cases():
        if c.raw is not None:
            for src, b in zip(c.raw, c.chunks):
                assert (np.frombuffer(src, np.uint8) != 0).astype(np.uint8).tobytes() == b and src != b
