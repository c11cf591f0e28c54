"""The directed gzip-encoder payloads on the CPU.  TEST INFRASTRUCTURE ONLY.

For every case of tests/gz_enc_cases.py and every level it runs at:

  * the witness holds: the payload reaches the branch it is named for, as
    read from zlib's own stream or from the model's path report;
  * the serial model (zz_host_deflate) writes zlib's bytes;
  * at levels 4-9 the segment emulation (zz_host_deflate_seg), which restates
    dz_parse's stitch, writes zlib's bytes at seg 32 and at the GPU's seg, and
    cuts the serial parse's block records.

So a difference that tests/test_gpu_gzip_enc_craft.py finds on the GPU points
at the kernels, not at the core they share with the model.
"""
import os
import re
import zlib

import numpy as np
import pytest

import deflate_kit as dk
import gz_enc_cases as ec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zarr_amd", "csrc")


def test_constants_pinned():
    """The segment rule and the tail cap as the kernel has them, and zlib's level table as the core has it."""
    src = open(os.path.join(CSRC, "zcg_deflate.hip")).read()
    assert f"constexpr u32 DZ_TAILCAP = {ec.DZ_TAILCAP};" in src
    assert "const u32 seg = D32 ? (((D32 + 63) / 64 + 31) & ~31u) : 32u;" in src
    assert "if (nt + 1 >= DZ_TAILCAP) {" in src and "if (p - wb >= 250) {" in src
    assert [ec.gpu_seg(D) for D in (0, 1, 2048, 2049, 6000, 540000)] == [32, 32, 32, 64, 96, 8448]
    core = open(os.path.join(CSRC, "zcg_zlib_core.h")).read()
    for lv, cfg in ec.CONFIG.items():
        if lv != 6:  # (the default of the switch)
            assert re.search(r"case %d: return \{%d, %d, %d, %d\};" % ((lv,) + cfg), core), lv
    assert "default: return {8, 16, 128, 128};" in core
    assert "constexpr uint32_t BLOCK_SYMS = LIT_BUFSIZE - 1;" in core and ec.BLOCK_SYMS == (1 << 14) - 1


def test_case_list():
    cases = ec.all_cases()
    assert tuple(c.name for c in cases) == ec.CASE_NAMES and len(set(ec.CASE_NAMES)) == len(ec.CASE_NAMES)
    assert ec.RUNS == tuple((c.name, lv) for c in cases for lv in c.levels)
    for c in cases:
        assert 1 <= len(c.chunks) <= 8 and c.D <= 537 * 1024 and {len(x) for x in c.chunks} == {c.D}
        assert c.src is None or [len(x) for x in c.src] == [c.D] * len(c.chunks)


def test_reader_against_zlib():
    """deflate_kit.read_blocks on zlib's streams: the tokens rebuild the
    input, every block type occurs, and first_difference names the place."""
    text = dk.text(40000, 3)
    for payload in (b"", b"a", text, dk.noise(20000, 1), text[:3000] + dk.noise(17000, 2) + bytes(5000)):
        for level in (1, 6, 9):
            blocks = dk.read_blocks(ec.zlib_raw(payload, level))
            out = bytearray()
            for b in blocks:
                assert b.b0 == len(out)
                if b.type == 0:
                    out += payload[b.b0:b.b1]
                for p, n, d in b.tokens:
                    assert p == len(out)
                    if n == 0:
                        out.append(d)
                    else:
                        for _ in range(n):
                            out.append(out[-d])
                assert b.b1 == len(out)
            assert bytes(out) == payload and [b.last for b in blocks] == [0] * (len(blocks) - 1) + [1]
    types = [dk.read_blocks(ec.zlib_raw(x, 6))[0].type for x in (dk.noise(2000, 2), b"abcabc", text)]
    assert types == [0, 1, 2]
    a, b = ec.zlib_raw(text, 6), ec.zlib_raw(text[:30000] + b"#" + text[30001:], 6)
    msg = dk.first_difference(b, a)
    assert msg.startswith("block 1 symbol") or msg.startswith("block 0 symbol"), msg
    at = int(re.search(r"at input (\d+)", msg).group(1))
    assert 30000 - 258 <= at <= 30000, msg
    assert dk.first_difference(a, a).startswith("same structure")
    assert "does not parse" in dk.first_difference(a[:len(a) // 2], a)


def test_path_report():
    """The report against facts known otherwise: symbol counts and block
    ranges against zlib's stream, the segment sums, a tree that is limited
    (zlib's own stream then has a 15-bit code) and trees that are not."""
    b = ec.case("lit_overflow").chunks[0]
    for level in (1, 6):
        rep, z = ec.block_report(b, level), ec.zblocks(b, level)
        assert [(r.b0, r.b1, r.last, r.type) for r in rep] == [(x.b0, x.b1, x.last, x.type) for x in z]
        assert [r.s1 - r.s0 for r in rep if r.type] == [len(x.tokens) for x in z if x.type]
        limited = [bool(r.lim_l) for r in rep if r.type == 2]
        # a dynamic block whose tree was not limited is a Huffman tree: Kraft sum 1; 15 bits need the repair
        assert limited == [level == 6] and (max(z[1].ll) == 15) == (level == 6)
    r = ec.seg_report(ec.walk(6000, 3000), 6)
    assert r.nseg == 63 and r.nsym == sum(len(x.tokens) for x in ec.zblocks(ec.walk(6000, 3000), 6))
    assert r.nsym <= int(r.n1.sum() + r.nt.sum())
    one = ec.seg_report(b"abc", 6)
    assert (one.nseg, one.fin, one.fallback, one.nsym) == (1, 1, 0, 3)


@pytest.mark.parametrize("name,level", ec.RUNS, ids=[f"{n}-{lv}" for n, lv in ec.RUNS])
def test_case(name, level):
    c = ec.case(name)
    assert c.witness(c, level)
    for i, b in enumerate(c.chunks):
        ref = ec.zlib_raw(b, level)
        got = ec.host_deflate(b, level)
        assert got == ref, (name, level, i, dk.first_difference(got, ref))
        if level >= 4:
            for seg in (32, ec.gpu_seg(len(b))):
                got = ec.host_deflate(b, level, seg)
                assert got == ref, (name, level, i, seg, dk.first_difference(got, ref))
            # the block records zz::block_rec cuts on the stitched stream are the serial parse's
            serial = [(r.s0, r.s1, r.b0, r.b1, r.in_win, r.last) for r in ec.block_report(b, level)]
            assert ec.seg_block_records(b, level) == serial, (name, level, i)


def test_serialised_sources():
    """The device gets the array's native bytes; the stream holds the serialised ones."""
    for c in ec.all_cases():
        if c.dt == ">u2":
            for src, b in zip(c.src, c.chunks):
                assert np.frombuffer(src, "<u2").astype(">u2").tobytes() == b
        elif c.dt == "bool":
            for src, b in zip(c.src, c.chunks):
                assert (np.frombuffer(src, np.uint8) != 0).astype(np.uint8).tobytes() == b
        else:
            assert c.dt == "u1" and c.src is None
    assert {c.dt for c in ec.all_cases()} == {"u1", ">u2", "bool"}
    assert zlib.ZLIB_VERSION  # (the reference of every comparison here)
