"""Directed block-level bzip2 streams on the CPU.  TEST INFRASTRUCTURE ONLY.

tests/bz2_craft.py writes streams libbz2's encoder cannot: randomised
blocks, blocks that end in a run of four without its count byte (`tail4`),
L / origPtr pairs that are not one cycle, blocks of a chosen size, chosen
group counts, code lengths, table orders and surplus selectors.  Here

  * the writer is pinned against libbz2 (Python's bz2 and the oracle), so
    that a GPU failure on the same streams points at the kernel;
  * zh_bz2_decode, the host instantiation of the device's serial core, is
    compared with the oracle over the whole matrix (status, and the bytes
    when the oracle says OK).

The GPU runs the same cases in tests/test_gpu_bzip2_craft.py.
"""
import bz2

import numpy as np

import bz2_cases as cs
import bz2_craft as bc
import zref
from test_hostcore import host_bz2


def same(case, stream=None, D=None):
    s = case.stream() if stream is None else stream
    D = case.D if D is None else D
    r1 = zref.decode(zref.BZIP2, s, D)
    r2 = host_bz2(s, D)
    assert r1[0] == r2[0], (case.name, "oracle", r1[0], "host", r2[0])
    if r1[0] == zref.OK:
        assert r1[1] == r2[1], case.name
    return r1[0]


# ---- the writer against libbz2 ---------------------------------------------------
def test_writer_helpers():
    assert bc.crc32_msb(b"123456789") == 0xFC891918 and bc.crc32_msb(b"") == 0
    for n in (1, 2, 255, 4097):
        d = np.random.default_rng(n).integers(0, 256, n).astype(np.uint8).tobytes()
        assert bc.crc32_msb(d) == bc.crc32_msb_bytewise(d)
    assert bc.crc_combine(0x80000001, 0x10) == 0x00000013
    assert bc.rnums()[:3] == (619, 720, 127)
    assert bc.rand_positions(1400).tolist() == [617, 1337]
    assert [bc.rand_mask_at(p) for p in (0, 616, 617, 618, 1337)] == [0, 0, 1, 0, 1]
    assert bc.rle1_encode(b"aaaa") == b"aaaa\0"
    assert bc.rle1_encode(b"a" * 260) == b"aaaa\xfb" + b"aaaa\x01"
    assert bc.rle1_encode(b"xaaaaa", open_tail=True) == b"xaaaa"
    for c in (b"", b"abc", b"a" * 4, b"a" * 255 + b"b" * 256 + b"c" * 3, bytes(1000)):
        assert bc.rle1_decode(bc.rle1_encode(c)) == c
    assert bc.bwt(b"banana") == (b"nnbaaa", 3)
    rng = np.random.default_rng(8)
    for k, n in ((1, 1), (2, 9), (3, 700), (256, 3000), (40, 5000)):
        L = (rng.integers(0, k, n) * (rng.random(n) < 0.6)).astype(np.uint8).repeat(rng.integers(1, 4, n)).tobytes()
        used = sorted(set(L) | {7})
        assert bc.mtf_rle2(L, used).tolist() == bc.mtf_rle2_serial(L, used)
    assert bc.mtf_rle2(bytes(260) + b"\1", [0, 1]).tolist() == bc.mtf_rle2_serial(bytes(260) + b"\1", [0, 1])
    assert bc.count_blocks(bz2.compress(bytes(10))) == 1
    assert [bc.symbol_count(bc.bwt(cs.block_with_symbols(k))[0]) for k in (2, 50, 51, 101)] == [2, 50, 51, 101]
    assert bc.decode_rounds(1, 9) == 3 and bc.decode_rounds(720001, 9) == 4


def test_writer_multi_block_streams():
    """The streams of the GPU module's whole-stream and randomised tests."""
    blocks = list(cs.many_blocks())
    s, exp = bc.write_stream(blocks)
    assert bc.count_blocks(s) == 40 and bz2.decompress(s) == exp and len(exp) % 2 == 0
    streams, D, n = cs.fallback_streams()
    assert streams[0] == s and D == len(exp) and n == 40
    sts = [zref.decode(zref.BZIP2, x, D)[0] for x in streams]
    assert sts == [zref.OK, zref.INVALID_DATA, zref.EOF, zref.OK]
    streams, D = cs.randomised_streams()
    assert [zref.decode(zref.BZIP2, x, D)[0] for x in streams] == [zref.OK, zref.OK, zref.OK, zref.OK, zref.OK, zref.OK]
    assert len(bz2.decompress(streams[0])) == D
    for c in cs.sampling_cases():
        assert bz2.decompress(c.stream()) == c.expected() and len(c.blocks[0].T) in cs.SAMPLING_NBLOCK


def test_writer_large_block():
    """150 000 bytes over four symbols: many rounds of prefix doubling."""
    T = np.random.default_rng(0).integers(0, 4, 150000).astype(np.uint8).tobytes()
    s, exp = bc.write_stream([bc.Block(T=cs.closed(T), ngroups=6)], level=2)
    assert bz2.decompress(s) == exp


def _valid_cases():
    return [c for c in cs.host_matrix() if c.expected() is not None and not c.suffix and c.blocks
            and not any(b.is_tail4() or b.ngroups < 2 or b.ngroups > 6 for b in c.blocks)]


def test_writer_valid_streams_decode_under_libbz2():
    """Every valid crafted stream gives its content under bz2.decompress and
    OK with the same bytes under the oracle."""
    seen = set()
    for c in _valid_cases():
        s = c.stream()
        if s in seen:
            continue
        seen.add(s)
        exp = c.expected()
        assert bz2.decompress(s) == exp, c.name
        st, out = zref.decode(zref.BZIP2, s, len(exp))
        assert st == zref.OK and out == exp, c.name
    assert len(seen) >= 150, len(seen)
    # the empty stream, and a stream twice over
    empty = bc.write_stream([])[0]
    assert len(empty) == 14 and bz2.decompress(empty) == b""
    s, exp = bc.write_stream([bc.Block(T=b"hello", randomised=1), bc.Block(T=b"wooorld")])
    assert bz2.decompress(s + s) == exp * 2


def test_writer_filler_form_keeps_the_case():
    """Case.at(D): the same blocks behind a filler block, decoded to D."""
    for c in (cs.ladder_content_cases()[100], cs.tail4_cases()[50], cs.ladder_raw_cases()[7]):
        s = c.at(5000)
        st0, out0 = zref.decode(zref.BZIP2, c.stream(), c.D)
        st1, out1 = zref.decode(zref.BZIP2, s, 5000)
        assert st0 == st1, c.name
        if st0 == zref.OK:
            assert out1[5000 - c.D:] == out0 and out1[:5000 - c.D] == cs.filler(5000 - c.D).T


# ---- zh_bz2_decode against the oracle ---------------------------------------------
def _run(cases):
    ok = 0
    for c in cases:
        ok += same(c) == zref.OK
    return ok


def test_host_ladder_content():
    """nblock pinned at the sizes where stage B's wave quarters, the sample
    stride and stage C's per-thread segments change, randomised and not.
    A randomised block with a wrong CRC whose output ends exactly at D must
    still fail its CRC check (libbz2 checks it whatever the output loop
    returned)."""
    cases = cs.ladder_content_cases()
    assert len(cases) == 16 * 2 * 4 * 4
    assert _run(cases) == LADDER_CONTENT_OK
    bad = []
    for c in cases:
        if c.D == len(c.expected()):
            blk = c.blocks[0]
            bad.append(cs.Case(c.name + "-badcrc",
                               [bc.Block(T=blk.T, randomised=blk.randomised, crc_xor=0x00400000)], c.D))
    assert _run(bad) == 0  # all InvalidData


def test_host_ladder_raw():
    """L / origPtr pairs that are not one cycle: the serial walk's bytes are
    compared whenever D is reached before the block's CRC check, so the
    number of such cases is pinned (from the oracle's own run)."""
    cases = cs.ladder_raw_cases()
    assert len(cases) == 16 * 2 * 4 * 5 * 4
    ok = _run(cases)
    assert ok == LADDER_RAW_OK and 4 * ok >= len(cases)
    walked = [c for c in cases if c.blocks[0].orig < len(c.blocks[0].L)
              and not bc.is_one_cycle(c.blocks[0].L, c.blocks[0].orig)]
    assert _run(walked) == LADDER_RAW_OK_NOT_ONE_CYCLE and 4 * LADDER_RAW_OK_NOT_ONE_CYCLE >= len(cases)


def test_host_tail4():
    cases = cs.tail4_cases()
    assert len(cases) == 8 * 2 * 3 * 14
    assert _run(cases) == TAIL4_OK
    # the same on chains that are not one cycle: the count byte is chain
    # position nblock, which is not the block's first byte there
    assert _run(cs.walk_tail4_cases()) == WALK_TAIL4_OK


def test_host_knobs_zero_runs_and_stream_shapes():
    cases = cs.knob_cases() + cs.zero_run_cases() + cs.stream_shape_cases()
    assert _run(cases) == KNOBS_OK


def test_host_gpu_batches():
    """The streams of the GPU module's batches (every case behind a filler
    block, one D per batch).  The GPU tests compare bytes only where the
    oracle says OK, so the number of such streams per batch is pinned: the
    filler form must keep every case's verdict."""
    got = {}
    for name, (cases, D) in cs.gpu_batches().items():
        got[name] = sum(same(c, c.at(D), D) == zref.OK for c in cases)
        plain = sum(zref.decode(zref.BZIP2, c.stream(), c.D)[0] == zref.OK for c in cases)
        assert got[name] == plain, name
    assert got == GPU_BATCH_OK
    raw = [k for k in got if k.startswith("raw")]
    assert 4 * sum(got[k] for k in raw) >= sum(len(cs.gpu_batches()[k][0]) for k in raw)
    streams, D, _ = cs.fallback_streams()
    for s in streams:
        same(cs.Case("fallback", [], D), s, D)
    streams, D = cs.randomised_streams()
    for s in streams:
        same(cs.Case("randomised", [], D), s, D)


def test_host_matrix_ok_count():
    """How many cases of the whole matrix the oracle accepts, so that a
    change to the writer cannot silently move the matrix off the paths it
    was written for."""
    cases = cs.host_matrix()
    assert len(cases) == MATRIX_CASES
    assert _run(cases) == MATRIX_OK


# OK verdicts of the oracle (libbz2 1.0.8), recorded from its own run
LADDER_CONTENT_OK = 384
LADDER_RAW_OK = 907
LADDER_RAW_OK_NOT_ONE_CYCLE = 878
TAIL4_OK = 262
WALK_TAIL4_OK = 33
KNOBS_OK = 82
MATRIX_CASES = 3910
MATRIX_OK = 1668
# per GPU batch, in filler form
GPU_BATCH_OK = {"content": 360, "content_big": 24, "tail4": 295, "stage_a": 71, "shapes": 11, "sampling": 9,
                "raw-two": 228, "raw_big-two": 18, "raw-five_doubled": 216, "raw_big-five_doubled": 20,
                "raw-all256": 171, "raw_big-all256": 12, "raw-three_runs6": 224, "raw_big-three_runs6": 18}
