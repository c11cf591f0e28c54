"""The bzip2 stream reader and the directed encoder payloads on the CPU.
TEST INFRASTRUCTURE ONLY.

  * tests/bz2_read.py is pinned against libbz2's encoder (Python's bz2) and
    against the block-level writer (tests/bz2_craft.py): contents, CRCs,
    every header field, and the parsed fields written back give the stream
    bit for bit;
  * every case of tests/bz2_enc_cases.py asserts its witness under the model:
    that the payload reaches the branch of zcg_bz2_enc.hip it is named for;
  * every payload goes through libbz2's own encoder and back, and
    check_stream, which tests/test_gpu_bzip2_enc_craft.py applies to the
    GPU's streams, holds for libbz2's (but for the cut rule, which is the
    kernel's own), so a failure on the GPU points at the kernel.
"""
import bz2

import numpy as np
import pytest

import bz2_cases as cs
import bz2_craft as bc
import bz2_enc_cases as ec
import bz2_read as br
from test_hostcore import _data


def parsed(stream, content, level):
    lv, blocks, comb, pad = br.read_stream(stream)
    assert lv == level and pad < 8
    assert b"".join(b.content for b in blocks) == content
    c = 0
    for b in blocks:
        assert b.crc == bc.crc32_msb(b.content) and len(b.L) == len(b.T)
        assert b.symbols[-1] == len(b.used) + 1 and b.symbols.count(b.symbols[-1]) == 1
        assert b.nselectors == len(b.selectors) and len(b.lengths) == b.ngroups
        c = bc.crc_combine(c, b.crc)
    assert comb == c
    assert br.write_back(lv, blocks, comb) == stream
    return blocks


# ---- the reader ---------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_reader_against_libbz2(kind, level):
    for n in (0, 1, 777, 250001):
        content = _data(np.random.default_rng(kind * 10 + level), kind, n)
        s = bz2.compress(content, level)
        blocks = parsed(s, content, level)
        assert len(blocks) == bc.count_blocks(s)
        assert [b.bit_off for b in blocks[:1]] == [32][:len(blocks)]
        assert all(b.randomised == 0 for b in blocks)
        ec.check_stream(s, content, level, ours=False)


def test_reader_against_writer():
    """Randomised blocks, 2 to 6 tables in any order, equal lengths of 8 and
    17, surplus selectors, unused bytes in the symbol map."""
    blocks = list(cs.many_blocks())
    s, exp, offs = bc.write_stream_info(blocks)
    got = parsed(s, exp, 1)
    assert [b.bit_off for b in got] == offs[:-1]
    for b, w in zip(got, blocks):
        assert (b.randomised, b.ngroups, b.T) == (w.randomised, w.ngroups, w.T)
        assert (b.L, b.orig) == w.resolved()[:2]
    seen = set()
    for c in cs.knob_cases():
        blk = c.blocks[0]
        if blk.T is None or blk.crc_xor or (blk.lengths == 20 and "len20" in seen):
            continue
        seen.add(f"len{blk.lengths}")
        s, exp = bc.write_stream(c.blocks)
        if not 2 <= blk.ngroups <= 6:
            with pytest.raises(br.FormatError):
                br.read_stream(s)
            continue
        b = parsed(s, exp, 1)[0]
        need = -(-len(b.symbols) // bc.G_SIZE)
        assert (b.ngroups, b.nselectors, b.randomised) == (blk.ngroups, need + blk.extra_selectors, blk.randomised)
        assert b.used == sorted(set(b.L) | set(blk.used_extra))
        if blk.lengths != "huffman":
            assert all(l == blk.lengths for tab in b.lengths for l in tab)
        if blk.order is not None:
            assert b.selectors == [blk.order[g % len(blk.order)] for g in range(b.nselectors)]
    assert {"len8", "len17", "len20", "lenhuffman"} <= seen


def test_reader_rejects():
    s = bz2.compress(b"hello hello hello", 1)
    for bad in (s[:-1], s[:20], b"BZh0" + s[4:], s[:-1] + bytes([s[-1] | 1]), s[:4] + b"\x00" + s[5:]):
        with pytest.raises(br.FormatError):
            br.read_stream(bad)
    assert br.read_stream(bz2.compress(b"", 3)) == (3, [], 0, 0)
    assert br.read_stream(s + b"\0")[3] >= 8


# ---- the model's helpers -------------------------------------------------------------
def _brute_lcp(t):
    n = len(t)
    rots = sorted((t[i:] + t[:i], i) for i in range(n))
    out = []
    for (a, _), (b, _) in zip(rots, rots[1:]):
        k = 0
        while k < n and a[k] == b[k]:
            k += 1
        out.append(k)
    return out, len({r for r, _ in rots})


def test_sort_witness_helpers():
    rng = np.random.default_rng(12)
    texts = [b"abab", b"abcabc", b"aab" * 5, b"banana", b"a", b"aaaaaaa", b"ab" * 9 + b"c"]
    texts += [rng.integers(0, k, n).astype(np.uint8).tobytes() for k, n in ((2, 97), (3, 200), (2, 64), (5, 333))]
    for t in texts:
        lcp, distinct = _brute_lcp(t)
        assert bc.adjacent_lcp(t).tolist() == lcp
        assert bc.adjacent_lcp(t, cap=5).tolist() == [min(x, 5) for x in lcp]
        assert int(bc.rotation_ranks(t)[-1][1].max()) + 1 == distinct
        L, orig = bc.bwt(t)
        first, count = bc.orig_range(t)
        assert count == len(t) // distinct and first <= orig < first + count
        for dpre in (1, 2, 3):
            keys = sorted((t * 4)[i:i + dpre] for i in range(len(t)))
            sizes = [keys.count(k) for k in sorted(set(keys))]
            assert bc.prefix_group_sizes(t, dpre).tolist() == sizes
    assert ec.sub_batches(64, 5000) == [4096, 904] and ec.sub_batches(1 << 20, 300) == [128, 128, 44]
    assert ec.sub_batches(60000, 6) == [6] and ec.sub_batches(200 << 20, 3) == [1, 1, 1]
    assert [ec.prefix_bytes(n) for n in (1, 2, 256, 257, 300, 4096, 65536, 65537)] == [3, 3, 3, 2, 2, 2, 2, 1]
    assert [ec.ngroups_rule(n) for n in ec.NGROUPS_NMTF] == [2, 3, 3, 4, 4, 5, 5, 6]


def test_cut_model():
    rng = np.random.default_rng(13)
    for n in (0, 1, 5, 300, 4000):
        c = (rng.integers(0, 3, n) * (rng.random(n) < 0.4)).astype(np.uint8).repeat(rng.integers(1, 300, n))
        c = c.tobytes()[:3 * n]
        assert ec.rle1(c) == bc.rle1_encode(c)
        pin, pout = ec.pieces(c)
        assert pin.sum() == len(c) and pout.sum() == len(bc.rle1_encode(c)) and (pin <= 255).all()
    for level in (1, 2):
        bm = ec.bmax(level)
        assert bm == 100000 * level - 19
        c = cs.norun_bytes(bm, seed=1) + b"\7" * 3 + cs.norun_bytes(50, seed=2)
        assert ec.model_cuts(c, level) == [(0, bm), (bm, bm + 53)]  # the three equal bytes are one piece
        c = cs.norun_bytes(bm - 2, seed=1) + b"\7" * 3 + cs.norun_bytes(50, seed=2)
        assert ec.model_cuts(c, level) == [(0, bm - 2), (bm - 2, bm + 51)]
        c = cs.norun_bytes(bm - 3, seed=1) + b"\7" * 3 + cs.norun_bytes(50, seed=2)
        assert ec.model_cuts(c, level) == [(0, bm), (bm, bm + 50)]
        assert ec.cut_paths(c, level) == ["step"]
        assert ec.model_cuts(c[:bm], level) == [(0, bm)] and ec.cut_paths(c[:bm], level) == []
        blocks = ec.model_blocks(b"\5" * (60 * bm), level)   # 255 bytes are 5: bmax is no multiple of 5
        assert b"".join(blocks) == b"\5" * (60 * bm) and len(blocks) == 2
        assert len(ec.rle1(blocks[0])) == bm - bm % 5 and len(blocks[0]) == bm // 5 * 255


# ---- the cases ---------------------------------------------------------------------------
CASES = ec.CASE_NAMES


def test_case_list():
    """Every case has a name to be collected under, and the shape the GPU
    test expects: one length per batch, chunks of at most 200 KB."""
    assert tuple(c.name for c in ec.all_cases()) == CASES and len(set(CASES)) == len(CASES)
    assert [tuple(c.name for c in build()) for _, build in ec._GROUPS] == [names for names, _ in ec._GROUPS]
    for c in ec.all_cases():
        assert len({len(x) for x in c.chunks}) == 1 and c.D <= 200 * 1024 + 2000 and len(c.chunks) <= 5000
        assert c.src is None or [len(x) for x in c.src] == [c.D] * len(c.chunks)


@pytest.mark.parametrize("name", CASES)
def test_witness(name):
    c = ec.case(name)
    assert c.witness(c)


@pytest.mark.parametrize("name", CASES)
def test_payload_through_libbz2(name):
    c = ec.case(name)
    streams = [bz2.compress(x, c.level) for x in c.chunks]
    for x, s in zip(c.chunks, streams):
        assert bz2.decompress(s) == x
    step = max(1, len(c.chunks) // 50)
    for i in range(0, len(c.chunks), step):
        blocks = ec.check_stream(streams[i], c.chunks[i], c.level, ours=False, at=(name, i))
        # libbz2 cuts a few bytes later than the model where a run ends at bmax, never earlier
        assert len(blocks) <= len(c.texts()[i])


def test_deep_codes_through_libbz2():
    """libbz2's encoder, whose table selection and length limiting the
    kernel restates, codes the whole block with one table, cuts its codes
    at 17 bits, and an unrestricted tree over what that table coded is 20
    deep.  (The GPU test asserts the same of the kernel's stream.)"""
    c = ec.case("deep_codes")
    deep = [t for t in ec.table_depths(bz2.compress(c.chunks[0], c.level)) if t[0]]
    assert deep == [(len(c.chunks[0]) + 1, 17, 20)]


def _rejected(stream, content, what, level=1):
    with pytest.raises(AssertionError) as e:
        ec.check_stream(stream, content, level)
    assert any(what in str(x) for x in e.value.args[0]), e.value.args[0]


def test_check_stream_rejects():
    """check_stream accepts a stream written the encoder's way and names the
    stage of one that is not: every field it compares, changed by the writer."""
    T = cs.norun_bytes(3000, seed=5)
    L, orig = bc.bwt(T)
    ng = ec.ngroups_rule(bc.symbol_count(L))
    good = dict(T=T, ngroups=ng, plain=True)
    ec.check_stream(bc.write_stream([bc.Block(**good)])[0], T, 1)
    for what, blocks, level in (
            ("level", [bc.Block(**good)], 2),
            ("nGroups", [bc.Block(**dict(good, ngroups=ng - 1))], 1),
            ("nSelectors", [bc.Block(**dict(good, extra_selectors=1))], 1),
            ("randomised", [bc.Block(**dict(good, randomised=1))], 1),
            ("lengths", [bc.Block(**dict(good, lengths=18))], 1),
            ("crc", [bc.Block(**dict(good, crc_xor=1 << 9))], 1),
            ("symbol map", [bc.Block(**dict(good, used_extra=[0xF0]))], 1),
            ("cuts", [bc.Block(T=T[:1000], ngroups=4, plain=True), bc.Block(T=T[1000:], ngroups=5, plain=True)], 1),
            ("content", [bc.Block(L=L, orig=orig + 1, crc=bc.crc32_msb(T), ngroups=ng)], 1)):
        _rejected(bc.write_stream(blocks, level)[0], T, what)
    # a last column that is not the sorted rotations' (two bytes swapped), with the CRC of what it decodes to
    i = next(i for i in range(len(L) - 1) if L[i] != L[i + 1])
    L2 = L[:i] + L[i + 1:i + 2] + L[i:i + 1] + L[i + 2:]
    walked = br.read_stream(bc.write_stream([bc.Block(L=L2, orig=orig, crc=0, ngroups=ng)])[0])[1][0].content
    _rejected(bc.write_stream([bc.Block(L=L2, orig=orig, crc=bc.crc32_msb(walked), ngroups=ng)])[0], walked, "L")
    # a run of three across the limit: whole in the second block, not one byte and two
    bm = ec.bmax(1)
    c = cs.norun_bytes(bm - 1, seed=1) + b"\7" * 3 + cs.norun_bytes(50, seed=2)
    split = [bc.Block(T=c[:bm], ngroups=6, plain=True), bc.Block(T=c[bm:], ngroups=2, plain=True)]
    _rejected(bc.write_stream(split)[0], c, "cuts")
    # a periodic text: origPtr at any of the equal rotations; anywhere else is another text
    P = b"abc" * 40
    Lp, _ = bc.bwt(P)
    first, count = bc.orig_range(P)
    assert (first, count) == (0, 40)
    for o in (0, 17, 39):
        ec.check_stream(bc.write_stream([bc.Block(L=Lp, orig=o, crc=bc.crc32_msb(P), ngroups=2)])[0], P, 1)
    _rejected(bc.write_stream([bc.Block(L=Lp, orig=40, crc=bc.crc32_msb(P), ngroups=2)])[0], P, "content")


def test_serialised_sources():
    """The device gets the array's native bytes; the stream holds the
    serialised ones: byte-swapped, and 0 / 1 for a bool array."""
    for name, dt in (("swapped_runs_u4", ">u4"), ("swapped_runs_i2", ">i2")):
        c = ec.case(name)
        native = np.frombuffer(c.src[0], np.dtype(dt).newbyteorder("="))
        assert native.astype(np.dtype(dt)).tobytes() == c.chunks[0]
    c = ec.case("swapped_runs_bool")
    raw = np.frombuffer(c.src[0], np.uint8)
    assert set(raw.tolist()) == {0, 1, 2, 255} and (raw != 0).astype(np.uint8).tobytes() == c.chunks[0]
