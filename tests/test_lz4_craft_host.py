"""Directed sequence-level LZ4 frames on the CPU.  TEST INFRASTRUCTURE ONLY.

tests/lz4_craft.py writes frames liblz4's encoder cannot (offset 0, matches
ending at the last legal byte of a full block, chosen offsets, lengths and
positions); tests/lz4_cases.py holds the tables.  Here

  * every case gets the status its table names from the reference decoder,
    and an "ok" case the bytes of the plain model, at the batch's D and at
    full length;
  * the writer is pinned the other way: frames of liblz4's encoder are parsed
    into sequences and written again, byte for byte;
  * the census of the tables is pinned, so that a change to the writer or the
    tables cannot silently move them off the branches they were written for.

The GPU runs the same batches in tests/test_gpu_lz4_craft.py.
"""
import numpy as np
import pytest

import lz4_cases as cs
import lz4_craft as lc
import zref

STATUS = {zref.OK: "ok", zref.INVALID_DATA: "invalid", zref.EOF: "eof"}


def oracle(cases, D):
    st, out = zref.decode_batch(zref.LZ4, [np.frombuffer(c.frame, np.uint8) for c in cases], D)
    return [STATUS[int(x)] for x in st], out


@pytest.mark.parametrize("family", "A B C1 C2 C3 C4 D E F G H".split())
def test_cases_against_oracle_and_model(family):
    seen = 0
    for name, (D, cases) in cs.batches().items():
        if cases[0].family != family:
            continue
        got, out = oracle(cases, D)
        for c, st, o in zip(cases, got, out):
            seen += 1
            assert st == c.want, (c.name, D, st, c.want)
            m = lc.model(c.blocks, c.linked)
            if c.want != "ok":
                continue
            assert m is not None and len(m) == c.length >= D, c.name
            assert o.tobytes() == m[:D], c.name
            if c.length != D:
                st2, o2 = zref.decode(zref.LZ4, c.frame, c.length)
                assert st2 == zref.OK and o2 == m, c.name
    assert seen == cs.census()["cases"][family]


def test_model_declines_offsets_before_low():
    first = [(b"abcdefgh", None, None)]
    reach = [(b"xy", 10, 4), (b"0123456789ab", None, None)]
    assert lc.model([first, reach], linked=True) == b"abcdefghxyabcd0123456789ab"
    assert lc.model([first, reach], linked=False) is None
    assert lc.model([[(b"xy", 3, 4), (b"", None, None)]]) is None
    assert lc.model([[(b"", 0, 4), (b"ab", 2, 5), (b"", None, None)]]) == bytes(4) + b"abababa"
    assert lc.decoded_len([first, reach, ("stored", b"123")]) == 29
    for c in cs.all_cases():  # the invalid offset cases are those the model declines
        if c.want == "invalid" and ("off=op+1" in c.name or "reach-op" in c.name):
            assert lc.model(c.blocks, c.linked) is None, c.name


def test_writer_helpers():
    assert lc.xxh32(b"") == 0x02CC5D05 and lc.xxh32(b"a") == 0x550D7456
    assert lc.seq(b"", 0, 4) == b"\x00\x00\x00" and lc.seq(b"ab") == b"\x20ab"
    assert lc.seq(b"x" * 15, 1, 19) == b"\xff\x00" + b"x" * 15 + b"\x01\x00\x00"
    assert lc.seq(b"x" * 270)[:3] == b"\xf0\xff\x00" and lc.seq(b"x" * 269)[:2] == b"\xf0\xfe"
    assert lc.seq(b"", 513, 274) == b"\x0f\x01\x02\xff\x00" and lc.seq(b"", 1, 273) == b"\x0f\x01\x00\xfe"
    for n in (0, 14, 15, 269, 270, 271, 5000):
        for ml in (None, 4, 18, 19, 274, 40000):
            assert lc.seq_len(n, ml) == len(lc.seq(bytes(n), None if ml is None else 1, ml))


def payloads():
    rng = np.random.default_rng(3)
    walk = np.cumsum(rng.integers(-3, 4, 40000)).astype("<i2").tobytes()                # two blocks
    runs = np.repeat(rng.integers(0, 4, 3000, dtype=np.uint8), rng.integers(1, 90, 3000))[:70000].tobytes()
    mixed = rng.integers(0, 256, 66000, dtype=np.uint8).tobytes() + walk[:30000]        # a stored block first
    return [walk, runs, mixed]


@pytest.mark.parametrize("prefs", [{}, dict(linked=True), dict(block_checksum=True), dict(content_size=True),
                                   dict(content_checksum=False), dict(block_size_id=5),
                                   dict(linked=True, block_checksum=True, content_size=True)],
                         ids=lambda p: "+".join(p) or "default")
def test_writer_reproduces_encoder_frames(prefs):
    for p in payloads():
        f = zref.lz4_frame_custom(p, **prefs)
        blocks, got = lc.parse_frame(f)
        assert got["linked"] == bool(prefs.get("linked")) and got["block_checksum"] == bool(prefs.get("block_checksum"))
        assert (got["content_size"] == len(p)) if prefs.get("content_size") else got["content_size"] is None
        assert lc.frame(blocks, **got) == f
        assert lc.model(blocks, got["linked"]) == p and lc.decoded_len(blocks) == len(p)
    p = payloads()[0]
    st, f = zref.encode(zref.LZ4, 65536, np.frombuffer(p, np.uint8))  # the frame the product's writer emits
    blocks, got = lc.parse_frame(f)
    assert st == zref.OK and lc.frame(blocks, **got) == f


def test_census():
    cen = cs.census()
    s = cen["sets"]
    assert cen["cases"] == CASES
    assert cen["want"] == WANT
    assert s["A.lit"] == set(cs.LIT_LENGTHS) and s["A.ml"] == set(cs.MATCH_LENGTHS)
    assert s["A.lit_token_at"] == set(range(64)) and s["A.ml_token_at"] == set(range(64))
    assert s["A.lit_chain"] == {(nb, w) for nb in range(14, 21) for w in (0, 3, 15, 16, 47, 48, 49, 62, 63)}
    assert s["B.successor_at"] == {63, 64, 65} and s["B.total"] == {(0, 32), (28, 4), (29, 4), (0, 33)}
    assert s["C1"] == {(off, ml, ph) for off in range(16) for ml in (4, 15, 16, 17, 31, 32, 33, 48, 100, 1030)
                       for ph in (0, 1, 15, 16, 17, 64, 111, 112, 113, 127)}
    assert s["C2.near"] == {(off, ml, ph) for off in range(90, 101) for ml in (20, 40) for ph in range(128)}
    assert s["C2"] == {(off, ml, ph) for off in (16, 17, 31, 32, 63, 64, 65, 123, 124, 127, 128, 129)
                       for ml in (20, 40) for ph in (0, 1, 15, 16, 17, 64, 111, 112, 113, 127)}
    assert s["C3.far"] == {(off, ml) for off in (2047, 2048, 2049, 4095, 65535) for ml in (20, 40)}
    assert s["C3.ring"] == {(off, ml) for off in range(1900, 2050) for ml in (20, 100)}
    assert s["C3.block_start"] == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert s["C4.overlap"] == {(off, 100) for off in range(16, 32)}
    assert s["D.lit"] == {1024, 1025, 2048, 2049, 3073}
    assert s["D.match"] == {(off, n) for off in (1, 7, 16, 100, 1000, 1024, 1025, 2047, 2048, 2049, 3000)
                            for n in (1024, 1025, 2048, 2049, 3073)}
    pairs = {"end-cap5": "ok", "end-cap4": "invalid", "start-cap12": "ok", "start-cap11": "invalid",
             "start-cap9": "invalid", "lits-cap": "ok", "lits-cap+1": "invalid", "match-past-cap": "invalid"}
    assert s["E"] == {(k + tag, v) for k, v in pairs.items() for tag in ("", "-256k")}
    assert s["G.reach"] == {(d, ml) for d in (0, -1, 1, 65535) for ml in (20, 400)}
    # the size words: most cut a sequence (invalid), the exact one and a few others decode
    f_words = [c for c in cs.all_cases() if c.name[:4] in ("F-a-", "F-b-") and ("-word" in c.name or "-cut" in c.name)]
    assert len(f_words) == 2 * (42 + 39)
    assert sum(c.want != "ok" for c in f_words) * 4 > 3 * len(f_words) and sum(c.want == "ok" for c in f_words) > 0
    assert cs.step_census() == STEPS
    assert cs.h_values() == H_VALUES and all(len(b[1]) == 8 for n, b in cs.batches().items() if n.startswith("H@"))
    # a batch: at most a few hundred streams of at most about 130 KiB, except the 256 KiB blocks of E
    for name, (D, cases) in cs.batches().items():
        assert len(cases) <= 300 and (D <= 2 * cs.CAP or name.startswith("E-256k")), name




# the tables' own numbers
CASES = {"A": 110, "B": 27, "C1": 16, "C2": 23, "C3": 30, "C4": 2, "D": 21, "E": 32, "F": 458, "G": 51, "H": 408}
WANT = {("A", "ok"): 110, ("B", "ok"): 27, ("C1", "ok"): 16, ("C2", "ok"): 23, ("C3", "ok"): 21,
        ("C3", "invalid"): 9, ("C4", "ok"): 2, ("D", "ok"): 21, ("E", "ok"): 12, ("E", "invalid"): 20,
        ("F", "invalid"): 449, ("F", "ok"): 5, ("F", "eof"): 4, ("G", "ok"): 29, ("G", "eof"): 12,
        ("G", "invalid"): 10, ("H", "ok"): 408}
H_VALUES = [1344, 1407, 1408, 1409, 1415, 1416, 1431, 1432, 1443, 1444, 1445, 1447, 1448, 1449, 1472, 1475, 1476,
            1491, 1492, 1503, 1504, 1505, 1507, 1508, 1509, 1536, 1600, 1649, 1650, 1664, 1665, 1666, 1677, 1678,
            1679, 1681, 1682, 1683, 1728, 3392, 3424, 3425, 3440, 3441, 3452, 3453, 3454, 3456, 3457, 3458, 3520]
# steps and rounds of the wave kernel by path (lz4_cases.step_census)
STEPS = {
    ("A", "exit64-heavy"): 2,
    ("A", "exit64-light"): 16,
    ("A", "exit65-heavy"): 40,
    ("A", "exit65-light"): 32,
    ("A", "heavy"): 286,
    ("A", "light"): 64,
    ("A", "literals past 64-light"): 8,
    ("A", "ring+0-heavy"): 3,
    ("A", "ring+1-heavy"): 1,
    ("A", "round of 1024"): 5142,
    ("A", "successor at 63"): 7,
    ("B", "21+ sequences"): 2,
    ("B", "exit64-heavy"): 2,
    ("B", "exit64-light"): 7,
    ("B", "exit65-heavy"): 2,
    ("B", "exit65-light"): 3,
    ("B", "final-light"): 3,
    ("B", "heavy"): 49,
    ("B", "light"): 30,
    ("B", "literals past 64-light"): 14,
    ("B", "round of 1024"): 1269,
    ("B", "successor at 63"): 9,
    ("C1", "exit64-heavy"): 80,
    ("C1", "exit64-light"): 192,
    ("C1", "exit65-heavy"): 32,
    ("C1", "exit65-light"): 112,
    ("C1", "heavy"): 560,
    ("C1", "light"): 1360,
    ("C1", "literals past 64-light"): 848,
    ("C1", "round of 1024"): 576,
    ("C1", "successor at 63"): 192,
    ("C2", "exit64-heavy"): 170,
    ("C2", "exit64-light"): 147,
    ("C2", "exit65-light"): 23,
    ("C2", "heavy"): 351,
    ("C2", "light"): 423,
    ("C2", "literals past 64-light"): 131,
    ("C2", "round of 1024"): 958,
    ("C2", "successor at 63"): 48,
    ("C3", "exit65-light"): 150,
    ("C3", "heavy"): 353,
    ("C3", "light"): 158,
    ("C3", "literals past 64-light"): 8,
    ("C3", "ring+0-heavy"): 1,
    ("C3", "ring+0-light"): 1,
    ("C3", "ring+1-heavy"): 1,
    ("C3", "ring+1-light"): 1,
    ("C3", "ring-1-heavy"): 1,
    ("C3", "ring-1-light"): 1,
    ("C3", "round of 1024"): 1144,
    ("C3", "successor at 63"): 3,
    ("C4", "exit64-heavy"): 1,
    ("C4", "heavy"): 7,
    ("C4", "light"): 2,
    ("C4", "literals past 64-light"): 2,
    ("C4", "round of 1024"): 93,
    ("D", "heavy"): 102,
    ("D", "ring+0-heavy"): 6,
    ("D", "ring-1-heavy"): 13,
    ("D", "round of 1"): 39,
    ("D", "round of 1024"): 989,
    ("E", "heavy"): 36,
    ("E", "round of 1024"): 1908,
}
