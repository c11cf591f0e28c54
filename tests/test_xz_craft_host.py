"""Directed symbol-level LZMA2 / .xz streams on the CPU.  TEST INFRASTRUCTURE ONLY.

tests/xz_craft.py writes streams liblzma's encoder cannot (several blocks,
size fields, chunks that continue without a reset, dictionary resets in
mid-block, chosen symbols, distances and lengths); tests/xz_cases.py holds
the tables.  Here

  * the writer is pinned against liblzma: streams of the reference encoder and
    of Python's lzma are parsed into symbols and written again, byte for byte,
    and the model gives their payload;
  * every case gets the status its table names from the reference decoder, an
    "ok" case the bytes of the plain model, and the host build of the decode
    core (zcg_xz_core.h, the source the kernel runs) the same status and bytes;
  * the host core runs every case once more with every index of its IO
    counted: none may leave the output, the input or the probability model.
    That is the gate for tests/test_gpu_xz_craft.py, which imports the same
    tables and nothing else;
  * the census of the tables is pinned, with a model of the device's history
    ring for both ring sizes, so that a change to the writer, the tables or
    the kernel's constants cannot silently move the cases off the branches
    they were written for.
"""
import ctypes
import lzma

import numpy as np
import pytest

import xz_cases as cs
import xz_craft as xc
import zref
from gpu_check import KIND, SHORT
from test_hostcore import host, host_xz

FAMILIES = "A B C D E F G H".split()


def host_xz_checked(s: bytes, D: int):
    """(status, bytes, indexes out of bounds) of the host core with a counting IO."""
    h = host()
    h.zh_xz_decode_checked.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p]
    h.zh_xz_decode_checked.restype = ctypes.c_int
    out = np.zeros(max(D, 1), np.uint8)
    a = np.frombuffer(s, np.uint8) if s else np.zeros(1, np.uint8)
    bad = ctypes.c_uint64(123)
    st = h.zh_xz_decode_checked(a.ctypes.data, len(s), out.ctypes.data, D, ctypes.byref(bad))
    return st, out[:D].tobytes(), bad.value


@pytest.mark.parametrize("family", FAMILIES)
def test_cases_against_oracle_model_and_host_core(family):
    seen = 0
    for name, (D, cases) in cs.batches().items():
        if cases[0].family != family:
            continue
        st, out = zref.decode_batch(zref.XZ, [np.frombuffer(c.frame, np.uint8) for c in cases], D)
        for c, s, o in zip(cases, st, out):
            seen += 1
            kind = KIND[int(s)]
            assert kind == SHORT[c.want], (c.name, D, kind, c.want)
            hs, ho = host_xz(c.frame, D)
            assert hs == int(s), (c.name, D, hs, int(s))
            cs_, co, bad = host_xz_checked(c.frame, D)
            assert (cs_, bad) == (int(s), 0), (c.name, D, cs_, bad)
            if kind != "Ok":
                continue
            assert ho == o.tobytes() and co == ho, c.name
            if c.exact:
                m = xc.model(c.spec, D)
                assert m is not None and len(m) == D and m == ho, c.name
    assert seen == CASES[family]


def test_counting_io_counts():
    """The counting IO is no dummy: an index at each bound passes, one past it
    is counted and clamped (the clamped write lands on byte 0)."""
    h = host()
    h.zh_xz_checked_selftest.restype = ctypes.c_uint64
    assert h.zh_xz_checked_selftest() == 3


def payloads():
    rng = np.random.default_rng(3)
    walk = np.cumsum(rng.integers(-3, 4, 12000)).astype("<i2").tobytes()
    runs = np.repeat(rng.integers(0, 4, 3000, dtype=np.uint8), rng.integers(1, 90, 3000))[:65536].tobytes()
    noise = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    return dict(walk=walk, runs=runs, noise=noise)


def reemit(s, payload):
    spec = xc.parse(s)
    assert xc.write(spec) == s
    assert xc.model(spec) == payload
    return spec


@pytest.mark.parametrize("preset", [0, 6, 9])
def test_writer_reproduces_liblzma_presets(preset):
    for name, p in list(payloads().items())[:2]:
        st, s = zref.encode(zref.XZ, preset, np.frombuffer(p, np.uint8))
        assert st == zref.OK
        reemit(s, p)
        reemit(lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC32, preset=preset), p)


@pytest.mark.parametrize("lclppb", [(3, 0, 2), (0, 4, 0), (4, 0, 4), (1, 3, 1), (2, 2, 3)])
def test_writer_reproduces_liblzma_variants(lclppb):
    lc, lp, pb = lclppb
    p = payloads()["walk"]
    for check in (lzma.CHECK_NONE, lzma.CHECK_CRC64, lzma.CHECK_SHA256):
        filt = [{"id": lzma.FILTER_LZMA2, "preset": 6, "lc": lc, "lp": lp, "pb": pb}]
        spec = reemit(lzma.compress(p, format=lzma.FORMAT_XZ, check=check, filters=filt), p)
        assert spec["blocks"][0]["chunks"][0][3]["props"] == lclppb


def test_writer_reproduces_stored_chunks_and_filters():
    noise, walk = payloads()["noise"], payloads()["walk"]
    # 64 KiB that liblzma cuts into: two stored chunks; a stored and an LZMA chunk; two LZMA chunks
    for p, want in ((noise, [("stored", 1), ("stored", 2)]),
                    (noise[:62000] + bytes(3536), [("stored", 1), ("lzma", 0xC0)]),
                    (walk[:3000] + noise[:62000] + walk[3000:3536], [("lzma", 0xE0), ("lzma", 0x80)])):
        spec = reemit(lzma.compress(p, format=lzma.FORMAT_XZ, preset=6), p)
        assert [(c[0], c[1]) for c in spec["blocks"][0]["chunks"]] == want
    filt = [{"id": lzma.FILTER_DELTA, "dist": 2}, {"id": lzma.FILTER_LZMA2, "preset": 6}]
    w = payloads()["walk"]
    spec = reemit(lzma.compress(w, format=lzma.FORMAT_XZ, filters=filt), w)
    assert spec["blocks"][0]["filters"] == (("delta", 2),)


def test_writer_helpers():
    assert xc.crc64(b"123456789") == 0x995DC9BBDF1939FA
    assert xc.vli(0) == b"\x00" and xc.vli(127) == b"\x7f" and xc.vli(128) == b"\x80\x01"
    assert [xc.dist_slot(d) for d in (0, 1, 3, 4, 5, 6, 7, 8, 95, 96, 127, 128, (1 << 20) - 1, 1 << 20, xc.EOPM)] == \
        [0, 1, 3, 4, 4, 5, 5, 6, 12, 13, 13, 14, 39, 40, 63]
    for slot in range(64):
        lo, hi = xc.slot_range(slot)
        assert xc.dist_slot(lo) == xc.dist_slot(hi) == slot and (slot == 0 or xc.slot_range(slot - 1)[1] == lo - 1)
    assert xc.props_byte(3, 0, 2) == 0x5D and xc.props_byte(8, 4, 4) == 224
    # the model declines what reaches before the dictionary, by chunk kind
    lz = xc.lzma
    assert xc.model_block([lz(0xE0, [("lit", 65), ("match", 1, 3)])]) == b"AAAA"
    assert xc.model_block([lz(0xE0, [("lit", 65), ("match", 2, 3)])]) is None
    assert xc.model_block([xc.stored(1, b"ab"), lz(0xC0, [("match", 2, 3)])]) == b"ababa"
    assert xc.model_block([xc.stored(1, b"ab"), lz(0xE0, [("lit", 1), ("match", 2, 3)])]) is None
    assert xc.model_block([xc.stored(1, b"ab"), xc.stored(1, b"c"), lz(0xC0, [("match", 2, 3)])]) is None
    assert xc.model_block([lz(0xE0, [("lit", 1), ("lit", 2), ("match", 2, 2), ("match", 1, 2), ("rep", 1, 2)])]) == \
        bytes([1, 2, 1, 2, 2, 2, 2, 2])


def test_census():
    cen = cs.census()
    assert cen["cases"] == CASES and cen["want"] == WANT
    kinds = ("lit", "match", "rep", "srep")
    assert {p for p in cen["pairs"] if p[1] in kinds} == {(st, k) for st in range(12) for k in kinds}
    assert cen["first_diff"] == {None, 0, 1, 2, 3, 4, 5, 6, 7} and cen["rep_k"] == {0, 1, 2, 3}
    assert cen["slots"] == set(range(41)) | {62, 63} and cen["len_ctx"] == {0, 1, 2, 3}
    every = {(n, ps, pb) for pb in range(5) for ps in range(1 << pb) for n in cs.LENGTHS}
    assert every <= cen["match_len"] and every <= cen["rep_len"]
    assert {(c, lp, lc) for lc, lp in cs.LCLP for c in range(1 << lp)} <= cen["lit_ctx"]
    assert {(lc, lp, pb) for lc, lp in cs.LCLP for pb in range(5)} <= cen["props"]
    # the control table: every row is a case, and the rules of the format give its kind
    by_name = {c.name: c for c in cs.all_cases()}
    assert len(cs.CONTROL_TABLE) == 30
    for (prev, ctl), want in cs.CONTROL_TABLE.items():
        legal = (ctl in (0x01, 0xE0) if prev in ("first", "block2") else ctl not in (0x80, 0xA0) if prev == 0x01 else True)
        assert want == ("ok" if legal else "invalid")
        assert by_name["F-%s-then-%02X" % (prev if isinstance(prev, str) else "%02X" % prev, ctl)].want == want
    assert all(by_name["F-control-%02X" % ctl].want == "invalid" for ctl in range(3, 0x80))
    # a batch: one D, at most 64 streams
    for name, (D, cases) in cs.batches().items():
        assert len(cases) <= 64 and {c.D for c in cases} == {D} and len({c.family for c in cases}) == 1, name
    assert len(cs.batches()) == 49 and sum(D > cs.MAIN for D, _ in cs.batches().values()) == 1


@pytest.mark.parametrize("R", cs.RINGS)
def test_ring_census(R):
    """The device's ring (zcg_xz.hip: put, copy, copy_in, flush with XZ_RING = R,
    in_ring's 512 margin, the R / 2 trigger) modelled over every valid case.
    If this fails after one of those constants moved, move RINGS, MARGIN and
    PIECE in tests/xz_cases.py (family E is built from them), then these numbers."""
    cen = cs.ring_census(R)
    assert cen["unsafe"] == 0                     # no source is read from HBM at or above gfl
    for key in ("copy-ring", "copy-hbm", "copy-split", "back-ring", "back-hbm", "trigger-1", "trigger+0", "trigger+1",
                "wrap-in-copy-ring", "wrap-in-copy-hbm", "wrap-in-copy-split", "put-flush", "copy_in-flush",
                "copy_in-trigger-1", "copy_in-trigger+0", "copy_in-trigger+1"):
        assert cen[key] > 0, key
    assert cen == RING[R]


# the tables' own numbers
CASES = {"A": 17, "B": 40, "C": 12, "D": 25, "E": 310, "F": 300, "G": 77, "H": 756}
WANT = {("A", "ok"): 12, ("A", "invalid"): 5, ("B", "ok"): 40, ("C", "ok"): 7, ("C", "invalid"): 5, ("D", "ok"): 12,
        ("D", "invalid"): 13, ("E", "ok"): 310, ("F", "ok"): 26, ("F", "invalid"): 274, ("G", "ok"): 30,
        ("G", "invalid"): 47, ("H", "ok"): 349, ("H", "invalid"): 226, ("H", "eof"): 181}
# copies and short-rep / matched-literal reads by where their sources lie, copies at the flush
# trigger (pos + len - gfl - R / 2), stored pieces at it, flushes by what set them off
RING = {
    4096: {"back-hbm": 391, "back-ring": 3329, "copy-hbm": 290, "copy-ring": 3660, "copy-split": 74,
           "copy_in-flush": 16855, "copy_in-trigger+0": 7345, "copy_in-trigger+1": 1754, "copy_in-trigger-1": 41,
           "overlap": 1803, "put-flush": 72, "trigger+0": 307, "trigger+1": 41, "trigger-1": 27, "unsafe": 0,
           "wrap-in-copy": 192, "wrap-in-copy-hbm": 59, "wrap-in-copy-ring": 116, "wrap-in-copy-split": 17},
    32768: {"back-hbm": 117, "back-ring": 3603, "copy-hbm": 21, "copy-ring": 3918, "copy-split": 85,
            "copy_in-flush": 1691, "copy_in-trigger+0": 715, "copy_in-trigger+1": 182, "copy_in-trigger-1": 65,
            "overlap": 1803, "put-flush": 39, "trigger+0": 25, "trigger+1": 30, "trigger-1": 25, "unsafe": 0,
            "wrap-in-copy": 53, "wrap-in-copy-hbm": 1, "wrap-in-copy-ring": 35, "wrap-in-copy-split": 17},
}
