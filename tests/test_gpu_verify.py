"""Opt-in checksum verification on decode (ZCG_FLAG_VERIFY_GZIP_TRAILER,
ZCG_FLAG_VERIFY_LZ4_CONTENT; rules in include/zchunk_gpu.h).

There is no oracle for the verify verdict (the reference never reads the
trailers), so every case states its expected status by construction, and first
asserts through the oracle what the status is WITHOUT verification: the
"silent" cases are Ok there, which is what the feature is for.  Good chunks
must also match the oracle's bytes, and the 0xAB guard after the D decoded
bytes must stay intact.  Streams are packed with a D + GUARD stride (odd for
odd D, so destinations are misaligned), one batch launch per flag set.
"""
import struct
import zlib

import numpy as np
import pytest

import zref
from deflate_kit import PLAIN_HEADER, deflate, flip, member, noise, stored, text
from golden_util import dtype_info
from gpu_check import GUARD, check_many, decode, oracle
from lz4_craft import xxh32
from zarr_amd import ArrayMetadata, DefaultChunk, FilesystemHierarchy, Gzip, Lz4, SliceDataChunk, _native
from zarr_amd.chunk import ZarrIOError, abi_array

pytestmark = pytest.mark.gpu

VG, VL = _native.FLAG_VERIFY_GZIP_TRAILER, _native.FLAG_VERIFY_LZ4_CONTENT
GZ_SETS = (0, _native.FLAG_SERIAL_INFLATE, _native.FLAG_INFLATE_BLOCK_PAR, _native.FLAG_INFLATE_WAVE)
LZ_SETS = (0, _native.FLAG_LZ4_WAVE_PER_BLOCK, _native.FLAG_LZ4_LANE_PER_BLOCK)
DTYPES = ["u1", ">u2", ">f4", ">u8", "bool"]
OK, EOF, BAD = "Ok", "UnexpectedEof", "InvalidData"


# ---- builders (this file's streams: zlib at memLevel 9, text() with 8 spare words) ---------------
def lz4_stored_frame(blocks, content_checksum=True, content_size=None, end_mark=True):
    """An LZ4 frame of stored (uncompressed) blocks, independent, 64 KiB block maximum."""
    flg = 0x60 | (0x04 if content_checksum else 0) | (0x08 if content_size is not None else 0)
    desc = bytes([flg, 0x40]) + (struct.pack("<Q", content_size) if content_size is not None else b"")
    out = struct.pack("<I", 0x184D2204) + desc + bytes([(xxh32(desc) >> 8) & 0xFF])
    for b in blocks:
        out += struct.pack("<I", len(b) | 0x80000000) + b
    if end_mark:
        out += struct.pack("<I", 0)
        if content_checksum:
            out += struct.pack("<I", xxh32(b"".join(blocks)))
    return out


def flip_first_literal(frame, data_at=11):
    """One bit of the first literal of a frame's first (compressed) block."""
    assert not struct.unpack_from("<I", frame, data_at - 4)[0] & 0x80000000
    i = data_at + 1
    assert frame[data_at] >> 4 >= 1  # the block starts with literals
    if frame[data_at] >> 4 == 15:    # length bytes first
        while frame[i] == 255:
            i += 1
        i += 1
    return flip(frame, i)


def lz4_frame(payload):
    st, s = zref.encode(zref.LZ4, 65536, np.frombuffer(payload, np.uint8))
    assert st == zref.OK and s[4] == 0x64
    return s


# ---- the check ----------------------------------------------------------------------------------
def check_group(codec, cases, dt, n, flag_sets=None):
    """cases: [(stream, status without verification, status with)].  The oracle
    must give the first; every flag set OR-ed with the codec's verify flag the
    second (and the oracle's bytes for Ok chunks); the other codec's verify
    flag must change nothing against a plain decode."""
    streams = [c[0] for c in cases]
    ref = oracle(codec, streams, dt, n)
    assert ref[0] == [c[1] for c in cases], (n, dt, ref[0])
    mine, other = (VG, VL) if codec == "gzip" else (VL, VG)
    sets = flag_sets if flag_sets is not None else (GZ_SETS if codec == "gzip" else LZ_SETS)
    st0, out0 = decode(codec, streams, dt, n, 0, guard=GUARD)
    st1, out1 = decode(codec, streams, dt, n, other, guard=GUARD)
    assert st0.tolist() == st1.tolist() and out0.tobytes() == out1.tobytes(), (n, dt, st0.tolist(), st1.tolist())
    check_many(codec, streams, dt, n, [f | mine for f in sets], guard=GUARD, expect=[c[2] for c in cases], ref=ref)


def payload_for(dt, D, seed):
    # bool: bytes above 1 must come out as 1, and the CRC is of the bytes as stored
    return noise(D, seed) if dt == "bool" else text(D, seed, spare=8)


# ---- gzip ---------------------------------------------------------------------------------------
GZ_SIZES = [1, 15, 16, 17, 4095, 65537]


@pytest.mark.parametrize("dt", DTYPES)
def test_gzip_valid_members(dt):
    es = dtype_info(dt)[0]
    for size in GZ_SIZES:
        n = (size + es - 1) // es if es > 1 and size > 17 else size
        p = payload_for(dt, n * es, 100 + size)
        cases = [(member(deflate(p, mem=9), p), OK, OK), (member(deflate(p, 0, mem=9), p), OK, OK),
                 (member(deflate(p, 6, zlib.Z_FIXED, mem=9), p), OK, OK)]
        check_group("gzip", cases, dt, n)


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_gzip_one_mib(dt):
    es = dtype_info(dt)[0]
    D = 1 << 20
    p = payload_for(dt, D, 7)
    good = member(deflate(p, mem=9), p)
    bad = member(deflate(p, mem=9), flip(p, D - 3))  # the trailer of another payload
    check_group("gzip", [(good, OK, OK), (bad, OK, BAD)], dt, D // es)


def fixed_literal_flip(payload):
    """A fixed-Huffman stream of `payload` with one bit flipped so that it still
    parses to the end and inflates to as many, but different, bytes."""
    raw = deflate(payload, 6, zlib.Z_FIXED, mem=9)
    for bit in range(40, len(raw) * 8 - 40):
        cand = flip(raw, bit // 8, 1 << (bit % 8))
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(cand)
        except zlib.error:
            continue
        if d.eof and not d.unused_data and len(out) == len(payload) and out != payload:
            return cand
    raise AssertionError("no parsing flip found")


def fancy_header():
    """FEXTRA + FNAME + FHCRC."""
    h = bytes([0x1f, 0x8b, 8, 4 | 8 | 2, 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 5) + b"extra" + b"name.bin\0"
    return h + struct.pack("<H", zlib.crc32(h) & 0xFFFF)


def gzip_cases(n, seed):
    """Every gzip case at one chunk size n (bytes)."""
    p = noise(n, seed, 144)  # literals 0..143: 8-bit fixed codes
    q = noise(n + 57, seed + 1)
    st_p = member(stored(p, True), p)
    empties = b"\x00\x00\x00\xff\xff" * 10000  # 50 000 bytes of empty stored blocks: past flate2's window
    sync = stored(p) + empties + stored(b"", True)
    second = member(deflate(text(500, 3, spare=8), mem=9), text(500, 3, spare=8))
    cases = [
        (st_p, OK, OK),
        (member(deflate(p, mem=9), p), OK, OK),
        (flip(st_p, 10 + 5 + n // 2), OK, BAD),                       # stored payload byte
        (member(fixed_literal_flip(p), p), OK, BAD),                  # fixed-Huffman literal
        (flip(st_p, len(st_p) - 8), OK, BAD),                         # CRC field
        (flip(st_p, len(st_p) - 2), OK, BAD),                         # ISIZE field
        (flip(st_p, len(st_p) - 4, 0x80), OK, BAD),
    ]
    cases += [(st_p[:-k], OK, EOF) for k in range(1, 9)]              # cut inside the trailer
    cases += [
        (member(stored(q[:n]) + stored(q[n:], True), q), OK, BAD),    # longer: n at a block boundary
        (member(deflate(q, 6, zlib.Z_FIXED, mem=9), q), OK, BAD),     # longer: Huffman tokens go on
        (member(stored(q, True), q), OK, BAD),                        # longer: inside a stored block
        (member(sync, p), OK, OK),
        (flip(member(sync, p), 10 + 5 + 7), OK, BAD),
        (st_p + second, OK, OK),                                      # a second member is ignored
        (flip(st_p, 10 + 5 + 1) + second, OK, BAD),
        (member(stored(p, True), p, fancy_header()), OK, OK),
        (flip(member(stored(p, True), p, fancy_header()), len(fancy_header()) + 5 + 2), OK, BAD),
        (st_p[:10 + 5 + n // 2], EOF, EOF),                           # already short
        (PLAIN_HEADER + b"\x07" + st_p[11:], BAD, BAD),               # block type 3
        (b"\x1f\x8c" + st_p[2:], BAD, BAD),                           # bad magic
        (member(deflate(p, 0, mem=9), p), OK, OK),
        (member(deflate(p, 9, zlib.Z_FIXED, mem=9), p), OK, OK),
    ]
    return cases


def test_gzip_mixed_batch_of_33():
    n = 3001
    cases = gzip_cases(n, 50)
    p = text(n, 9, spare=8)
    while len(cases) < 33:
        cases.append((member(deflate(p, mem=9), p), OK, OK))
    assert len(cases) == 33
    check_group("gzip", cases, "u1", n)


@pytest.mark.parametrize("dt", [">u2", "bool"])
def test_gzip_cases_with_element_transform(dt):
    check_group("gzip", gzip_cases(2048, 60), dt, 2048 // dtype_info(dt)[0])


def test_gzip_output_fills_inside_a_match():
    p = b"\0" * 1000
    m = member(deflate(p, mem=9), p)
    check_group("gzip", [(m, OK, BAD), (member(deflate(p[:100], mem=9), p[:100]), OK, OK)], "u1", 100)


# ---- LZ4 ----------------------------------------------------------------------------------------
LZ_SIZES = [1, 15, 16, 17, 65536, 131077]


@pytest.mark.parametrize("dt", DTYPES)
def test_lz4_valid_frames(dt):
    es = dtype_info(dt)[0]
    for size in LZ_SIZES:
        n = (size + es - 1) // es if es > 1 and size > 17 else size
        p = payload_for(dt, n * es, 200 + size)
        check_group("lz4", [(lz4_frame(p), OK, OK), (lz4_stored_frame([p[i:i + 65536] for i in range(0, len(p), 65536)]),
                                                     OK, OK)], dt, n)


@pytest.mark.parametrize("dt", [">f4", "bool"])
def test_lz4_one_mib(dt):
    es = dtype_info(dt)[0]
    D = 1 << 20
    p = payload_for(dt, D, 8)
    f = lz4_frame(p)
    check_group("lz4", [(f, OK, OK), (flip(f, len(f) - 1), OK, BAD)], dt, D // es)


def lz4_cases(n, seed):
    p = text(n, seed, spare=8)
    q = text(n + 100, seed + 1, spare=8)
    f = lz4_frame(p)
    r = noise(n, seed + 2)
    cases = [
        (f, OK, OK),
        (flip_first_literal(f), OK, BAD),                                  # a literal inside the block
        (flip(f, len(f) - 3), OK, BAD),                                    # checksum word
    ]
    cases += [(f[:-k], OK, EOF) for k in range(1, 5)]                      # cut inside the checksum
    cases += [
        (f[:-5], OK, EOF), (f[:-8], OK, EOF),                              # cut inside / before the EndMark
        (lz4_stored_frame([r], content_checksum=False), OK, OK),           # nothing to compare
        (flip(lz4_stored_frame([r], content_checksum=False), 15), OK, OK),
        (lz4_stored_frame([r], content_size=n), OK, OK),
        (lz4_stored_frame([r], content_size=n + 5), BAD, BAD),             # (LZ4F itself checks it at the EndMark)
        (flip(lz4_stored_frame([r], content_size=n), 7 + 8 + 4 + 9), OK, BAD),
        (lz4_stored_frame([r, r[:100]]), OK, BAD),                         # a further data block
        (lz4_frame(q), OK, BAD),                                           # the block decodes past n
        (f[:40], EOF, EOF),                                                # already short
        (b"\x05" + f[1:], BAD, BAD),                                       # bad magic
    ]
    return cases


def test_lz4_mixed_batch_of_33():
    n = 3001
    cases = lz4_cases(n, 70)
    p = text(n, 10, spare=8)
    while len(cases) < 33:
        cases.append((lz4_frame(p), OK, OK))
    assert len(cases) == 33
    check_group("lz4", cases, "u1", n)


@pytest.mark.parametrize("dt", [">u2", "bool"])
def test_lz4_cases_with_element_transform(dt):
    check_group("lz4", lz4_cases(2048, 80), dt, 2048 // dtype_info(dt)[0])


def test_lz4_linked_block_frame():
    n = 70000  # two linked blocks: the serial path
    p = text(n // 2, 90, spare=8)
    linked = zref.lz4_frame_custom(p + p, linked=True, content_checksum=True)
    assert linked[4] & 0x20 == 0
    bad = flip_first_literal(linked)
    check_group("lz4", [(linked, OK, OK), (bad, OK, BAD), (linked[:-2], OK, EOF)], "u1", n)


# ---- entry points -------------------------------------------------------------------------------
def test_read_chunk_flag():
    p = text(4000, 5, spare=8)
    good = member(stored(p, True), p)
    bad = flip(good, 100)
    meta = ArrayMetadata.new([4000], [4000], "u1", Gzip(-1))
    assert DefaultChunk.read_chunk(good, meta, [0], np.uint8, flags=_native.FLAG_VERIFY).get_data().tobytes() == p
    assert DefaultChunk.read_chunk(bad, meta, [0], np.uint8).get_data().tobytes() != p  # silent
    with pytest.raises(ZarrIOError) as e:
        DefaultChunk.read_chunk(bad, meta, [0], np.uint8, flags=_native.FLAG_VERIFY)
    assert e.value.kind == "InvalidData"


@pytest.mark.parametrize("comp", [Gzip(6), Lz4(65536)], ids=["gzip", "lz4"])
def test_hierarchy_chunk_corrupted_on_disk(tmp_path, comp):
    from zarr_amd.region import BoundingBox, read_ndarray
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    meta = ArrayMetadata.new([64, 64], [32, 64], "<i2", comp)
    h.create_array("a", meta)
    data = [np.arange(2048, dtype=np.int16) + 7 * g for g in range(2)]
    for g in range(2):
        h.write_chunk("a", meta, SliceDataChunk([g, 0], data[g]))
    box = BoundingBox([0, 0], [64, 64])
    a = read_ndarray(h, "a", meta, box, np.int16, flags=_native.FLAG_VERIFY)
    assert a.tolist() == read_ndarray(h, "a", meta, box, np.int16).tolist() and a[32:].any()
    path = h.chunk_path("a", meta, [1, 0])
    with open(path, "rb") as f:
        s = f.read()
    with open(path, "wb") as f:  # the checksum word: CRC32 of the gzip trailer, the LZ4 content checksum
        f.write(flip(s, len(s) - (8 if isinstance(comp, Gzip) else 4)))
    got = h.read_chunks("a", meta, [[0, 0], [1, 0]], np.int16)  # passes without the flag
    assert got[1].get_data().tolist() == data[1].tolist()
    read_ndarray(h, "a", meta, box, np.int16)
    with pytest.raises(ZarrIOError) as e:
        h.read_chunks("a", meta, [[0, 0], [1, 0]], np.int16, flags=_native.FLAG_VERIFY)
    assert e.value.kind == "InvalidData"
    with pytest.raises(ZarrIOError) as e:
        read_ndarray(h, "a", meta, box, np.int16, flags=_native.FLAG_VERIFY)
    assert e.value.kind == "InvalidData"


@pytest.mark.parametrize("codec", ["gzip", "lz4"])
def test_workspace_and_fresh_stream(codec):
    import ctypes
    import torch
    from zarr_amd.batch import BatchCodec, PackedStreams
    n = 5000
    meta = ArrayMetadata.new([n], [n], "u1", Gzip(-1) if codec == "gzip" else Lz4(65536))
    lib = _native.load_library()
    for extra in GZ_SETS if codec == "gzip" else LZ_SETS:
        plain = lib.zcg_workspace_bytes(ctypes.byref(abi_array(meta, extra)), 40, 0)
        ver = lib.zcg_workspace_bytes(ctypes.byref(abi_array(meta, extra | _native.FLAG_VERIFY)), 40, 0)
        assert ver >= plain and ver > 0
    p = text(n, 12, spare=8)
    good = member(deflate(p, mem=9), p) if codec == "gzip" else lz4_frame(p)
    bad = flip(good, len(good) - 1)
    s = torch.cuda.Stream()
    for flags in (_native.FLAG_SERIAL_INFLATE | _native.FLAG_VERIFY, _native.FLAG_VERIFY):
        packed = PackedStreams([good, bad], n, "cuda:0")
        BatchCodec(0).decode(meta, packed, stream=s, flags=flags)
        s.synchronize()
        assert packed.status.cpu().tolist() == [zref.OK, zref.INVALID_DATA]
        assert packed.dst[:n].cpu().numpy().tobytes() == p


@pytest.mark.parametrize("codec", ["gzip", "lz4"])
def test_capture_and_replay(codec):
    """The steady-state promise of zcg_decode_batch holds under the flags: no
    allocation, no host synchronisation, capturable after one warm-up call."""
    import torch
    from zarr_amd.batch import BatchCodec, PackedStreams
    n = 20000
    dt = ">u2"
    meta = ArrayMetadata.new([n // 2], [n // 2], dt, Gzip(-1) if codec == "gzip" else Lz4(65536))
    p, q = text(n, 13, spare=8), text(n, 14, spare=8)
    mk = (lambda x: member(deflate(x, mem=9), x)) if codec == "gzip" else lz4_frame
    streams = [mk(p), flip(mk(q), len(mk(q)) - 1), mk(q), mk(p)[:-2]]
    want = [zref.OK, zref.INVALID_DATA, zref.OK, zref.EOF]
    packed = PackedStreams(streams, n, "cuda:0")
    bc = BatchCodec(0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        bc.decode(meta, packed, flags=_native.FLAG_VERIFY)  # warm-up: the stream's workspace exists
    s.synchronize()
    eager_st, eager = packed.status.cpu().tolist(), packed.dst.cpu().numpy().copy()
    assert eager_st == want
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bc.decode(meta, packed, flags=_native.FLAG_VERIFY)
    for _ in range(2):
        packed.dst.fill_(0x55)
        packed.status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert packed.status.cpu().tolist() == eager_st
        got = packed.dst.cpu().numpy()
        for i in (0, 2):
            assert got[i * n:(i + 1) * n].tobytes() == eager[i * n:(i + 1) * n].tobytes()
