"""What the GPU decode-parity tests share: the payloads, the one-chunk check
through read_chunk, and the batch check (pack the streams, one launch per flag
set, compare every chunk with the oracle); and what the encode tests share:
one encode call over a batch, and the check of a gzip member against zlib.  Every expected output comes from
the oracle (oracle/zref.c over the reference's own C codec libraries).
"""
import functools
import struct
import zlib

import numpy as np

import zref
from deflate_kit import deflate, first_difference
from golden_util import CODEC_IDS, DEFAULT_PARAM, dtype_info
from zarr_amd import ArrayMetadata, DefaultChunk, Gzip, Lz4, Raw, ZarrIOError, _native
from zarr_amd.compression import Bzip2, Xz

COMP = {"raw": lambda p: Raw(), "gzip": lambda p: Gzip(p), "lz4": lambda p: Lz4(p),
        "bzip2": lambda p: Bzip2(p), "xz": lambda p: Xz(p)}
KIND = {zref.OK: "Ok", zref.EOF: "UnexpectedEof", zref.INVALID_DATA: "InvalidData"}
SHORT = {"ok": "Ok", "eof": "UnexpectedEof", "invalid": "InvalidData"}  # the names in lz4_cases.py and xz_cases.py
GUARD = 4096  # bytes of 0xAB behind each chunk's D bytes in the guarded checks


def meta_for(codec, dt, n, param=None):
    p = DEFAULT_PARAM[codec] if param is None else param
    return ArrayMetadata.new([n], [n], dt, COMP[codec](p))


# ---- payloads -------------------------------------------------------------------------------------
def rw(n, seed=0):
    return np.cumsum(np.random.default_rng(seed).integers(-3, 4, n)).astype("<i2")


def quant_f32(seed=0):
    i = np.arange(256)[:, None, None]
    j = np.arange(256)[None, :, None]
    k = np.arange(4)[None, None, :]
    phi = seed * 7
    v = np.round(64 * (100 * np.sin(0.05 * (i + phi)) * np.cos(0.03 * j) + k)) / 64
    return v.astype("<f4").reshape(-1)


DATASETS = {
    "randwalk_i2": lambda: rw(524288).tobytes(),
    "quant_f4": lambda: quant_f32(3).tobytes(),
    "uniform_u1": lambda: np.random.default_rng(5).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes(),
    "zeros": lambda: bytes(1 << 20),
    "text_like": lambda: (b"the quick brown fox jumps over the lazy dog %d\n" * 30000)[: 1 << 20],
}


# ---- one chunk through read_chunk -----------------------------------------------------------------
def gpu_decode(codec, stream, dt, n, param=None, flags=0):
    """read_chunk on the GPU; returns (kind or 'Ok', host-native bytes)."""
    es, be, isb, npdt = dtype_info(dt)
    meta = meta_for(codec, dt, n, param)
    try:
        ch = DefaultChunk.read_chunk(stream, meta, [0], npdt, flags=flags)
    except ZarrIOError as e:
        return e.kind, b""
    return "Ok", ch.get_data().tobytes()


def check(codec, stream, dt, n, param=None):
    """A one-chunk gzip read runs the 256-lane kernel by default (small batch);
    every gzip check also forces the one-wave-per-chunk kernel (the C2 kernel)."""
    es, be, isb, _ = dtype_info(dt)
    st, ref = zref.decode(CODEC_IDS[codec], stream, n * es, es, be, isb)
    for flags in ((0, _native.FLAG_INFLATE_WAVE) if codec == "gzip" else (0,)):
        kind, out = gpu_decode(codec, stream, dt, n, param, flags)
        assert kind == KIND[st], (kind, st, flags)
        if st == zref.OK:
            assert out == ref, flags


# ---- a batch: one launch per flag set ---------------------------------------------------------------
def decode(codec, streams, dt, n, flags, param=None, guard=0):
    """One batch launch.  With `guard`, each chunk's destination is D + guard
    bytes pre-filled with 0xAB (dst_cap is then D + guard in the kernels);
    without, PackedStreams allocates the D bytes per chunk and leaves them
    unfilled.  Returns the host statuses and an (N, D + guard) byte array."""
    import torch
    from zarr_amd.batch import BatchCodec, PackedStreams
    stride = n * dtype_info(dt)[0] + guard
    dst = torch.full((len(streams) * stride,), 0xAB, dtype=torch.uint8, device="cuda:0") if guard else None
    packed = PackedStreams(streams, stride, "cuda:0", dst=dst)
    BatchCodec(0).decode(meta_for(codec, dt, n, param), packed, flags=flags)
    torch.cuda.synchronize()
    return packed.status.cpu().numpy(), packed.dst.cpu().numpy().reshape(len(streams), stride)


def _oracle(codec, streams, D, dt):
    es, be, isb, _ = dtype_info(dt)
    st, out = zref.decode_batch(CODEC_IDS[codec], [np.frombuffer(s, np.uint8) for s in streams], D,
                                elem_size=es, big_endian=be, is_bool=isb)
    return [KIND[int(x)] for x in st], [o.tobytes() for o in out]


_oracle_once = functools.lru_cache(maxsize=None)(_oracle)


def oracle(codec, streams, dt, n, cache=False):
    """The oracle's (kinds, D bytes per stream) of a batch.  `cache` keeps the
    answer for the session (the craft suites ask for one batch under every flag
    set); the large corruption sweeps must not, they would pin tens of MiB."""
    return (_oracle_once if cache else _oracle)(codec, tuple(streams), n * dtype_info(dt)[0], dt)


def check_many(codec, streams, dt, n, flags=0, param=None, guard=0, want=None, expect=None, names=None,
               cache=False, ref=None):
    """Batch decode of many streams under one flag set or each of a list (one
    launch each, so sweeps of corruptions stay fast).  Per stream the status
    kind is the oracle's, an Ok chunk has the oracle's bytes, and with `guard`
    the bytes behind D are still 0xAB whatever the status.
      want    the kinds the oracle itself must give (asserted first; KIND or SHORT names)
      expect  the kinds the GPU must give where they are not the oracle's (a verify flag)
      names   labels for the messages instead of the stream index
      ref     the oracle's answer, for a caller that has asked already
    Returns the oracle's kinds."""
    D = n * dtype_info(dt)[0]
    kinds, outs = ref if ref is not None else oracle(codec, streams, dt, n, cache)
    if want is not None:
        assert kinds == [SHORT.get(w, w) for w in want], (D, dt, kinds)
    exp = kinds if expect is None else list(expect)
    for f in ((flags,) if isinstance(flags, int) else flags):
        st, out = decode(codec, streams, dt, n, f, param, guard)
        for i in range(len(streams)):
            at = (names[i] if names else i, D, dt, hex(f))
            assert KIND.get(int(st[i]), int(st[i])) == exp[i], at + (int(st[i]), exp[i])
            if exp[i] == "Ok":
                assert out[i, :D].tobytes() == outs[i], at
            assert (out[i, D:] == 0xAB).all(), at
    return kinds


# ---- encode: one zcg_encode_batch call, and the gzip member check ---------------------------------
def encode_batch(meta, arrays, cap_extra=0, src_lens=None):
    """zcg_encode_batch over device buffers; returns (status, [bytes]).
    `src_lens`: {chunk index: src_len} for descriptors that say less than D."""
    import torch
    from zarr_amd.batch import BatchCodec, make_encode_batch
    codec = BatchCodec(0)
    D = arrays[0].nbytes
    n = len(arrays)
    host = np.concatenate([a.view(np.uint8).reshape(-1) for a in arrays]) if D else np.zeros(1, np.uint8)
    elems = torch.from_numpy(host).to("cuda:0")
    cap = codec.encode_bound(meta, D) + cap_extra
    desc, dst, out_len, status = make_encode_batch(elems, n, cap, "cuda:0") if D else (None,) * 4
    if not D:  # zero-byte chunks: descriptors by hand
        desc, dst, out_len, status = make_encode_batch(torch.zeros(n, dtype=torch.uint8, device="cuda:0"),
                                                       n, cap, "cuda:0")
        d = desc.cpu().numpy().view(np.uint64).reshape(n, 4).copy()
        d[:, 1] = 0
        desc = torch.from_numpy(d.view(np.int64)).to("cuda:0")
    if src_lens:
        d = desc.cpu().numpy().view(np.uint64).reshape(n, 4).copy()
        for i, v in src_lens.items():
            d[i, 1] = v
        desc = torch.from_numpy(d.view(np.int64)).to("cuda:0")
    codec.encode(meta, desc, n, out_len, status)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    ol = out_len.cpu().numpy()
    buf = dst.cpu().numpy().reshape(n, cap)
    return st, [buf[i, : ol[i]].tobytes() for i in range(n)]


def zlib_raw(content: bytes, level: int) -> bytes:
    """flate2's deflate body: zlib raw deflate, windowBits -15, memLevel 8, default strategy."""
    return deflate(content, level)


def check_gzip_member(stream: bytes, content: bytes, level: int, exact=None):
    eff = 6 if (level < 0 or level > 9) else level
    xfl = 2 if eff >= 9 else (4 if eff <= 1 else 0)
    assert stream[:10] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, xfl, 255])
    crc, isize = struct.unpack_from("<II", stream, len(stream) - 8)
    assert crc == zlib.crc32(content) and isize == len(content) & 0xFFFFFFFF
    d = zlib.decompressobj(-15)
    assert d.decompress(stream[10:-8]) == content and d.eof and not d.unused_data
    if exact if exact is not None else eff >= 1:
        # levels 1-9: byte-identical to zlib (gzip.rs:54-56 -> flate2 -> zlib deflate_fast / deflate_slow)
        ref = zlib_raw(content, eff)
        body = stream[10:-8]
        if body != ref:
            k = next((i for i in range(min(len(body), len(ref))) if body[i] != ref[i]), min(len(body), len(ref)))
            raise AssertionError(f"gzip level {eff}: deflate body differs from zlib's at byte {k} "
                                 f"(len {len(body)} vs {len(ref)}): {first_difference(body, ref)}")
