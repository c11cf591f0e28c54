"""What the zlib codec's tests share.  The oracle is Python's zlib module: a
raw deflate body wrapped both ways (zlib stream, gzip member), the payloads,
one batch decode and one batch encode through _native, and the comparisons."""
import struct
import zlib

import numpy as np

from deflate_kit import PLAIN_HEADER, deflate
from golden_util import dtype_info
from zarr_amd import ArrayMetadata, Gzip, Zlib, _native

OK, EOF, INVALID_DATA, INVALID_INPUT, UNSUPPORTED, OUTPUT_TOO_SMALL = 0, 1, 2, 3, 4, 5
GUARD = 4096  # bytes of 0xAB behind each chunk's D bytes
KERNELS = {"default": 0, "wave": _native.FLAG_INFLATE_WAVE, "block_par": _native.FLAG_INFLATE_BLOCK_PAR,
           "serial": _native.FLAG_SERIAL_INFLATE}
HEADER = {0: b"\x78\x01", 1: b"\x78\x01", 2: b"\x78\x5e", 3: b"\x78\x5e", 4: b"\x78\x5e", 5: b"\x78\x5e",
          6: b"\x78\x9c", 7: b"\x78\xda", 8: b"\x78\xda", 9: b"\x78\xda"}


# ---- streams --------------------------------------------------------------------------------------
def adler_trailer(payload: bytes) -> bytes:
    return struct.pack(">I", zlib.adler32(payload))


def zlib_wrap(raw: bytes, payload: bytes = None, header: bytes = b"\x78\x9c") -> bytes:
    """A zlib stream around a raw deflate body; no trailer when payload is None."""
    return header + raw + (adler_trailer(payload) if payload is not None else b"")


def gzip_wrap_bare(raw: bytes) -> bytes:
    """A gzip member around the same body, without its trailer."""
    return PLAIN_HEADER + raw


def zlib_wbits(payload: bytes, wbits: int, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(payload) + c.flush()


# ---- payloads (n bytes each) ----------------------------------------------------------------------
def quant(n, seed=3):
    i = np.arange((n + 3) // 4 + 1)
    v = np.round(64 * (100 * np.sin(0.05 * (i + 7 * seed)) * np.cos(0.0003 * i) + (i & 3))) / 64
    return v.astype("<f4").tobytes()[:n]


def walk(n, seed=0):
    return np.cumsum(np.random.default_rng(seed).integers(-3, 4, n // 2 + 1)).astype("<i2").tobytes()[:n]


def text(n, seed=0):
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"chunk", b"array", b"zarr"]
    rng = np.random.default_rng(seed)
    out = b" ".join(words[k] for k in rng.integers(0, len(words), n // 3 + 8))
    return out[:n]


PAYLOADS = {"quant": quant, "walk": walk, "text": text}


def stream_bytes(payload: bytes, dt: str) -> bytes:
    """The payload is the chunk's bytes in STREAM order; this is what the
    decoded chunk holds in host-native order (and what encode is given)."""
    es, be, isb, _ = dtype_info(dt)
    a = np.frombuffer(payload, np.uint8)
    if isb:
        return (a != 0).astype(np.uint8).tobytes()
    if be and es > 1:
        return a.reshape(-1, es)[:, ::-1].tobytes()
    return payload


# ---- GPU calls ------------------------------------------------------------------------------------
def meta_for(dt, n, comp):
    return ArrayMetadata.new([n], [n], dt, comp)


def decode(streams, dt, n, flags=0, comp=None, guard=GUARD):
    """One zcg_decode_batch launch (n elements per chunk, 0 allowed); each
    destination is D + guard bytes pre-filled with 0xAB.  Returns (statuses,
    (N, D + guard) byte array)."""
    import ctypes
    import torch
    from zarr_amd.batch import PackedStreams
    from zarr_amd.chunk import abi_array
    stride = n * dtype_info(dt)[0] + guard
    dst = torch.full((max(len(streams) * stride, 1),), 0xAB, dtype=torch.uint8, device="cuda:0")
    packed = PackedStreams(streams, stride, "cuda:0", dst=dst)
    arr = abi_array(meta_for(dt, max(n, 1), comp if comp is not None else Zlib()), flags)
    arr.chunk_num_elements = n
    ctx = _native.context(0)
    r = ctx.lib.zcg_decode_batch(ctx.handle, ctypes.byref(arr), packed.desc.data_ptr(), packed.n,
                                 packed.status.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
    assert r == 0, r
    torch.cuda.synchronize()
    return packed.status.cpu().numpy().astype(int), packed.dst.cpu().numpy()[: len(streams) * stride].reshape(
        len(streams), stride)


def check_decode(streams, payloads, dt, flags=0, want=None, comp=None):
    """Statuses are `want` (default all OK); an OK chunk holds its payload under
    `dt`; the guard behind D is untouched whatever the status."""
    es = dtype_info(dt)[0]
    D = len(payloads[0])
    st, out = decode(streams, dt, D // es, flags, comp)
    want = [OK] * len(streams) if want is None else want
    for i in range(len(streams)):
        assert st[i] == want[i], (i, D, dt, hex(flags), st[i], want[i])
        if want[i] == OK:
            assert out[i, :D].tobytes() == stream_bytes(payloads[i], dt), (i, D, dt, hex(flags))
        assert (out[i, D:] == 0xAB).all(), (i, D, dt, hex(flags))
    return st, out


def encode(arrays, dt, comp, flags=0, cap_delta=0):
    """One zcg_encode_batch call over equal-sized chunks of host-native bytes;
    returns (statuses, [stream bytes])."""
    import torch
    from zarr_amd.batch import BatchCodec, make_encode_batch
    codec = BatchCodec(0)
    D, n = len(arrays[0]), len(arrays)
    meta = meta_for(dt, D // dtype_info(dt)[0], comp)
    elems = torch.from_numpy(np.frombuffer(b"".join(arrays), np.uint8).copy()).to("cuda:0")
    cap = codec.encode_bound(meta, D) + cap_delta
    desc, dst, out_len, status = make_encode_batch(elems, n, cap, "cuda:0")
    codec.encode(meta, desc, n, out_len, status, flags=flags)
    torch.cuda.synchronize()
    st, ol = status.cpu().numpy().astype(int), out_len.cpu().numpy()
    buf = dst.cpu().numpy().reshape(n, cap)
    return st, [buf[i, : ol[i]].tobytes() for i in range(n)]
