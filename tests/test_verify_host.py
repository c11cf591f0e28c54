"""The verify flags on the host side: the Python constants against the C
header, the `flags` keywords of the storage / region layer down to the ABI
descriptor, and the pure-Python XXH32 the GPU test builds its frames with."""
import importlib.util
import inspect
import os
import re
import struct

import numpy as np

import zref
from zarr_amd import ArrayMetadata, Gzip, _native, region, storage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("verify_gpu_cases", os.path.join(ROOT, "tests", "test_gpu_verify.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_values_match_the_header():
    with open(os.path.join(ROOT, "include", "zchunk_gpu.h")) as f:
        defs = dict(re.findall(r"#define (ZCG_FLAG_\w+) (0x[0-9a-fA-F]+)u", f.read()))
    assert _native.FLAG_VERIFY_GZIP_TRAILER == int(defs["ZCG_FLAG_VERIFY_GZIP_TRAILER"], 16) == 0x1
    assert _native.FLAG_VERIFY_LZ4_CONTENT == int(defs["ZCG_FLAG_VERIFY_LZ4_CONTENT"], 16) == 0x2
    assert _native.FLAG_VERIFY == _native.FLAG_VERIFY_GZIP_TRAILER | _native.FLAG_VERIFY_LZ4_CONTENT
    assert len(set(int(v, 16) for v in defs.values())) == len(defs)  # no two flags share a bit


def test_flags_keywords_exist():
    for fn in (storage.store_read, storage.store_read_device, storage.FilesystemHierarchy.read_chunk,
               storage.FilesystemHierarchy.read_chunk_into, storage.FilesystemHierarchy.read_chunks,
               region.read_ndarray, region.read_ndarray_into):
        p = inspect.signature(fn).parameters
        assert "flags" in p and p["flags"].default == 0, fn
    assert "flags" not in inspect.signature(region.write_ndarray).parameters  # its read-modify-write stays plain


class _FakeLib:
    def __init__(self):
        self.flags = []

    def _call(self, handle, arr, n, paths, dsts, status, io_threads):
        self.flags.append(int(arr._obj.compression.flags))
        return _native.OK

    zcg_store_read_chunks = _call
    zcg_store_read_chunks_device = _call


class _FakeCtx:
    handle = None
    device = 0

    def __init__(self):
        self.lib = _FakeLib()

    def last_error(self):
        return ""


def test_flags_reach_the_abi_descriptor(monkeypatch, tmp_path):
    ctx = _FakeCtx()
    monkeypatch.setattr(_native, "context", lambda device=0: ctx)
    monkeypatch.setattr(_native, "store_path", lambda root, key: (_native.OK, os.path.join(root, key.lstrip("/"))))
    meta = ArrayMetadata.new([8], [4], "<i2", Gzip(6))
    storage.store_read(meta, ["a", "b"], np.int16, flags=_native.FLAG_VERIFY)
    storage.store_read(meta, ["a"], np.int16)
    storage.store_read_device(meta, ["a"], [0], flags=_native.FLAG_VERIFY_GZIP_TRAILER)
    h = storage.FilesystemHierarchy(str(tmp_path), {})
    h.read_chunks("x", meta, [[0], [1]], np.int16, flags=_native.FLAG_VERIFY_LZ4_CONTENT)
    h.read_chunk("x", meta, [0], np.int16, flags=_native.FLAG_VERIFY)
    h.read_chunk("x", meta, [1], np.int16)
    assert ctx.lib.flags == [3, 0, 1, 2, 3, 0]


def test_python_xxh32_matches_an_encoded_frame():
    mod = _gpu_test_module()
    for n in (0, 1, 15, 16, 17, 100, 5000):
        data = np.random.default_rng(n).integers(0, 256, n).astype(np.uint8).tobytes()
        frame = zref.lz4_frame_custom(data, content_checksum=True)
        assert struct.unpack("<I", frame[-4:])[0] == mod.xxh32(data), n
        assert frame[6] == (mod.xxh32(frame[4:6]) >> 8) & 0xFF  # the header checksum byte
    p = mod.text(3000, 1)
    st, s = zref.encode(zref.LZ4, 65536, np.frombuffer(p, np.uint8))
    assert st == zref.OK and struct.unpack("<I", s[-4:])[0] == mod.xxh32(p)
