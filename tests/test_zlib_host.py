"""The zlib codec on the host side (no GPU): the Python variant and its JSON,
the native metadata parser, the constants against the C header, and the codec
entry points of the ABI that need no device."""
import ctypes
import json
import os
import re
import zlib

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, CompressionType, Gzip, Zlib, _native
from zarr_amd.compression import CODEC_ZLIB, codec_param, to_abi_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_json_round_trip():
    for comp, doc in ((Zlib(), {"codec": "zlib", "configuration": {"level": -1}}),
                      (Zlib(4), {"codec": "zlib", "configuration": {"level": 4}})):
        assert CompressionType.to_json(comp) == doc
        assert CompressionType.from_json(doc) == comp
    assert CompressionType.from_json({"codec": "zlib"}) == Zlib(-1)
    assert CompressionType.from_json({"codec": "zlib", "configuration": None}) == Zlib(-1)
    meta = ArrayMetadata.new([12, 10], [4, 5], "<i2", Zlib(7))
    assert ArrayMetadata.from_json(meta.to_json()).compressor == Zlib(7)


def test_from_str_display_and_levels():
    assert CompressionType.from_str("zlib") == Zlib() == CompressionType.from_str("ZLIB")
    assert CompressionType.Zlib is Zlib and CompressionType.display(Zlib()) == "Zlib"
    assert [Zlib(l).effective_level() for l in (-1, 0, 1, 9, 10)] == [6, 0, 1, 9, 6]
    assert Zlib(3) != Gzip(3)


def test_abi_fields_carry_the_level_in_gzip_level():
    assert CODEC_ZLIB == 5 == Zlib.codec_id
    f = to_abi_fields(Zlib(4))
    assert f["codec"] == 5 and f["gzip_level"] == 4
    assert to_abi_fields(Zlib())["gzip_level"] == -1
    assert codec_param(Zlib(8)) == 8


@pytest.mark.parametrize("doc,level", [({"codec": "zlib", "configuration": {"level": 4}}, 4),
                                       ({"codec": "zlib"}, -1),
                                       ({"codec": "zlib", "configuration": None}, -1),
                                       ({"codec": "zlib", "configuration": {}}, -1)])
def test_native_parser(doc, level):
    text = json.dumps({"shape": [12, 10], "chunk_grid": {"type": "regular", "chunk_shape": [4, 5], "separator": "/"},
                       "data_type": "<i2", "chunk_memory_layout": "C", "compressor": doc, "fill_value": None,
                       "extensions": [], "attributes": {}})
    st, m, err = _native.array_meta_from_json(text)
    assert st == 0, err
    assert m.array.compression.codec == 5 and m.array.compression.gzip_level == level
    # and the Python parser agrees
    assert ArrayMetadata.from_json(text).compressor == Zlib(level)


def test_constants_match_the_header():
    with open(os.path.join(ROOT, "include", "zchunk_gpu.h")) as f:
        src = f.read()
    defs = dict(re.findall(r"#define (ZCG_FLAG_\w+) (0x[0-9a-fA-F]+)u", src))
    assert _native.FLAG_VERIFY_ZLIB_TRAILER == int(defs["ZCG_FLAG_VERIFY_ZLIB_TRAILER"], 16) == 0x8
    assert _native.FLAG_VERIFY_ALL == 0xB == _native.FLAG_VERIFY | _native.FLAG_VERIFY_ZLIB_TRAILER
    assert _native.FLAG_VERIFY == 0x3
    assert len(set(int(v, 16) for v in defs.values())) == len(defs)  # no two flags share a bit
    assert int(re.search(r"ZCG_CODEC_ZLIB = (\d+)", src).group(1)) == CODEC_ZLIB
    assert re.search(r"#define ZCG_ABI_VERSION 1\b", src)


def test_codec_on_gpu_both_directions():
    L = _native.load_library()
    assert L.zcg_codec_on_gpu(5, 0) == 1 and L.zcg_codec_on_gpu(5, 1) == 1
    assert L.zcg_codec_on_gpu(6, 0) == 0


@pytest.mark.parametrize("n", [1, 65535, 65536])
def test_encode_bound_covers_stored_streams(n):
    L = _native.load_library()
    x = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    c = _native.Compression(5, 0, 65536, 9, 6, 0)
    g = _native.Compression(2, 0, 65536, 9, 6, 0)
    bound = int(L.zcg_encode_bound(ctypes.byref(c), n))
    assert bound >= len(zlib.compress(x, 0))
    assert bound == int(L.zcg_encode_bound(ctypes.byref(g), n)) - 12  # the frame's 6 bytes in place of 18
