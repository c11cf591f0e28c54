"""ZCG_FLAG_XZ_RING_32K: the xz decoder with 32 KiB of LDS history must give
the same bytes and statuses as the default 4 KiB history (xz.rs:34-43 ->
liblzma), on long-distance data, all check types and truncated streams."""
import lzma

import numpy as np
import pytest

from gpu_check import decode
from zarr_amd._native import FLAG_XZ_RING_32K

pytestmark = pytest.mark.gpu


def _data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "far":  # repeats 4-60 KiB back: matches beyond both histories
        base = rng.integers(0, 256, 65536, dtype=np.uint8)
        out = np.empty(n, np.uint8)
        p = 0
        while p < n:
            d = int(rng.integers(4096, 61440))
            ln = min(int(rng.integers(8, 300)), n - p)
            src = base if p < d else out[p - d:p - d + ln]
            out[p:p + ln] = src[:ln] if p >= d else base[:ln]
            p += ln
        return out
    return (np.cumsum(rng.integers(-2, 3, n)) % 97).astype(np.uint8)


@pytest.mark.parametrize("kind", ["far", "walk"])
@pytest.mark.parametrize("check", [lzma.CHECK_CRC64, lzma.CHECK_CRC32, lzma.CHECK_NONE])
def test_ring_32k_matches_default(kind, check):
    D = 1 << 20
    datas = [_data(kind, D, s) for s in range(4)]
    streams = [lzma.compress(d.tobytes(), format=lzma.FORMAT_XZ, check=check, preset=6) for d in datas]
    streams.append(streams[0][: len(streams[0]) // 2])  # truncated -> UnexpectedEof
    s0, o0 = decode("xz", streams, "u1", D, 0)
    s1, o1 = decode("xz", streams, "u1", D, FLAG_XZ_RING_32K)
    assert s0.tolist() == s1.tolist()
    assert s0[:4].tolist() == [0, 0, 0, 0] and s0[4] == 1
    for i in range(4):
        assert np.array_equal(o0[i], datas[i]) and np.array_equal(o1[i], datas[i])
