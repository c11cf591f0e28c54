"""Directed blocks through the GPU LZ4 encoder (zcg_lz4_enc.hip): liblz4's
frame, byte for byte.

A wave-parallel search that is wrong still writes a stream that decodes; only
the comparison with liblz4 on a block that reaches the branch tells.  The
batches of tests/lz4_enc_cases.py reach le_block's batch cut (a stale table
value behind it, deferred matches, short and empty last batches), the table
mode by block length, the 65 535 distance limit at both of its sites, catch-up
past 64 bytes, the three return-0 sites and their neighbours, the length
fields' edges, LZ4_count's lanes and byte-wise tail, rematch chains,
lz4_frame_finalize's compaction and lz4_content_xxh32's stripes and tails;
each has a witness asserted on the CPU (tests/test_lz4_enc_cases_host.py).

Here each case is one zcg_encode_batch call; every frame must equal the
oracle's liblz4 LZ4F frame and decode on the GPU.  A case whose length is a
multiple of 8 runs again as a big-endian u64 array holding the same stream
(the kernels then read every byte through the dtype transform), and a case of
0 / 1 bytes as a bool array.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

zref = pytest.importorskip("zref")

import lz4_enc_cases as ec  # noqa: E402
from golden_util import dtype_info  # noqa: E402
from gpu_check import encode_batch, meta_for  # noqa: E402
from zarr_amd import DefaultChunk  # noqa: E402

INVALID_DATA = 2  # ZCG_ERR_INVALID_DATA


def _expected(c):
    out = []
    for chunk in c.chunks:
        st, ref = zref.encode(zref.LZ4, c.B, np.frombuffer(chunk, np.uint8))
        assert st == zref.OK
        out.append(ref)
    return out


def _run(c, dt, sources):
    es, _, isb, npdt = dtype_info(dt)
    meta = meta_for("lz4", dt, c.D // es, c.B)
    short = {i: v - v % es for i, v in c.short.items()}
    st, outs = encode_batch(meta, [np.frombuffer(x, np.uint8) for x in sources], src_lens=short)
    for i, (got, ref, content) in enumerate(zip(outs, _expected(c), c.chunks)):
        if i in c.short:
            assert st[i] == INVALID_DATA and got == b"", (c.name, dt, i, int(st[i]))
            continue
        assert st[i] == 0, (c.name, dt, i, st.tolist())
        if got != ref:
            k = next((j for j in range(min(len(got), len(ref))) if got[j] != ref[j]), min(len(got), len(ref)))
            raise AssertionError(f"{c.name} as {dt} chunk {i}: lz4 frame differs from liblz4's at byte {k} "
                                 f"(len {len(got)} vs {len(ref)})")
        back = DefaultChunk.read_chunk(got, meta, [0], npdt).get_data()
        want = np.frombuffer(content, np.uint8).astype(bool) if isb else np.frombuffer(content, dt).astype(npdt)
        assert np.array_equal(back.reshape(-1), want), (c.name, dt, i)


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_case(name):
    c = ec.case(name)
    _run(c, "u1", c.chunks)


@pytest.mark.parametrize("name", [c.name for c in ec.all_cases() if c.D % 8 == 0])
def test_case_big_endian_u64(name):
    """The same stream from a `>u8` array: the source holds each element byte-swapped."""
    c = ec.case(name)
    src = [np.frombuffer(x, np.uint8).reshape(-1, 8)[:, ::-1].tobytes() for x in c.chunks]
    _run(c, ">u8", src)


@pytest.mark.parametrize("name", [c.name for c in ec.all_cases() if c.is_bits()])
def test_case_bool(name):
    c = ec.case(name)
    _run(c, "bool", c.raw)
