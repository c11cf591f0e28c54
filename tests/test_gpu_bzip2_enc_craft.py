"""Directed payloads through the GPU bzip2 encoder (zcg_bz2_enc.hip), every
stream taken apart and compared with the CPU model, by equality alone.

libbz2 decoding a stream says that the stream is right.  It does not say
which branches of the encoder wrote it: uniform bytes resolve in the first
radix sort, one run pattern meets one phase of the 64-byte RLE1 step, and no
generic payload has 5 tables or more than 256 blocks in a sort.  The batches
of tests/bz2_enc_cases.py are built to reach those branches, each with a
witness asserted on the CPU (tests/test_bz2_enc_cases_host.py) that it does.
Here each batch is one encode call, and per chunk

  * status 0, out_len within encode_bound, the 4 096 guard bytes behind the
    bound untouched;
  * libbz2 (Python's bz2 and the oracle) and the GPU decoder return the
    content;
  * the reader (tests/bz2_read.py) parses the stream, and check_stream
    compares every stage of every block with the model: the cuts fall
    between RLE1 pieces, within bmax and as late as they may; block and
    stream CRCs; L; origPtr (for a periodic text: among the positions of the
    rotations equal to it); symbol map and symbols; libbz2's table and
    selector counts; selectors and lengths in range.
"""
import bz2

import numpy as np
import pytest

import bz2_enc_cases as ec
from golden_util import dtype_info
from gpu_check import GUARD, check_many, meta_for, oracle

pytestmark = pytest.mark.gpu

ZCG_ERR_OUTPUT_TOO_SMALL = 5


def encode(meta, src, D, caps=None):
    """One encode call over chunks of D bytes, each with a destination of
    encode_bound bytes (dst_cap, or caps[i]) and GUARD bytes of 0xAB behind
    them.  Returns (status, out_len, destinations as an (n, bound + GUARD)
    array, bound)."""
    import torch
    from zarr_amd.batch import BatchCodec
    codec = BatchCodec(0)
    n = len(src)
    bound = codec.encode_bound(meta, D)
    stride = bound + GUARD
    elems = torch.from_numpy(np.frombuffer(b"".join(src), np.uint8).copy()).to("cuda:0")
    dst = torch.full((n * stride,), 0xAB, dtype=torch.uint8, device="cuda:0")
    desc = np.zeros((n, 4), np.uint64)
    desc[:, 0] = elems.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(D)
    desc[:, 1] = D
    desc[:, 2] = dst.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    desc[:, 3] = bound if caps is None else np.array(caps, np.uint64)
    d = torch.from_numpy(desc.view(np.int64)).to("cuda:0")
    out_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    codec.encode(meta, d, n, out_len, status)
    torch.cuda.synchronize()
    return status.cpu().numpy(), out_len.cpu().numpy(), dst.cpu().numpy().reshape(n, stride), bound


def run_case(name):
    case = ec.case(name)
    es, be, isb, _ = dtype_info(case.dt)
    D, n = case.D, len(case.chunks)
    assert D % es == 0
    meta = meta_for("bzip2", case.dt, D // es, case.level)
    src = case.src if case.src is not None else case.chunks
    st, ol, out, bound = encode(meta, src, D)
    assert (st == 0).all(), (name, np.flatnonzero(st != 0)[:10], st[st != 0][:10])
    assert (ol <= bound).all(), (name, int(ol.max()), bound)
    assert (out[:, bound:] == 0xAB).all(), name
    streams = [out[i, :ol[i]].tobytes() for i in range(n)]
    assert all((out[i, ol[i]:] == 0xAB).all() for i in range(n)), name
    for i, (s, content) in enumerate(zip(streams, case.chunks)):
        at = (name, i)
        assert s[:4] == b"BZh" + bytes([0x30 + case.level]), at
        d = bz2.BZ2Decompressor()
        assert d.decompress(s) == content and d.eof and not d.unused_data, at
        ec.check_stream(s, content, case.level, at=at)
    # the oracle and the GPU decoder return the array's native bytes
    native = case.chunks if (isb or case.src is None) else case.src
    ref = oracle("bzip2", streams, case.dt, D // es)
    assert ref[0] == ["Ok"] * n and ref[1] == list(native), name
    check_many("bzip2", streams, case.dt, D // es, param=case.level, guard=GUARD, ref=ref)
    return streams


@pytest.mark.parametrize("name", ec.SORT_NAMES)
def test_rotation_sort(name):
    """One block per chunk and a 3-byte prefix: prefix groups that the LDS
    pass insertion-sorts, bitonic-sorts, or leaves to the global rounds
    because they pass 2 048; ties within the 35 bytes the LDS pass compares
    and far past them; periodic texts, whose equal rotations leave the
    doubling only when h reaches the block's length."""
    run_case(name)


@pytest.mark.parametrize("name", ec.BATCH_NAMES)
def test_batches(name):
    """Blocks of 1 180 to 99 981 bytes, periodic and not, in one sort; more
    than 256 blocks in a sub-batch (a 2-byte prefix) at 600 KB instead of
    28 MiB; 5 000 chunks, which make_layout splits at 4 096."""
    run_case(name)


@pytest.mark.parametrize("name", ec.RLE1_NAMES)
def test_rle1_and_cuts(name):
    """A run across bmax at every offset and four phases of the 64-byte
    step, at levels 1 and 2; a cut inside a run of 12 000, found in the step
    or remembered from an earlier one; runs of every length around 4 and
    255 at the step's edges; runs at the end of the input; runs that exist
    only in the serialised bytes of a byte-swapped or bool array."""
    run_case(name)


def test_table_counts():
    """nMTF on both sides of 200, 600, 1 200 and 2 400: 2 to 6 tables."""
    from bz2_read import read_stream
    streams = run_case("ngroups_each")
    got = [read_stream(s)[1][0].ngroups for s in streams]
    assert got == [ec.ngroups_rule(x) for x in ec.NGROUPS_NMTF]


def test_deep_codes():
    """bze_make_lengths' halve-and-retry loop: some table has a code of 17
    bits, and a Huffman tree over the counts of the symbols that table coded
    is deeper than that."""
    stream, = run_case("deep_codes")
    tabs = ec.table_depths(stream)
    assert any(longest == 17 and free > 17 for _, longest, free in tabs), tabs


def test_output_too_small():
    """A dst_cap one byte short: status 5 and the needed length for that
    chunk, nothing written behind either chunk's cap, and the chunk beside
    it, whose cap is exact, comes out as before."""
    case = ec.case("run_phases")
    meta = meta_for("bzip2", "u1", case.D, case.level)
    st, ol, out, bound = encode(meta, case.chunks, case.D)
    assert st.tolist() == [0, 0]
    st2, ol2, out2, _ = encode(meta, case.chunks, case.D, caps=[int(ol[0]) - 1, int(ol[1])])
    assert st2.tolist() == [ZCG_ERR_OUTPUT_TOO_SMALL, 0]
    assert ol2.tolist() == ol.tolist()
    assert (out2[0, ol[0] - 1:] == 0xAB).all() and (out2[1, ol[1]:] == 0xAB).all()
    assert out2[1, :ol[1]].tobytes() == out[1, :ol[1]].tobytes()
