"""Batched box reads on the GPU: zcg_read_regions (many boxes of one shape in
one launch, one shared chunk table) against zcg_read_region per box and the
numpy oracle (oracle/region_ref.py), and the store-level calls behind
read_ndarrays against the oracle's read_ndarray per box."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from golden_util import zarrita_chunks  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Lz4, Raw, SliceDataChunk, _native  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.compression import Bzip2, Xz  # noqa: E402
from zarr_amd.region import (BoundingBox, _strides, assemble_region, assemble_regions, read_ndarrays,  # noqa: E402
                             region_grid)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TYPESTR = {1: "u1", 2: "<u2", 4: "<u4", 8: "<u8"}


def union_grid(meta, offsets, shape):
    L = _native.load_library()
    nd = meta.get_ndim()
    r = _native.Region()
    r.ndim, r.elem_size = nd, 1
    for d in range(nd):
        r.array_shape[d], r.chunk_shape[d], r.bbox_shape[d] = meta.shape[d], meta.chunk_shape[d], shape[d]
    offs = np.ascontiguousarray(np.asarray(offsets, np.uint64).reshape(-1, nd))
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    n = (ctypes.c_uint64 * _native.MAX_DIMS)()
    L.zcg_regions_grid(ctypes.byref(r), offs.ctypes.data, len(offs), ctypes.addressof(lo), ctypes.addressof(n))
    return [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]


def boxes_tensor(offsets, out_ptrs, dev):
    """Device tensor of _native.Box records."""
    import torch
    B = len(offsets)
    arr = (_native.Box * max(B, 1))()
    for b in range(B):
        for d, o in enumerate(offsets[b]):
            arr[b].offset[d] = int(o)
        arr[b].out = int(out_ptrs[b])
    raw = np.frombuffer(bytes(arr), np.uint8).copy()
    return torch.from_numpy(raw).to(dev)


class Store:
    """Synthetic decoded chunks on the device over a grid range, ~25 % absent."""

    def __init__(self, rng, meta, lo, n, es, order, absent_frac=0.25):
        import torch
        self.meta, self.lo, self.n = meta, lo, n
        cs = meta.chunk_shape
        N = int(np.prod(cs))
        self.coords = list(itertools.product(*[range(a, a + k) for a, k in zip(lo, n)]))
        host = rng.integers(0, 256, (max(len(self.coords), 1), N * es), dtype=np.uint8)
        self.chunks = {}
        self.dev = torch.device("cuda", 0)
        self.slots = torch.from_numpy(host.reshape(-1)).to(self.dev)
        self.ptr = {}
        for i, c in enumerate(self.coords):
            if rng.random() < absent_frac:
                continue
            self.chunks[c] = host[i].view(UINT[es])
            self.ptr[c] = self.slots.data_ptr() + i * N * es

    def table(self, lo=None, n=None):
        """int64 pointers, C order over lo .. lo + n (default: the store's own range)."""
        lo = self.lo if lo is None else lo
        n = self.n if n is None else n
        cc = itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])
        return np.array([self.ptr.get(c, 0) for c in cc] or [0], np.int64)


def draw_case(seed):
    """Shapes for the equivalence test (see its docstring)."""
    rng = np.random.default_rng(9000 + seed)
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    B = [1, 2, 17, 300][(seed + seed // 4) % 4]
    if seed == 10:  # the fixed 8-dimensional case, extents <= 3
        nd = 8
        shape = [3, 2, 3, 1, 2, 3, 2, 3]
        cs = [2, 1, 3, 1, 2, 2, 1, 2]
        bshape = [2, 1, 2, 1, 2, 3, 1, 2]
    else:
        nd = int(rng.integers(1, 5))
        fast = {0: 600, 1: 33, 2: 7, 3: 1, 4: 33, 5: 600, 6: 600, 7: 600, 8: 7, 9: 1, 11: 70}[seed]
        slow_max = 9 if nd < 3 else 5
        while True:  # redraw until the test stays small: box elements, chunks in all, chunks per box
            bslow = [int(rng.integers(1, slow_max)) for _ in range(nd - 1)]
            cs = [int(rng.integers(1, 10)) for _ in range(nd)]
            aslow = [int(rng.integers(1, 2 * slow_max)) for _ in range(nd - 1)]
            afast = int(rng.integers(max(1, fast // 2), fast + 30))
            if order == "F":  # dim 0 is the fast one
                shape, bshape = [afast] + aslow, [fast] + bslow
            else:
                shape, bshape = aslow + [afast], bslow + [fast]
            n_all = int(np.prod([(s + 3 + b) // c + 1 for s, b, c in zip(shape, bshape, cs)]))
            n_box = int(np.prod([b // c + 2 for b, c in zip(bshape, cs)]))
            if int(np.prod(bshape)) <= (4096 if B == 300 else 40000) and n_all <= 20000 and n_box * B <= 60000:
                break
    offsets = [[int(rng.integers(0, s + 3)) for s in shape] for _ in range(B)]
    if B >= 2:
        offsets[1] = list(offsets[0])  # a duplicate offset, written to its own output
    return rng, es, order, B, shape, cs, bshape, offsets


@pytest.mark.parametrize("seed", range(12))
def test_regions_equal_single_region_and_oracle(seed):
    """12 seeds: 1-4 dims and one 8-dim case, element sizes 1/2/4/8, C and F
    order, chunk extents 1-9, ~25 % absent chunks, 1/2/17/300 boxes; the box's
    fast-dimension length comes from {1, 7, 33, 70, 600}, so that the tile
    walk and the row walk (rows of >= 32*16/es elements) both run for every
    element size; offsets are random, unaligned and partly beyond the array,
    one duplicated.  Outputs are sentinel-filled views with unit and doubled
    strides, with and without fill.  Every box must equal, byte for byte over
    the whole output buffer, what zcg_read_region writes from the box's own
    sub-table, and the oracle's read_ndarray / read_ndarray_into."""
    import torch
    rng, es, order, B, shape, cs, bshape, offsets = draw_case(seed)
    nd = len(shape)
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lo, n = union_grid(meta, offsets, bshape)
    store = Store(rng, meta, lo, n, es, order)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    # each box's own sub-table (zcg_region_grid range), back to back
    subs, sub_at = [], []
    for off in offsets:
        blo, bn = region_grid(meta, BoundingBox(off, bshape))
        sub_at.append(sum(len(s) for s in subs))
        subs.append(store.table(blo, bn))
    subtab = torch.from_numpy(np.concatenate(subs)).to(dev)
    total = int(np.prod(bshape))
    fillv = 0x1122334455667788 & ((1 << (8 * es)) - 1)
    dt = UINT[es]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    # the oracle's boxes, once per fill mode
    want = {}
    for fill in (0, 1):
        want[fill] = []
        for off in offsets:
            if fill:
                w = region_ref.read_ndarray(shape, cs, order, off, bshape, store.chunks.get, dt, fillv)
            else:
                w = np.full(tuple(bshape), sent, dtype=dt)
                region_ref.read_ndarray_into(shape, cs, order, off, bshape, store.chunks.get, w)
            want[fill].append(w)
    for mult, fill in itertools.product((1, 2), (0, 1)):
        strides = [s * mult for s in _strides(bshape, order)]
        span = total * mult * es
        out = torch.full((max(B * span, 1),), SENTINEL, dtype=torch.uint8, device=dev)
        ref = torch.full((max(B * span, 1),), SENTINEL, dtype=torch.uint8, device=dev)
        status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        boxes = boxes_tensor(offsets, [out.data_ptr() + b * span for b in range(B)], dev)
        assemble_regions(meta, bshape, es, table, lo, n, boxes, status, strides, bool(fill), fillv)
        for b, off in enumerate(offsets):
            assemble_region(meta, BoundingBox(off, bshape), es, subtab[sub_at[b]:], ref[b * span:], strides,
                            bool(fill), fillv)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        got = out.cpu().numpy()
        assert np.array_equal(got, ref.cpu().numpy()), (seed, mult, fill)
        for b in range(B):
            view = np.ndarray(tuple(bshape), dtype=dt, buffer=got, offset=b * span,
                              strides=tuple(s * es for s in strides))
            assert np.array_equal(view, want[fill][b]), (seed, mult, fill, b)


@pytest.mark.parametrize("fast", [20, 200])
def test_box_outside_the_table(fast):
    """A table that misses one box's grid range: that box gets InvalidInput and
    its output stays all sentinel; its neighbours are Ok and correct (tile walk
    and row walk)."""
    import torch
    rng = np.random.default_rng(fast)
    shape, cs, bshape = [40, 1000], [4, 16], [5, fast]
    meta = ArrayMetadata.new(shape, cs, "<u4")
    meta.chunk_memory_layout = "C"
    offsets = [[3, 10], [30, 700], [6, 40]]
    lo, n = union_grid(meta, [offsets[0], offsets[2]], bshape)  # box 1 lies outside
    store = Store(rng, meta, lo, n, 4, "C", absent_frac=0.0)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    total = int(np.prod(bshape))
    out = torch.full((3 * total * 4,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    boxes = boxes_tensor(offsets, [out.data_ptr() + b * total * 4 for b in range(3)], dev)
    assemble_regions(meta, bshape, 4, table, lo, n, boxes, status, _strides(bshape, "C"), True, 9)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK, _native.INVALID_INPUT, _native.OK]
    got = out.cpu().numpy()
    assert (got[total * 4:2 * total * 4] == SENTINEL).all()
    for b in (0, 2):
        w = region_ref.read_ndarray(shape, cs, "C", offsets[b], bshape, store.chunks.get, np.uint32, 9)
        assert np.array_equal(got[b * total * 4:(b + 1) * total * 4].view(np.uint32).reshape(bshape), w)


def test_trivial_calls_write_nothing():
    """n_boxes = 0 and a zero-extent box shape return Ok and leave outputs and
    statuses untouched."""
    import torch
    meta = ArrayMetadata.new([20, 20], [4, 4], "<u2")
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(5)
    store = Store(rng, meta, [0, 0], [5, 5], 2, "C", absent_frac=0.0)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    assemble_regions(meta, [3, 3], 2, table, [0, 0], [5, 5], None, status, [3, 1], True, 0)
    boxes = boxes_tensor([[1, 1], [2, 2]], [out.data_ptr(), out.data_ptr() + 2048], dev)
    assemble_regions(meta, [3, 0], 2, table, [0, 0], [5, 5], boxes, status, [1, 1], True, 0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and status.cpu().tolist() == [-1, -1]


def test_capture_and_replay_with_new_boxes():
    """One captured zcg_read_regions call, replayed twice with different box
    records in d_boxes: the kernel reads them when it runs."""
    import torch
    rng = np.random.default_rng(6)
    shape, cs, bshape = [50, 60], [7, 9], [6, 11]
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    sets = [[[int(rng.integers(0, s - 2)) for s in shape] for _ in range(5)] for _ in range(3)]
    lo, n = union_grid(meta, [o for s in sets for o in s], bshape)
    store = Store(rng, meta, lo, n, 2, "C")
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    total = int(np.prod(bshape))
    out = torch.full((5 * total * 2,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((5,), -1, dtype=torch.int32, device=dev)
    ptrs = [out.data_ptr() + b * total * 2 for b in range(5)]
    boxes = boxes_tensor(sets[0], ptrs, dev)
    s = torch.cuda.Stream()
    strides = _strides(bshape, "C")
    with torch.cuda.stream(s):
        assemble_regions(meta, bshape, 2, table, lo, n, boxes, status, strides, True, 3)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assemble_regions(meta, bshape, 2, table, lo, n, boxes, status, strides, True, 3)
    for offs in sets[1:]:
        boxes.copy_(boxes_tensor(offs, ptrs, dev))
        out.fill_(SENTINEL)
        status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * 5
        got = out.cpu().numpy().view(np.uint16).reshape(5, *bshape)
        for b, off in enumerate(offs):
            w = region_ref.read_ndarray(shape, cs, "C", off, bshape, store.chunks.get, np.uint16, 3)
            assert np.array_equal(got[b], w), (off, b)


CODECS = [Raw(), Gzip(1), Lz4(65536), Bzip2(1), Xz(0)]


def random_store(tmp_path, seed):
    """The setup of test_gpu_region.test_region_random_vs_oracle: five codecs,
    dtypes with bool and big-endian ones, fill values, absent chunks."""
    rng = np.random.default_rng(500 + seed)
    nd = int(rng.integers(1, 5))
    dt = ["<i2", "<u1", "<f8", "<i4", "bool", ">u2", ">f4"][seed % 7]
    npdt = np.dtype("bool") if dt == "bool" else np.dtype(dt).newbyteorder("=")
    shape = [int(rng.integers(1, 30 if nd < 3 else 12)) for _ in range(nd)]
    cs = [int(rng.integers(1, 9)) for _ in range(nd)]
    meta = ArrayMetadata.new(shape, cs, dt, CODECS[seed % len(CODECS)])
    meta.chunk_memory_layout = "F" if seed % 2 else "C"
    if seed % 3 == 0 and dt != "bool":
        meta.fill_value = 7
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    n_el = int(np.prod(cs))
    chunks, todo = {}, []
    grid = [(s + c - 1) // c for s, c in zip(shape, cs)]
    for c in itertools.product(*[range(g) for g in grid]):
        if rng.random() < 0.25:
            continue  # absent chunk -> fill
        if dt == "bool":
            d = rng.integers(0, 2, n_el).astype(bool)
        elif npdt.kind == "f":
            d = rng.standard_normal(n_el).astype(npdt)
        else:
            d = rng.integers(0, 200, n_el).astype(npdt)
        chunks[c] = d
        todo.append(SliceDataChunk(list(c), d))
    h.write_chunks("a", meta, todo)
    return rng, h, meta, npdt, chunks


@pytest.mark.parametrize("seed", range(10))
def test_read_ndarrays_vs_oracle(tmp_path, seed):
    """read_ndarrays with 1-40 boxes (partly outside the array, overlapping)
    equals the oracle's read_ndarray per box, as numpy and as a device tensor;
    a slot budget of two chunks, which forces several groups, changes nothing."""
    rng, h, meta, npdt, chunks = random_store(tmp_path, seed)
    shape, cs = meta.shape, meta.chunk_shape
    nd = len(shape)
    B = [1, 40, 7, 13, 2, 25, 40, 3, 9, 31][seed]
    bshape = [int(rng.integers(1, 25 if nd < 3 else 10)) for _ in range(nd)]
    offsets = []
    while len(offsets) < B:
        off = [int(rng.integers(0, s + 3)) for s in shape]
        if all(meta.in_bounds(c) for c in region_ref.bounded_coord_iter(shape, cs, off, bshape)):
            offsets.append(off)
    fill = 7 if meta.fill_value is not None else 0
    order = meta.chunk_memory_layout
    want = np.stack([region_ref.read_ndarray(shape, cs, order, off, bshape, chunks.get, npdt, fill)
                     for off in offsets])
    es = npdt.itemsize
    budget = 2 * int(np.prod(cs)) * es
    for b in (0, budget):
        got = read_ndarrays(h, "a", meta, offsets, bshape, npdt, slot_budget_bytes=b)
        assert got.shape == (B, *bshape) and got.dtype == npdt
        assert np.array_equal(got, want), (seed, b)
        t, strides = read_ndarrays(h, "a", meta, offsets, bshape, npdt, as_tensor=True, slot_budget_bytes=b)
        assert strides == _strides(bshape, order)
        raw = t.cpu().numpy()
        total = int(np.prod(bshape))
        for i in range(B):
            view = np.ndarray(tuple(bshape), dtype=npdt, buffer=raw, offset=i * total * es,
                              strides=tuple(s * es for s in strides))
            assert np.array_equal(view, want[i]), (seed, b, i)


def gzip_store(tmp_path):
    meta = ArrayMetadata.new([10, 12], [4, 5], "<i4", Gzip(6))
    meta.chunk_memory_layout = "C"
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    rng = np.random.default_rng(3)
    chunks = {}
    for c in itertools.product(range(3), range(3)):
        chunks[c] = rng.integers(0, 1000, 20).astype(np.int32)
    h.write_chunks("a", meta, [SliceDataChunk(list(c), d) for c, d in chunks.items()])
    return h, meta, chunks


def test_corrupt_chunk_raises_its_status_and_names_the_chunk(tmp_path):
    h, meta, chunks = gzip_store(tmp_path)
    p = h.chunk_path("a", meta, [1, 2])
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:len(raw) // 2])  # a short stream
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [1, 2], np.int32)
    assert single.value.kind in ("UnexpectedEof", "InvalidData")
    offsets = [[0, 0], [3, 7], [5, 5]]
    with pytest.raises(ZarrIOError) as ei:
        read_ndarrays(h, "a", meta, offsets, [3, 4], np.int32)
    assert ei.value.kind == single.value.kind and "chunk [1, 2]" in str(ei.value)
    # boxes that do not visit the chunk still read
    got = read_ndarrays(h, "a", meta, offsets[:1], [3, 4], np.int32)
    want = region_ref.read_ndarray(meta.shape, meta.chunk_shape, "C", [0, 0], [3, 4], chunks.get, np.int32, 0)
    assert np.array_equal(got[0], want)


def test_verify_flag_reaches_the_decode(tmp_path):
    """A chunk whose gzip CRC is wrong reads silently without the flag (as the
    reference does) and raises InvalidData with FLAG_VERIFY_GZIP_TRAILER."""
    h, meta, chunks = gzip_store(tmp_path)
    p = h.chunk_path("a", meta, [0, 1])
    raw = bytearray(open(p, "rb").read())
    raw[-8] ^= 1  # CRC32 word of the trailer
    open(p, "wb").write(bytes(raw))
    offsets = [[0, 0], [2, 6]]
    got = read_ndarrays(h, "a", meta, offsets, [3, 4], np.int32)
    for b, off in enumerate(offsets):
        want = region_ref.read_ndarray(meta.shape, meta.chunk_shape, "C", off, [3, 4], chunks.get, np.int32, 0)
        assert np.array_equal(got[b], want)
    with pytest.raises(ZarrIOError) as ei:
        read_ndarrays(h, "a", meta, offsets, [3, 4], np.int32, flags=_native.FLAG_VERIFY_GZIP_TRAILER)
    assert ei.value.kind == "InvalidData" and "chunk [0, 1]" in str(ei.value)


def test_box_visiting_a_chunk_out_of_bounds_is_invalid_input(tmp_path):
    """Shape 10, chunk 4, offset 13: bounded_coord_iter visits chunk 3, outside
    the grid extent u64_ceil_div(10, 4) = 3, where the reference panics."""
    meta = ArrayMetadata.new([10], [4], "<i2")
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    h.write_chunks("a", meta, [SliceDataChunk([0], np.arange(4, dtype=np.int16))])
    assert not meta.in_bounds([3]) and region_ref.bounded_coord_iter([10], [4], [13], [2]) == [(3,)]
    with pytest.raises(ZarrIOError) as ei:
        read_ndarrays(h, "a", meta, [[0], [13]], [2], np.int16)
    assert ei.value.kind == "InvalidInput"
    assert read_ndarrays(h, "a", meta, [[0], [12]], [2], np.int16).tolist() == [[0, 1], [0, 0]]


def test_argument_errors(tmp_path):
    """ndim != chunk_ndim -> InvalidData, a raw (rN) type -> InvalidInput, a
    union chunk table above 2^24 entries -> Unsupported with a message; all
    before any file is read (the store holds no chunk)."""
    meta = ArrayMetadata.new([8192, 8192], [1, 1], "<u2")
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    ctx = _native.context(0)
    out = np.full(2, 0xA5A5, np.uint16)

    def call(am, offsets):
        offs = np.asarray(offsets, np.uint64).reshape(-1, 2)
        bshape = (ctypes.c_uint64 * 8)(1, 1)
        outs = (ctypes.c_void_p * len(offs))(*[out.ctypes.data + 2 * b for b in range(len(offs))])
        return ctx.lib.zcg_store_read_boxes(ctx.handle, ctypes.byref(am), os.fsencode(h.base_path), b"a",
                                            ctypes.addressof(bshape), offs.ctypes.data, ctypes.addressof(outs),
                                            len(offs), 0, 2)

    def fresh():
        st, am, msg = _native.array_meta_from_json(meta.to_json())
        assert st == _native.OK, msg
        return am

    am = fresh()
    am.chunk_ndim = 3
    assert call(am, [[0, 0]]) == _native.INVALID_DATA
    am = fresh()
    am.dtype_kind = 4  # ZCG_DT_RAW
    assert call(am, [[0, 0]]) == _native.INVALID_INPUT
    assert call(fresh(), [[0, 0], [8000, 8000]]) == _native.UNSUPPORTED
    assert "2^24" in ctx.last_error()
    assert (out == 0xA5A5).all()
    assert call(fresh(), [[0, 0], [8000, 7]]) == _native.OK and (out == 0).all()  # absent chunks: fill


def test_plain_c_caller_reads_boxes(tmp_path):
    """tests/c_abi/boxes_c.c, built here with gcc and the flags of
    tests/c_abi/Makefile, reads four 2x3x3 boxes of the zarrita fixture (one
    overhanging the array) with one zcg_store_read_boxes call."""
    c_abi = os.path.join(ROOT, "tests", "c_abi")
    libdir = os.path.join(ROOT, "zarr_amd")
    exe = str(tmp_path / "boxes_c")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    r = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(c_abi, "boxes_c.c"), "-L" + libdir, "-lzchunk_gpu", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + os.path.join(rocm, "lib")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    store = os.path.join(ROOT, "tests", "golden", "zarrita")
    outf = str(tmp_path / "boxes.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "boxes_c: ok (4 boxes)" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(outf, "<i2").reshape(4, 2, 3, 3)
    chunks = {g: v for g, _, v in zarrita_chunks()}
    for b, off in enumerate([[0, 0, 0], [1, 2, 3], [2, 1, 2], [3, 4, 5]]):
        want = region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", off, [2, 3, 3], chunks.get, np.int16, 0)
        assert np.array_equal(got[b], want), off
