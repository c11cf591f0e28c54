"""Batched box writes on the GPU: zcg_write_regions (many boxes of one shape
scattered into one shared chunk table in one launch) against zcg_write_region
per box and the numpy oracle (oracle/region_ref.py), and the store-level calls
behind write_ndarrays against the oracle's write_ndarray box by box and against
the existing single-box write_ndarray, file for file."""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from golden_util import zarrita_chunks, zarrita_meta_json  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Lz4, Raw, SliceDataChunk, _native  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.compression import Bzip2, Xz  # noqa: E402
from zarr_amd.region import (BoundingBox, _strides, region_grid, regions_waves, scatter_region,  # noqa: E402
                             scatter_regions, write_ndarray, write_ndarrays)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 8  # sentinel bytes before, between and after the slots (keeps 8-byte elements aligned)
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


def boxes_tensor(offsets, ptrs, dev):
    """Device tensor of _native.Box records."""
    import torch
    B = len(offsets)
    arr = (_native.Box * max(B, 1))()
    for b in range(B):
        for d, o in enumerate(offsets[b]):
            arr[b].offset[d] = int(o)
        arr[b].out = int(ptrs[b])
    raw = np.frombuffer(bytes(arr), np.uint8).copy()
    return torch.from_numpy(raw).to(dev)


BOX_BYTES = ctypes.sizeof(_native.Box)


class Slots:
    """Decoded chunk slots on the device over a grid range, ~25 % of them
    NULL in the table, every slot between sentinel guard bytes.  `image` is
    the host copy of the initial buffer; reset() restores it."""

    def __init__(self, rng, meta, lo, n, es, absent_frac=0.25):
        import torch
        self.meta, self.lo, self.n, self.es = meta, lo, n, es
        self.D = int(np.prod(meta.chunk_shape)) * es
        self.coords = list(itertools.product(*[range(a, a + k) for a, k in zip(lo, n)]))
        pitch = self.D + GUARD
        self.image = np.full(max(len(self.coords), 1) * pitch + GUARD, SENTINEL, np.uint8)
        self.at = {}
        for i, c in enumerate(self.coords):
            if rng.random() < absent_frac:
                continue  # a NULL entry; its bytes stay sentinel
            self.at[c] = GUARD + i * pitch
            self.image[self.at[c]:self.at[c] + self.D] = rng.integers(0, 256, self.D, dtype=np.uint8)
        self.dev = torch.device("cuda", 0)
        self.buf = torch.from_numpy(self.image.copy()).to(self.dev)

    def reset(self):
        import torch
        self.buf.copy_(torch.from_numpy(self.image))

    def table(self, lo=None, n=None):
        """int64 pointers, C order over lo .. lo + n (default: the slots' own range)."""
        lo = self.lo if lo is None else lo
        n = self.n if n is None else n
        cc = itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])
        return np.array([self.buf.data_ptr() + self.at[c] if c in self.at else 0 for c in cc] or [0], np.int64)

    def chunks(self, image=None):
        """coord -> flat elements of the present chunks in `image` (default: the initial one)."""
        image = self.image if image is None else image
        return {c: image[o:o + self.D].view(UINT[self.es]).copy() for c, o in self.at.items()}


def draw_case(seed):
    """The case generator of test_gpu_boxes.test_regions_equal_single_region_and_oracle."""
    rng = np.random.default_rng(9000 + seed)
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    B = [1, 2, 17, 300][(seed + seed // 4) % 4]
    if seed == 10:  # the fixed 8-dimensional case, extents <= 3
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
        offsets[1] = list(offsets[0])  # a duplicate offset: the later box wins
    return rng, es, order, B, shape, cs, bshape, offsets


def scatter_in_waves(meta, bshape, es, table, lo, n, offsets, boxes, status, strides):
    """One scatter_regions launch per wave of regions_waves, in order."""
    nw, wave_of = regions_waves(meta, offsets, bshape)
    b0 = 0
    while b0 < len(offsets):
        b1 = b0 + 1
        while b1 < len(offsets) and wave_of[b1] == wave_of[b0]:
            b1 += 1
        scatter_regions(meta, bshape, es, table, lo, n, boxes[b0 * BOX_BYTES:b1 * BOX_BYTES], status[b0:b1], strides)
        b0 = b1
    return nw


@pytest.mark.parametrize("seed", range(12))
def test_regions_equal_single_region_and_oracle(seed):
    """12 seeds: 1-4 dims and one 8-dim case, element sizes 1/2/4/8, C and F
    order, chunk extents 1-9, ~25 % NULL slots, 1/2/17/300 boxes; fast box
    lengths {1, 7, 33, 70, 600}, so that the tile walk and the row walk both
    run for every element size; offsets unaligned and partly beyond the array,
    one duplicated; input views with unit and doubled strides.  Split with
    regions_waves and launched per wave, the whole slot buffer — sentinel guard
    bytes before, between and after the slots included — must equal byte for
    byte what B sequential zcg_write_region calls over each box's own sub-table
    leave, and every present chunk must equal region_ref.write_ndarray applied
    box by box (chunks the oracle would create for absent coordinates are
    ignored)."""
    import torch
    rng, es, order, B, shape, cs, bshape, offsets = draw_case(seed)
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lo, n = union_grid(meta, offsets, bshape)
    slots = Slots(rng, meta, lo, n, es)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    subs, sub_at = [], []
    for off in offsets:
        blo, bn = region_grid(meta, BoundingBox(off, bshape))
        sub_at.append(sum(len(s) for s in subs))
        subs.append(slots.table(blo, bn))
    subtab = torch.from_numpy(np.concatenate(subs)).to(dev)
    total = int(np.prod(bshape))
    dt = UINT[es]
    for mult in (1, 2):
        strides = [s * mult for s in _strides(bshape, order)]
        span = total * mult * es
        src_h = rng.integers(0, 256, max(B * span, 1), dtype=np.uint8)
        src = torch.from_numpy(src_h).to(dev)
        ptrs = [src.data_ptr() + b * span for b in range(B)]
        # B sequential single-box calls, each over the box's own sub-table
        slots.reset()
        for b, off in enumerate(offsets):
            scatter_region(meta, BoundingBox(off, bshape), es, subtab[sub_at[b]:], src[b * span:], strides)
        torch.cuda.synchronize()
        ref = slots.buf.cpu().numpy()
        # the batched call, wave by wave
        slots.reset()
        status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        boxes = boxes_tensor(offsets, ptrs, dev)
        nw = scatter_in_waves(meta, bshape, es, table, lo, n, offsets, boxes, status, strides)
        torch.cuda.synchronize()
        assert B < 2 or nw >= 2  # the duplicate
        assert status.cpu().tolist() == [_native.OK] * B
        got = slots.buf.cpu().numpy()
        assert np.array_equal(got, ref), (seed, mult)
        assert np.array_equal(src.cpu().numpy(), src_h)  # the input views are only read
        # the oracle, box by box, on the present chunks
        want = slots.chunks()
        present = set(want)
        for b, off in enumerate(offsets):
            view = np.ndarray(tuple(bshape), dtype=dt, buffer=src_h, offset=b * span,
                              strides=tuple(s * es for s in strides))
            only = {c: want[c] for c in region_ref.bounded_coord_iter(shape, cs, off, bshape) if c in present}
            region_ref.write_ndarray(shape, cs, order, off, view, only)
            want.update({c: v for c, v in only.items() if c in present})
        have = slots.chunks(got)
        for c in present:
            assert np.array_equal(have[c], want[c]), (seed, mult, c)


@pytest.mark.parametrize("fast", [20, 200])
def test_box_outside_the_table(fast):
    """A table that misses one box's grid range: that box gets InvalidInput,
    and the slot buffer is byte-identical to a run without it (tile walk and
    row walk)."""
    import torch
    rng = np.random.default_rng(fast)
    shape, cs, bshape = [40, 1000], [4, 16], [5, fast]
    meta = ArrayMetadata.new(shape, cs, "<u4")
    meta.chunk_memory_layout = "C"
    offsets = [[3, 10], [30, 700], [12, 40]]
    lo, n = union_grid(meta, [offsets[0], offsets[2]], bshape)  # box 1 lies outside
    slots = Slots(rng, meta, lo, n, 4, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    total = int(np.prod(bshape))
    src = torch.from_numpy(rng.integers(0, 256, 3 * total * 4, dtype=np.uint8)).to(dev)
    ptrs = [src.data_ptr() + b * total * 4 for b in range(3)]
    strides = _strides(bshape, "C")
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    scatter_regions(meta, bshape, 4, table, lo, n, boxes_tensor(offsets, ptrs, dev), status, strides)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK, _native.INVALID_INPUT, _native.OK]
    got = slots.buf.cpu().numpy()
    slots.reset()
    status2 = torch.full((2,), -1, dtype=torch.int32, device=dev)
    scatter_regions(meta, bshape, 4, table, lo, n, boxes_tensor([offsets[0], offsets[2]], [ptrs[0], ptrs[2]], dev),
                    status2, strides)
    torch.cuda.synchronize()
    assert status2.cpu().tolist() == [_native.OK, _native.OK]
    without = slots.buf.cpu().numpy()
    assert np.array_equal(got, without)
    assert not np.array_equal(got, slots.image)  # the two inside boxes did write


def test_trivial_calls_write_nothing():
    """n_boxes = 0 and a zero-extent box shape return Ok and leave slots and
    statuses untouched."""
    import torch
    meta = ArrayMetadata.new([20, 20], [4, 4], "<u2")
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(5)
    slots = Slots(rng, meta, [0, 0], [5, 5], 2, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    src = torch.zeros((4096,), dtype=torch.uint8, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    scatter_regions(meta, [3, 3], 2, table, [0, 0], [5, 5], None, status, [3, 1])
    boxes = boxes_tensor([[1, 1], [2, 2]], [src.data_ptr(), src.data_ptr() + 2048], dev)
    scatter_regions(meta, [3, 0], 2, table, [0, 0], [5, 5], boxes, status, [1, 1])
    torch.cuda.synchronize()
    assert np.array_equal(slots.buf.cpu().numpy(), slots.image) and status.cpu().tolist() == [-1, -1]


def test_capture_and_replay_with_new_boxes():
    """One captured zcg_write_regions call (one stream, no parallel branches),
    replayed twice with different offsets in d_boxes and different input
    bytes: the kernel reads both when it runs."""
    import torch
    rng = np.random.default_rng(6)
    shape, cs, bshape = [50, 60], [7, 9], [6, 11]
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    # five boxes per set, one per band of ten rows: disjoint, so one launch is well defined
    sets = [[[10 * i + int(rng.integers(0, 4)), int(rng.integers(0, 58))] for i in range(5)] for _ in range(3)]
    lo, n = union_grid(meta, [o for s in sets for o in s], bshape)
    slots = Slots(rng, meta, lo, n, 2)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    total = int(np.prod(bshape))
    src = torch.zeros((5 * total * 2,), dtype=torch.uint8, device=dev)
    status = torch.full((5,), -1, dtype=torch.int32, device=dev)
    ptrs = [src.data_ptr() + b * total * 2 for b in range(5)]
    boxes = boxes_tensor(sets[0], ptrs, dev)
    s = torch.cuda.Stream()
    strides = _strides(bshape, "C")
    with torch.cuda.stream(s):
        scatter_regions(meta, bshape, 2, table, lo, n, boxes, status, strides)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        scatter_regions(meta, bshape, 2, table, lo, n, boxes, status, strides)
    for offs in sets[1:]:
        data = rng.integers(0, 1 << 16, (5, *bshape)).astype(np.uint16)
        boxes.copy_(boxes_tensor(offs, ptrs, dev))
        src.copy_(torch.from_numpy(data.reshape(-1).view(np.uint8)))
        slots.reset()
        status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * 5
        got = slots.buf.cpu().numpy()
        want = slots.chunks()
        present = set(want)
        for b, off in enumerate(offs):
            region_ref.write_ndarray(shape, cs, "C", off, data[b], want)
        have = slots.chunks(got)
        for c in present:
            assert np.array_equal(have[c], want[c]), (off, c)
        mask = np.ones(len(got), bool)
        for o in slots.at.values():
            mask[o:o + slots.D] = False
        assert (got[mask] == SENTINEL).all()  # guards and NULL slots


CODECS = [Raw(), Gzip(1), Lz4(65536), Bzip2(1), Xz(0)]


def random_store(root, seed):
    """The setup of test_gpu_boxes.random_store: five codecs, dtypes with bool
    and big-endian ones, fill values, ~25 % of the chunks absent."""
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
    h = FilesystemHierarchy.open_or_create(str(root))
    h.create_array("a", meta)
    n_el = int(np.prod(cs))
    chunks, todo = {}, []
    grid = [(s + c - 1) // c for s, c in zip(shape, cs)]
    for c in itertools.product(*[range(g) for g in grid]):
        if rng.random() < 0.25:
            continue  # absent chunk
        chunks[c] = draw_values(rng, npdt, n_el)
        todo.append(SliceDataChunk(list(c), chunks[c]))
    h.write_chunks("a", meta, todo)
    return rng, h, meta, npdt, chunks


def draw_values(rng, npdt, n):
    if npdt == np.dtype("bool"):
        return rng.integers(0, 2, n).astype(bool)
    if npdt.kind == "f":
        return rng.standard_normal(n).astype(npdt)
    return rng.integers(0, 200, n).astype(npdt)


def snapshot(root):
    """relative path -> bytes of every file under `root`."""
    out = {}
    for d, _, files in os.walk(str(root)):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, str(root))] = fh.read()
    return out


def chunk_files(root):
    return {k: v for k, v in snapshot(root).items() if k.split(os.sep)[0] == "data"}


def copy_store(src, dst):
    shutil.copytree(str(src), str(dst))
    return FilesystemHierarchy.open(str(dst))


def check_store_equals(h, root, meta, npdt, want):
    """The chunk files under `root` are exactly the oracle dict's keys, and
    every one decodes to the oracle's chunk."""
    keys = sorted(want)
    files = chunk_files(root)
    assert set(files) == {os.path.relpath(h.chunk_path("a", meta, list(c)), str(root)) for c in keys}
    got = h.read_chunks("a", meta, [list(c) for c in keys], npdt) if keys else []
    for c, ch in zip(keys, got):
        assert ch is not None and np.array_equal(np.asarray(ch.get_data()), want[c]), c


@pytest.mark.parametrize("seed", range(10))
def test_write_ndarrays_vs_oracle_and_single_box_path(tmp_path, seed):
    """write_ndarrays with 1-40 overlapping boxes (partly outside the array):
    the chunk files are the key set of the oracle's dict after sequential
    region_ref.write_ndarray, every file decodes to the oracle's chunk, and the
    existing write_ndarray applied box by box to a copy of the initial store
    leaves byte-identical files.  A slot budget of two chunks (several groups
    that share chunks) and device-tensor input give the same files."""
    import torch
    rng, h0, meta, npdt, chunks = random_store(tmp_path / "s0", seed)
    shape, cs = meta.shape, meta.chunk_shape
    nd = len(shape)
    B = [1, 40, 7, 13, 2, 25, 40, 3, 9, 31][seed]
    bshape = [int(rng.integers(1, 25 if nd < 3 else 10)) for _ in range(nd)]
    offsets = []
    while len(offsets) < B:
        off = [int(rng.integers(0, s + 3)) for s in shape]
        if all(meta.in_bounds(c) for c in region_ref.bounded_coord_iter(shape, cs, off, bshape)):
            offsets.append(off)
    arrays = draw_values(rng, npdt, B * int(np.prod(bshape))).reshape(B, *bshape)
    fill = 7 if meta.fill_value is not None else 0
    order = meta.chunk_memory_layout
    want = {c: v.copy() for c, v in chunks.items()}
    for b, off in enumerate(offsets):
        region_ref.write_ndarray(shape, cs, order, off, arrays[b], want, fill)

    ha = copy_store(tmp_path / "s0", tmp_path / "a")
    write_ndarrays(ha, "a", meta, offsets, arrays)
    check_store_equals(ha, tmp_path / "a", meta, npdt, want)
    files = chunk_files(tmp_path / "a")

    hb = copy_store(tmp_path / "s0", tmp_path / "b")
    for b, off in enumerate(offsets):
        write_ndarray(hb, "a", meta, off, arrays[b])
    assert chunk_files(tmp_path / "b") == files

    hc = copy_store(tmp_path / "s0", tmp_path / "c")
    write_ndarrays(hc, "a", meta, offsets, arrays, slot_budget_bytes=2 * int(np.prod(cs)) * npdt.itemsize)
    assert chunk_files(tmp_path / "c") == files

    hd = copy_store(tmp_path / "s0", tmp_path / "d")
    dense = np.concatenate([arrays[b].flatten(order=order) for b in range(B)])
    t = torch.from_numpy(dense.view(np.uint8).copy()).to(torch.device("cuda", 0))
    write_ndarrays(hd, "a", meta, offsets, t, shape=bshape)
    assert chunk_files(tmp_path / "d") == files


@pytest.mark.parametrize("es,n_el", [(1, 3), (1, 6), (1, 20), (1, 24), (2, 3), (2, 10), (2, 12), (4, 5), (4, 6),
                                     (8, 3)])
def test_absent_chunks_start_as_fill_value(tmp_path, es, n_el):
    """A store without chunk files and a nonzero fill value, element sizes
    1/2/4/8, chunks of 3, 6, 20 and 24 bytes (slots packed that far apart, so
    mostly not 16-byte aligned): each box partly covers several chunks, and
    every written chunk equals the oracle's."""
    dt = np.dtype(TYPESTR[es])
    shape, cs, bshape = [4 * n_el + 1, 5], [n_el, 1], [n_el + 1, 2]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es], Raw())
    meta.chunk_memory_layout = "F" if es in (2, 8) else "C"
    meta.fill_value = 201
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    rng = np.random.default_rng(es * 100 + n_el)
    offsets = [[1, 1], [n_el + 2, 0], [2 * n_el, 3], [3 * n_el - 1, 1]]
    arrays = rng.integers(0, 200, (len(offsets), *bshape)).astype(dt)
    want = {}
    for b, off in enumerate(offsets):
        region_ref.write_ndarray(shape, cs, meta.chunk_memory_layout, off, arrays[b], want, 201)
    assert len(want) >= 8
    write_ndarrays(h, "a", meta, offsets, arrays)
    check_store_equals(h, tmp_path, meta, dt, want)


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


def truncate(path):
    with open(path, "rb") as f:
        raw = f.read()
    with open(path, "wb") as f:
        f.write(raw[:len(raw) // 2])  # a short stream


def test_fully_covered_chunk_is_not_read(tmp_path):
    """Box 0 covers chunk [1, 1] completely, box 1 only partly: the chunk's
    corrupt old file is never read (ndarray.rs:327-335), the call succeeds and
    the store equals the oracle's."""
    h, meta, chunks = gzip_store(tmp_path)
    truncate(h.chunk_path("a", meta, [1, 1]))
    offsets = [[4, 5], [5, 6]]
    arrays = np.arange(2 * 4 * 5, dtype=np.int32).reshape(2, 4, 5) + 5000
    want = {c: v.copy() for c, v in chunks.items()}
    for b, off in enumerate(offsets):
        region_ref.write_ndarray(meta.shape, meta.chunk_shape, "C", off, arrays[b], want)
    write_ndarrays(h, "a", meta, offsets, arrays)
    check_store_equals(h, tmp_path, meta, np.int32, want)


def test_corrupt_chunk_under_a_partial_first_box_raises_and_writes_nothing(tmp_path):
    """Chunk [1, 2] is first visited by box 1, which covers it partly: its
    corrupt file makes the call raise the chunk's own status and name it, and
    every file of the store stays byte-identical (one group: reads precede
    writes)."""
    h, meta, chunks = gzip_store(tmp_path)
    truncate(h.chunk_path("a", meta, [1, 2]))
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [1, 2], np.int32)
    assert single.value.kind in ("UnexpectedEof", "InvalidData")
    before = snapshot(tmp_path)
    arrays = np.arange(2 * 4 * 5, dtype=np.int32).reshape(2, 4, 5) + 5000
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays(h, "a", meta, [[4, 5], [5, 6]], arrays)
    assert ei.value.kind == single.value.kind and "chunk [1, 2]" in str(ei.value)
    assert snapshot(tmp_path) == before


def test_verify_flag_reaches_the_decode(tmp_path):
    """A partly covered chunk whose gzip CRC is wrong: InvalidData with
    FLAG_VERIFY_GZIP_TRAILER, a silent success without the flag (as the
    reference)."""
    h, meta, chunks = gzip_store(tmp_path)
    p = h.chunk_path("a", meta, [0, 1])
    with open(p, "rb") as f:
        raw = bytearray(f.read())
    raw[-8] ^= 1  # CRC32 word of the trailer
    with open(p, "wb") as f:
        f.write(bytes(raw))
    before = snapshot(tmp_path)
    offsets = [[1, 6]]
    arrays = np.arange(4 * 5, dtype=np.int32).reshape(1, 4, 5) + 7000
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays(h, "a", meta, offsets, arrays, flags=_native.FLAG_VERIFY_GZIP_TRAILER)
    assert ei.value.kind == "InvalidData" and "chunk [0, 1]" in str(ei.value)
    assert snapshot(tmp_path) == before
    write_ndarrays(h, "a", meta, offsets, arrays)
    want = {c: v.copy() for c, v in chunks.items()}
    region_ref.write_ndarray(meta.shape, meta.chunk_shape, "C", offsets[0], arrays[0], want)
    check_store_equals(h, tmp_path, meta, np.int32, want)


def test_box_visiting_a_chunk_out_of_bounds_is_invalid_input(tmp_path):
    """Shape 10, chunk 4, offset 13: bounded_coord_iter visits chunk 3, outside
    the grid extent u64_ceil_div(10, 4) = 3, where the reference panics.  No
    file is created, not even for the box that is in bounds."""
    meta = ArrayMetadata.new([10], [4], "<i2")
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    assert not meta.in_bounds([3]) and region_ref.bounded_coord_iter([10], [4], [13], [2]) == [(3,)]
    before = snapshot(tmp_path)
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays(h, "a", meta, [[0], [13]], np.ones((2, 2), np.int16))
    assert ei.value.kind == "InvalidInput"
    assert snapshot(tmp_path) == before and not chunk_files(tmp_path)
    # empty calls write nothing either
    write_ndarrays(h, "a", meta, np.zeros((0, 1), np.uint64), np.ones((0, 2), np.int16))
    write_ndarrays(h, "a", meta, [[0], [5]], np.ones((2, 0), np.int16))
    assert snapshot(tmp_path) == before


def test_plain_c_caller_writes_boxes(tmp_path):
    """tests/c_abi/boxes_write_c.c, built here with gcc and the flags of
    tests/c_abi/Makefile, writes four 2x3x3 boxes into a copy of the zarrita
    fixture (one overhanging the array, two overlapping) with one
    zcg_store_write_boxes call and reads them back with zcg_store_read_boxes."""
    c_abi = os.path.join(ROOT, "tests", "c_abi")
    libdir = os.path.join(ROOT, "zarr_amd")
    exe = str(tmp_path / "boxes_write_c")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    r = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(c_abi, "boxes_write_c.c"), "-L" + libdir, "-lzchunk_gpu", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + os.path.join(rocm, "lib")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    store = str(tmp_path / "zarrita")
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "zarrita"), store)
    outf = str(tmp_path / "boxes.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "boxes_write_c: ok (4 boxes)" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(outf, "<i2").reshape(4, 2, 3, 3)
    want = {g: v.copy() for g, _, v in zarrita_chunks()}
    offsets = [[0, 0, 0], [1, 2, 3], [2, 1, 2], [3, 4, 5]]
    for b, off in enumerate(offsets):
        box = (1000 * (b + 1) + np.arange(18)).astype(np.int16).reshape(2, 3, 3)
        region_ref.write_ndarray([4, 5, 6], [2, 3, 4], "C", off, box, want)
    for b, off in enumerate(offsets):
        back = region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", off, [2, 3, 3], want.get, np.int16, 0)
        assert np.array_equal(got[b], back), off
    # the store itself: the eight chunk files, each the oracle's chunk
    h = FilesystemHierarchy.open(store)
    meta = ArrayMetadata.from_json(zarrita_meta_json())
    keys = sorted(want)
    chunks = h.read_chunks("/seq/i2", meta, [list(c) for c in keys], np.int16)
    for c, ch in zip(keys, chunks):
        assert ch is not None and np.array_equal(np.asarray(ch.get_data()), want[c]), c
