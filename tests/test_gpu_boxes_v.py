"""Batched calls for boxes of differing shapes on the GPU: zcg_read_regions_v /
zcg_write_regions_v (a shape and a view per box, one shared chunk table)
against zcg_read_region / zcg_write_region per box and the numpy oracle
(oracle/region_ref.py)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes import SENTINEL, TYPESTR, UINT, Store  # noqa: E402
from test_gpu_write_boxes import Slots  # noqa: E402
from zarr_amd import ArrayMetadata, _native  # noqa: E402
from zarr_amd.region import (BoundingBox, _strides, assemble_region, assemble_regions_v, region_grid,  # noqa: E402
                             regions_v_grid, regions_v_scratch_bytes, regions_v_waves, scatter_region,
                             scatter_regions_v, vboxes_tensor)

pytestmark = pytest.mark.gpu

GAP = 64  # sentinel bytes between two boxes' buffers


def bound_of(shapes, nd):
    return [max(int(s[d]) for s in shapes) for d in range(nd)]


def fast_dim(nd, order):
    return 0 if order == "F" else nd - 1


def slow_dim(nd, order):
    """The slowest dimension of the chunk memory order."""
    return nd - 1 if order == "F" else 0


class Views:
    """One buffer region per box, GAP sentinel bytes apart: box b's view has
    the strides of mode (b + shift) % 3 — dense in the chunk memory order,
    doubled (a view into a larger buffer), or dense with a negative stride
    along the slowest dimension (base at the last plane)."""

    def __init__(self, shapes, es, order, shift=0, modes=(0, 1, 2)):
        self.es = es
        self.shapes = shapes
        self.strides, self.start, self.rel = [], [], []
        at = GAP
        for b, shp in enumerate(shapes):
            nd = len(shp)
            st = _strides(shp, order)
            mode = modes[(b + shift) % len(modes)]
            rel = 0
            if mode == 1:
                st = [2 * s for s in st]
            elif mode == 2:
                d = slow_dim(nd, order)
                rel = max(int(shp[d]) - 1, 0) * st[d]
                st[d] = -st[d]
            span = int(np.prod([max(int(s), 1) for s in shp])) * (2 if mode == 1 else 1) * es
            self.strides.append(st)
            self.start.append(at)
            self.rel.append(rel * es)
            at += span + GAP
        self.size = at

    def bases(self, buf):
        return [buf.data_ptr() + s + r for s, r in zip(self.start, self.rel)]

    def view(self, host, b, dt):
        """Box b as an array over the host copy `host` of the buffer."""
        return np.ndarray(tuple(self.shapes[b]), dtype=dt, buffer=host, offset=self.start[b] + self.rel[b],
                          strides=tuple(s * self.es for s in self.strides[b]))


def mixed_case(seed):
    """The shapes every case mixes into one call, with V = 16 / elem_size: a
    fast extent of 1; a row shorter than 16 bytes; fast extents 32V-1, 32V and
    32V+1 (the rows / tiles rule); a row longer than one row piece (4 096 bytes
    and 5 elements); for ndim > 1 a tile-mode box (fast extent 3V+1) of more
    than one tile whose size is no multiple of 4 096 bytes; a zero-extent box
    between two others; a box partly and a box wholly outside the array; a
    duplicate of an earlier box."""
    rng = np.random.default_rng(31000 + seed)
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    V = 16 // es
    if seed == 9:  # the 8-dimensional case
        nd, aslow, cslow = 8, [2, 3, 2, 2, 2, 2, 2], [1, 2, 2, 1, 2, 1, 2]
        cfast = 257
    else:
        nd = 1 + seed % 4
        aslow = {1: [], 2: [96], 3: [10, 11], 4: [5, 6, 5]}[nd]
        cslow = [int(rng.integers(1, 5)) for _ in aslow]
        cfast = [61, 100, 257][seed % 3]
    afast = 4096 // es + 40

    def dims(slow, fast):  # per array dim: the fast dimension is the first in F order, the last in C order
        return [fast] + list(slow) if order == "F" else list(slow) + [fast]

    shape, cs = dims(aslow, afast), dims(cslow, cfast)
    fd = fast_dim(nd, order)

    def box(fast, off_fast=None, slow=None):
        shp = dims([int(rng.integers(1, min(3, a) + 1)) for a in aslow] if slow is None else slow, fast)
        off = [int(rng.integers(0, max(1, s - b + 1))) for s, b in zip(shape, shp)]
        if off_fast is not None:
            off[fd] = off_fast
        return off, shp

    boxes = [box(1), box(max(1, V // 2)), box(32 * V - 1)]
    zoff, zshp = box(5)
    zshp[int(rng.integers(0, nd))] = 0
    boxes.append((zoff, zshp))
    boxes += [box(32 * V), box(32 * V + 1), box(4096 // es + 5, off_fast=int(rng.integers(0, 30)))]
    if nd > 1:
        boxes.append(box(3 * V + 1, slow=aslow))
        assert int(np.prod(boxes[-1][1])) * es > 4096 and (int(np.prod(boxes[-1][1])) * es) % 4096
    poff, pshp = box(V + 2)
    boxes.append(([s - 1 for s in shape], pshp))  # partly outside: one element per dimension is inside
    woff, wshp = box(2 * V)
    d = int(rng.integers(0, nd))
    woff[d] = (shape[d] // cs[d] + 2) * cs[d]  # wholly outside, at a chunk boundary: it visits no chunk
    boxes.append((woff, wshp))
    boxes.append((list(boxes[2][0]), list(boxes[2][1])))  # a duplicate, into its own output
    offsets, shapes = [b[0] for b in boxes], [b[1] for b in boxes]
    absent = 0.25 if seed % 2 == 0 else 0.0
    return rng, es, order, shape, cs, offsets, shapes, absent


@pytest.mark.parametrize("seed", range(10))
def test_regions_v_equal_single_region_and_oracle(seed):
    """10 seeds: 1-4 dimensions and one 8-dimensional case, element sizes
    1/2/4/8, C and F order, with (even seeds) and without absent chunks, fill
    on and off; the boxes of mixed_case in one call, their views dense, doubled
    or with a negative stride.  Every box must equal, byte for byte over the
    whole buffer (sentinel bytes around and between the outputs included), what
    zcg_read_region writes for that box alone from the box's own sub-table, and
    the oracle's read_ndarray / read_ndarray_into."""
    import torch
    rng, es, order, shape, cs, offsets, shapes, absent = mixed_case(seed)
    nd, B = len(shape), len(offsets)
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lo, n = regions_v_grid(meta, offsets, shapes)
    store = Store(rng, meta, lo, n, es, order, absent_frac=absent)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    subs, sub_at = [], []
    for off, shp in zip(offsets, shapes):
        blo, bn = region_grid(meta, BoundingBox(off, shp))
        sub_at.append(sum(len(s) for s in subs))
        subs.append(store.table(blo, bn))
    subtab = torch.from_numpy(np.concatenate(subs)).to(dev)
    fillv = 0x1122334455667788 & ((1 << (8 * es)) - 1)
    dt = UINT[es]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    views = Views(shapes, es, order, shift=seed)
    bound = bound_of(shapes, nd)
    for fill in (0, 1):
        out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
        ref = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
        status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        vb = vboxes_tensor(offsets, shapes, views.strides, views.bases(out))
        assemble_regions_v(meta, bound, es, table, lo, n, vb, status, bool(fill), fillv)
        rbases = views.bases(ref)
        for b in range(B):
            assemble_region(meta, BoundingBox(offsets[b], shapes[b]), es, subtab[sub_at[b]:],
                            ref[rbases[b] - ref.data_ptr():], views.strides[b], bool(fill), fillv)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        got = out.cpu().numpy()
        assert np.array_equal(got, ref.cpu().numpy()), (seed, fill)
        for b in range(B):
            if fill:
                w = region_ref.read_ndarray(shape, cs, order, offsets[b], shapes[b], store.chunks.get, dt, fillv)
            else:
                w = np.full(tuple(shapes[b]), sent, dtype=dt)
                region_ref.read_ndarray_into(shape, cs, order, offsets[b], shapes[b], store.chunks.get, w)
            assert np.array_equal(views.view(got, b, dt), w), (seed, fill, b)


@functools.lru_cache(maxsize=None)
def tiny_store():
    """A 40 x 50 u16 array in 7 x 9 chunks, ~25 % absent, shared by the tests
    with many tiny boxes."""
    rng = np.random.default_rng(77)
    shape, cs = [40, 50], [7, 9]
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    store = Store(rng, meta, [0, 0], [6, 6], 2, "C")
    return meta, store


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_box_counts_at_the_edges_of_the_scan_and_the_search(B):
    """B tiny boxes of differing shapes (extents 0-6 x 0-9, so some have a
    zero extent), dense, in one call: wave and workgroup edges of the plan
    kernel's prefix scan and of the walk's unit search.  Each box against the
    oracle; sentinels between the boxes untouched; a status word per box."""
    import torch
    meta, store = tiny_store()
    shape, cs = meta.shape, meta.chunk_shape
    rng = np.random.default_rng(B)
    shapes = [[int(rng.integers(0, 7)), int(rng.integers(0, 10))] for _ in range(B)]
    offsets = [[int(rng.integers(0, 36)), int(rng.integers(0, 44))] for _ in range(B)]
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    views = Views(shapes, 2, "C", modes=(0,))
    out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    vb = vboxes_tensor(offsets, shapes, views.strides, views.bases(out))
    assemble_regions_v(meta, [6, 9], 2, table, store.lo, store.n, vb, status, True, 0xBEEF)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * B
    got = out.cpu().numpy()
    want = np.full(views.size, SENTINEL, np.uint8)
    for b in range(B):
        w = region_ref.read_ndarray(shape, cs, "C", offsets[b], shapes[b], store.chunks.get, np.uint16, 0xBEEF)
        want[views.start[b]:views.start[b] + w.nbytes] = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fast", [20, 200])
def test_refused_boxes_in_the_middle_of_a_call(fast):
    """A box above the bound and a box whose grid range is outside the table,
    in the middle of a call (tile walk and row walk): both get InvalidInput and
    their outputs stay all sentinel; their neighbours are Ok and correct; the
    zero-extent box gets a status word too."""
    import torch
    rng = np.random.default_rng(fast)
    shape, cs = [40, 1000], [4, 16]
    meta = ArrayMetadata.new(shape, cs, "<u4")
    meta.chunk_memory_layout = "C"
    offsets = [[3, 10], [5, 30], [6, 40], [30, 700], [7, 50], [1, 90]]
    shapes = [[5, fast], [6, fast], [2, fast - 3], [3, fast], [4, 0], [5, fast - 1]]
    good = [0, 2, 5]
    bound = bound_of([shapes[b] for b in good], 2)
    assert shapes[1][0] == bound[0] + 1  # box 1 is above the bound, in a slow dimension
    lo, n = regions_v_grid(meta, [offsets[b] for b in good], [shapes[b] for b in good])  # box 3 lies outside
    store = Store(rng, meta, lo, n, 4, "C", absent_frac=0.0)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    views = Views(shapes, 4, "C", modes=(0,))
    out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((6,), -1, dtype=torch.int32, device=dev)
    vb = vboxes_tensor(offsets, shapes, views.strides, views.bases(out))
    assemble_regions_v(meta, bound, 4, table, lo, n, vb, status, True, 9)
    torch.cuda.synchronize()
    bad = _native.INVALID_INPUT
    assert status.cpu().tolist() == [_native.OK, bad, _native.OK, bad, _native.OK, _native.OK]
    got = out.cpu().numpy()
    want = np.full(views.size, SENTINEL, np.uint8)
    for b in good:
        w = region_ref.read_ndarray(shape, cs, "C", offsets[b], shapes[b], store.chunks.get, np.uint32, 9)
        want[views.start[b]:views.start[b] + w.nbytes] = w.view(np.uint8).reshape(-1)
    assert np.array_equal(got, want)


def band_boxes(rng, es, order, nd_slow_rows):
    """Pairwise disjoint boxes of the mixed fast extents in a 2-D array: box i
    lies in its own band of slow rows."""
    V = 16 // es
    fasts = [1, max(1, V // 2), 32 * V - 1, 32 * V, 32 * V + 1, 4096 // es + 5, 3 * V + 1, 5, V + 2]
    heights = [2, 3, 1, 2, 3, 2, nd_slow_rows, 0, 2]  # the 3V+1 box: more than one tile; one zero extent
    afast = 4096 // es + 40
    offsets, shapes, row, last = [], [], 0, 0
    for f, h in zip(fasts, heights):
        last = row
        offs = int(rng.integers(0, afast - f + 1))
        if order == "F":
            offsets.append([offs, row])
            shapes.append([f, h])
        else:
            offsets.append([row, offs])
            shapes.append([h, f])
        row += h + int(rng.integers(0, 2))
    aslow = last + 1  # the last band overhangs the array by a row
    return ([afast, aslow] if order == "F" else [aslow, afast]), offsets, shapes


@pytest.mark.parametrize("seed", range(4))
def test_write_regions_v_disjoint_boxes_equal_write_region(seed):
    """Element sizes 1/2/4/8, C and F order, ~25 % NULL slots: pairwise
    disjoint boxes of the mixed shapes, their input views dense, doubled or
    with a negative stride, scattered by one zcg_write_regions_v call; the
    whole slot buffer (guard bytes and NULL slots included) must equal what
    zcg_write_region leaves box by box."""
    import torch
    rng = np.random.default_rng(52000 + seed)
    es = [1, 2, 4, 8][seed]
    order = "F" if seed % 2 else "C"
    rows = 4096 // ((3 * (16 // es) + 1) * es) + 7
    shape, offsets, shapes = band_boxes(rng, es, order, rows)
    cs = [61, 3] if order == "F" else [3, 61]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    B = len(offsets)
    lo, n = regions_v_grid(meta, offsets, shapes)
    slots = Slots(rng, meta, lo, n, es)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    views = Views(shapes, es, order, shift=seed)
    src = torch.from_numpy(rng.integers(0, 256, views.size, dtype=np.uint8)).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    vb = vboxes_tensor(offsets, shapes, views.strides, views.bases(src))
    scatter_regions_v(meta, bound_of(shapes, 2), es, table, lo, n, vb, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * B
    got = slots.buf.cpu().numpy()
    slots.reset()
    bases = views.bases(src)
    for b in range(B):
        blo, bn = region_grid(meta, BoundingBox(offsets[b], shapes[b]))
        sub = torch.from_numpy(slots.table(blo, bn)).to(dev)
        scatter_region(meta, BoundingBox(offsets[b], shapes[b]), es, sub, src[bases[b] - src.data_ptr():],
                       views.strides[b])
    torch.cuda.synchronize()
    want = slots.buf.cpu().numpy()
    assert not np.array_equal(want, slots.image)  # something was written
    assert np.array_equal(got, want), seed


@pytest.mark.parametrize("seed", range(3))
def test_write_regions_v_overlapping_boxes_in_waves_equal_the_sequential_result(seed):
    """40 overlapping boxes of differing shapes (tile and row walk), launched
    wave by wave (zcg_regions_v_waves) on one stream with one shared scratch
    buffer, leave the slots as zcg_write_region box by box in order does: a
    later box wins."""
    import torch
    rng = np.random.default_rng(61000 + seed)
    es = [2, 4, 1][seed]
    V = 16 // es
    shape, cs = [30, 40 * V + 50], [4, 11 * V]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = "C"
    B = 40
    shapes = [[int(rng.integers(0 if b == 7 else 1, 9)), int(rng.choice([3, V + 1, 32 * V - 1, 32 * V + 3, 36 * V]))]
              for b in range(B)]
    offsets = [[int(rng.integers(0, 26)), int(rng.integers(0, 12 * V))] for _ in range(B)]
    lo, n = regions_v_grid(meta, offsets, shapes)
    slots = Slots(rng, meta, lo, n, es, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    views = Views(shapes, es, "C", shift=seed)
    src = torch.from_numpy(rng.integers(0, 256, views.size, dtype=np.uint8)).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    vb = vboxes_tensor(offsets, shapes, views.strides, views.bases(src))
    scratch = torch.empty(regions_v_scratch_bytes(B), dtype=torch.uint8, device=dev)
    nw, wave_of = regions_v_waves(meta, offsets, shapes)
    assert nw > 1 and wave_of[0] == 0 and wave_of[-1] == nw - 1
    rec = ctypes.sizeof(_native.VBox)
    b0 = 0
    while b0 < B:
        b1 = b0 + 1
        while b1 < B and wave_of[b1] == wave_of[b0]:
            b1 += 1
        scatter_regions_v(meta, bound_of(shapes, 2), es, table, lo, n, vb[b0 * rec:b1 * rec], status[b0:b1],
                          scratch=scratch)
        b0 = b1
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * B
    got = slots.buf.cpu().numpy()
    slots.reset()
    bases = views.bases(src)
    for b in range(B):
        blo, bn = region_grid(meta, BoundingBox(offsets[b], shapes[b]))
        sub = torch.from_numpy(slots.table(blo, bn)).to(dev)
        scatter_region(meta, BoundingBox(offsets[b], shapes[b]), es, sub, src[bases[b] - src.data_ptr():],
                       views.strides[b])
    torch.cuda.synchronize()
    assert np.array_equal(got, slots.buf.cpu().numpy()), seed


def test_capture_and_replay_with_new_offsets_shapes_and_bases():
    """One captured zcg_read_regions_v call (one graph, no parallel branches),
    replayed twice with new offsets, shapes, strides and bases in d_boxes, all
    inside the bound: the kernels read them when they run."""
    import torch
    rng = np.random.default_rng(6)
    shape, cs, bound = [50, 600], [7, 9], [6, 290]  # rows of 256 elements and more go a wave per row piece
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    B = 5

    def draw():
        shapes = [[int(rng.integers(0, bound[0] + 1)), int(rng.choice([1, 11, 255, 256, 290]))] for _ in range(B)]
        offsets = [[int(rng.integers(0, shape[0] - 2)), int(rng.integers(0, shape[1] - 2))] for _ in range(B)]
        return offsets, shapes

    sets = [draw() for _ in range(3)]
    store = Store(rng, meta, [0, 0], [8, 67], 2, "C")
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    size = max(Views(s[1], 2, "C", shift=i).size for i, s in enumerate(sets))
    out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(regions_v_scratch_bytes(B), dtype=torch.uint8, device=dev)
    v0 = Views(sets[0][1], 2, "C")
    vb = vboxes_tensor(sets[0][0], sets[0][1], v0.strides, v0.bases(out))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assemble_regions_v(meta, bound, 2, table, store.lo, store.n, vb, status, True, 3, scratch=scratch)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assemble_regions_v(meta, bound, 2, table, store.lo, store.n, vb, status, True, 3, scratch=scratch)
    for i, (offsets, shapes) in enumerate(sets[1:], 1):
        views = Views(shapes, 2, "C", shift=i)
        vb.copy_(vboxes_tensor(offsets, shapes, views.strides, views.bases(out)))
        out.fill_(SENTINEL)
        status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        got = out.cpu().numpy()
        for b in range(B):
            w = region_ref.read_ndarray(shape, cs, "C", offsets[b], shapes[b], store.chunks.get, np.uint16, 3)
            assert np.array_equal(views.view(got, b, np.uint16), w), (i, b)


def test_trivial_calls():
    """n_boxes = 0 returns Ok and writes nothing; a bound whose extent plus the
    chunk extent reaches 2^32 is Unsupported, and nothing is launched."""
    import torch
    meta, store = tiny_store()
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    assemble_regions_v(meta, [3, 3], 2, table, store.lo, store.n, None, status, True, 0)
    scatter_regions_v(meta, [3, 3], 2, table, store.lo, store.n, None, status)
    vb = vboxes_tensor([[1, 1], [2, 2]], [[2, 2], [1, 3]], [[3, 1], [3, 1]], [out.data_ptr(), out.data_ptr() + 2048])
    with pytest.raises(_native.NativeUnavailable):
        assemble_regions_v(meta, [3, (1 << 32) - 8], 2, table, store.lo, store.n, vb, status, True, 0)  # chunk 9
    with pytest.raises(_native.NativeUnavailable):
        scatter_regions_v(meta, [(1 << 32) - 6, 3], 2, table, store.lo, store.n, vb, status)  # chunk 7
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and status.cpu().tolist() == [-1, -1]
