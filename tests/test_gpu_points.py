"""Lists of coordinates on the GPU: zcg_read_points / zcg_write_points (one
element per point, one lane per point) against the numpy oracle
(oracle/region_ref.py) and against zcg_read_regions_v with boxes of shape
(1, ..., 1), bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes import SENTINEL, TYPESTR, UINT, Store  # noqa: E402
from test_gpu_boxes_v import tiny_store  # noqa: E402
from test_gpu_write_boxes import Slots  # noqa: E402
from zarr_amd import ArrayMetadata, _native  # noqa: E402
from zarr_amd.region import (assemble_points, assemble_regions_v, points_grid, points_last,  # noqa: E402
                             scatter_points, vboxes_tensor)

pytestmark = pytest.mark.gpu

GAP = 64  # sentinel bytes before and after the values
U64_MAX = (1 << 64) - 1
PER_WORKGROUP = 4 * 256  # the kernel's points per lane x its workgroup size

# ndim, chunk shape, array shape: chunk extents 1, 5, 7, 61 and 64; every array has at least three chunks along
# dimension 0 and an edge chunk that overhangs along some dimension
CASES = [
    (1, [61], [200]),
    (1, [64], [321]),
    (2, [7, 64], [30, 150]),
    (2, [61, 5], [190, 23]),
    (3, [5, 7, 61], [17, 20, 130]),
    (3, [1, 64, 5], [4, 130, 12]),
    (8, [1, 5, 2, 1, 7, 2, 1, 2], [3, 7, 3, 2, 9, 3, 2, 3]),
    (8, [2, 1, 3, 1, 2, 2, 1, 2], [5, 2, 4, 2, 3, 3, 2, 3]),
]


def fate(meta, lo, n, c):
    """include/zchunk_gpu.h's rule: None when the point visits no chunk, else
    (chunk, element index per dimension, chunk inside the table lo .. lo+n)."""
    q, rem = [], []
    for d, x in enumerate(c):
        cs, a = meta.chunk_shape[d], meta.shape[d]
        if not (x < a or x % cs):
            return None
        q.append(x // cs)
        rem.append(x % cs)
    return tuple(q), tuple(rem), all(l <= g < l + k for g, l, k in zip(q, lo, n))


def oracle_values(meta, order, pts, get, dt, fill, fillv, sent):
    """read_ndarray (fill) or a sentinel-filled read_ndarray_into of the bounding
    hull of the points that lie within two chunks of the array, indexed at the
    points; a point further out has a 1-element read of its own."""
    nd = meta.get_ndim()
    shape, cs = meta.shape, meta.chunk_shape
    near = [i for i, c in enumerate(pts) if all(x < s + 2 * k for x, s, k in zip(c, shape, cs))]
    out = np.full(len(pts), sent, dtype=dt)

    def read(off, shp):
        if fill:
            return region_ref.read_ndarray(shape, cs, order, off, shp, get, dt, fillv)
        w = np.full(tuple(shp), sent, dtype=dt)
        region_ref.read_ndarray_into(shape, cs, order, off, shp, get, w)
        return w

    if near:
        off = [min(pts[i][d] for i in near) for d in range(nd)]
        hull = read(off, [max(pts[i][d] for i in near) - off[d] + 1 for d in range(nd)])
        for i in near:
            out[i] = hull[tuple(x - o for x, o in zip(pts[i], off))]
    for i in set(range(len(pts))) - set(near):
        out[i] = read(list(pts[i]), [1] * nd).reshape(-1)[0]
    return out


def draw_points(rng, meta, P, far):
    """P points: interior ones from the second chunk along dimension 0 on; at
    index 17 a point in the first chunk along dimension 0 and at index 40 the
    array's index 0 (the two a pruned table leaves outside); the array's last
    index; an overhang point; a point beyond the grid at a chunk boundary; a
    duplicate; with `far`, at the end, 2^63, 2^64-1 and a point beyond the grid
    inside a chunk's nominal extent (which a 1-element box visits)."""
    shape, cs = meta.shape, meta.chunk_shape
    nd = len(shape)

    def interior():
        return [int(rng.integers(cs[0], shape[0]))] + [int(rng.integers(0, s)) for s in shape[1:]]

    pts = [interior() for _ in range(P)]
    pts[17] = [cs[0] - 1] + interior()[1:]
    pts[40] = [0] * nd
    pts[3] = [s - 1 for s in shape]
    d = next(d for d in range(nd) if shape[d] % cs[d])
    pts[5] = interior()
    pts[5][d] = shape[d]  # the overhang of the edge chunk
    assert pts[5][0] >= cs[0] or d == 0
    pts[8] = interior()
    pts[8][nd - 1] = (-(-shape[nd - 1] // cs[nd - 1]) + 1) * cs[nd - 1]  # beyond the grid: no chunk
    pts[P - 1] = list(pts[11])  # a duplicate
    if far:
        beyond = interior()
        edge = -(-shape[d] // cs[d]) * cs[d]
        beyond[d] = edge + cs[d] + 1
        pts += [[1 << 63] * nd, [U64_MAX] * nd, beyond, [1 << 63] + interior()[1:]]
    return pts


def coords_tensor(pts, dev):
    import torch
    return torch.from_numpy(np.array(pts, dtype=np.uint64).reshape(len(pts), -1).view(np.int64)).to(dev)


def word(dev):
    import torch
    return torch.zeros(1, dtype=torch.int64, device=dev)


def word_value(t):
    return int(t.cpu().numpy().view(np.uint64)[0])


def pruned_table(store, meta, lo, n, pts):
    """The store's pointers over lo .. lo+n, NULL where no point of `pts` falls."""
    import itertools
    touched = {f[0] for f in (fate(meta, lo, n, c) for c in pts) if f is not None and f[2]}
    cc = itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])
    return np.array([store.ptr.get(c, 0) if c in touched else 0 for c in cc] or [0], np.int64)


def setup_case(seed, far):
    rng = np.random.default_rng(52000 + seed)
    nd, cs, shape = CASES[seed]
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    pts = draw_points(rng, meta, 150, far)
    inside = [c for i, c in enumerate(pts[:150]) if not (far and i in (17, 40))]
    lo, n = points_grid(meta, inside)
    if far:
        assert lo[0] > 0  # the table starts above 0
    return rng, meta, es, order, pts, lo, n


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("seed", range(len(CASES)))
def test_points_equal_oracle_and_one_element_boxes(seed, far):
    """8 cases (1, 2, 3 and 8 dimensions, element sizes 1/2/4/8, C and F order),
    fill off and on, the point kinds of draw_points in one call; the table is
    pruned to the touched chunks, one of which is made absent.  Without `far`
    the table holds every visited chunk and the word stays UINT64_MAX; with it
    the table starts above 0 along dimension 0, points 17 and 40 (and the far
    points that visit a chunk) lie outside it, the word is 17 and their
    elements are untouched.  The whole buffer, sentinel bytes around the values
    included, must equal the oracle's values and what zcg_read_regions_v writes
    for the same points as boxes of shape 1."""
    import torch
    rng, meta, es, order, pts, lo, n = setup_case(seed, far)
    nd, P = meta.get_ndim(), len(pts)
    store = Store(rng, meta, lo, n, es, order, absent_frac=0.0)
    gone = fate(meta, lo, n, pts[11])[0]  # the duplicated point's chunk is absent
    del store.chunks[gone], store.ptr[gone]
    dev = store.dev
    table = torch.from_numpy(pruned_table(store, meta, lo, n, pts)).to(dev)
    coords = coords_tensor(pts, dev)
    dt = UINT[es]
    fillv = 0x1122334455667788 & ((1 << (8 * es)) - 1)
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    fates = [fate(meta, lo, n, c) for c in pts]
    outside = [i for i, f in enumerate(fates) if f is not None and not f[2]]
    assert (outside[:2] == [17, 40] and len(outside) >= 3) if far else not outside
    assert any(f is None for f in fates) and any(f and f[2] and f[0] not in store.chunks for f in fates)
    for fill in (0, 1):
        want = oracle_values(meta, order, pts, store.chunks.get, dt, fill, fillv, sent)
        want[outside] = sent
        out = torch.full((2 * GAP + P * es,), SENTINEL, dtype=torch.uint8, device=dev)
        ref = torch.full((2 * GAP + P * es,), SENTINEL, dtype=torch.uint8, device=dev)
        first = word(dev)
        assemble_points(meta, es, table, lo, n, coords, out[GAP:], first, bool(fill), fillv)
        status = torch.full((P,), -1, dtype=torch.int32, device=dev)
        vb = vboxes_tensor(pts, [[1] * nd] * P, [[1] * nd] * P, [ref.data_ptr() + GAP + i * es for i in range(P)])
        assemble_regions_v(meta, [1] * nd, es, table, lo, n, vb, status, bool(fill), fillv)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:GAP] == SENTINEL).all() and (got[GAP + P * es:] == SENTINEL).all()
        assert np.array_equal(got[GAP:GAP + P * es].view(dt), want), (seed, fill)
        assert np.array_equal(got, ref.cpu().numpy()), (seed, fill)
        bad = [i for i, s in enumerate(status.cpu().tolist()) if s != _native.OK]
        assert bad == outside
        assert word_value(first) == (outside[0] if outside else U64_MAX)


@pytest.mark.parametrize("P", [1, 63, 64, 65, PER_WORKGROUP - 1, PER_WORKGROUP, PER_WORKGROUP + 1,
                               2 * PER_WORKGROUP + 1])
def test_point_counts_at_the_edges_of_a_wave_and_a_workgroup(P):
    """P random points over a 40 x 50 array, its edge chunks' overhang and the first
    index beyond the grid, fill on: every element against the oracle,
    the bytes after the last point untouched."""
    import torch
    meta, store = tiny_store()
    rng = np.random.default_rng(P)
    pts = [[int(rng.integers(0, 43)), int(rng.integers(0, 55))] for _ in range(P)]
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((P * 2 + GAP,), SENTINEL, dtype=torch.uint8, device=dev)
    first = word(dev)
    assemble_points(meta, 2, table, store.lo, store.n, coords_tensor(pts, dev), out, first, True, 0xBEEF)
    torch.cuda.synchronize()
    want = oracle_values(meta, "C", pts, store.chunks.get, np.uint16, 1, 0xBEEF, 0xA5A5)
    got = out.cpu().numpy()
    assert np.array_equal(got[:P * 2].view(np.uint16), want)
    assert (got[P * 2:] == SENTINEL).all() and word_value(first) == U64_MAX


def test_zero_points_launch_nothing_and_bad_arguments_are_refused():
    import torch
    meta, store = tiny_store()
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((16,), SENTINEL, dtype=torch.uint8, device=dev)
    first = torch.full((1,), 5, dtype=torch.int64, device=dev)
    ctx = _native.context(0)
    r = _native.Region()
    r.ndim, r.elem_size = 2, 2
    for d in range(2):
        r.array_shape[d], r.chunk_shape[d] = meta.shape[d], meta.chunk_shape[d]
    lo, n = (ctypes.c_uint64 * 8)(0, 0), (ctypes.c_uint64 * 8)(6, 6)
    c = coords_tensor([[1, 1]], dev)

    def call(n_points, fn=ctx.lib.zcg_read_points):
        return fn(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n), table.data_ptr(),
                  c.data_ptr(), n_points, out.data_ptr(), first.data_ptr(), None)

    assert call(0) == _native.OK and call(0, ctx.lib.zcg_write_points) == _native.OK
    torch.cuda.synchronize()
    assert word_value(first) == 5 and (out.cpu().numpy() == SENTINEL).all()  # not even the reset
    # the codes zcg_read_regions gives for the same descriptor
    for field, value in (("ndim", 0), ("ndim", 9), ("elem_size", 3)):
        keep = getattr(r, field)
        setattr(r, field, value)
        assert call(1) == _native.INVALID_INPUT and call(0) == _native.INVALID_INPUT
        setattr(r, field, keep)
    r.chunk_shape[1] = 0
    assert call(1) == _native.INVALID_INPUT
    r.chunk_shape[1] = meta.chunk_shape[1]
    r.bbox_shape[0] = 1 << 40  # ignored
    assert call(1) == _native.OK
    torch.cuda.synchronize()
    assert word_value(first) == U64_MAX


def slots_model(slots, meta, order, lo, n, pts, vals, image=None):
    """The slots' bytes after the scatter of `pts` in order, from `image`."""
    image = (slots.image if image is None else image).copy()
    es = slots.es
    raw = np.ascontiguousarray(vals).view(np.uint8).reshape(len(pts), es)
    for i, c in enumerate(pts):
        f = fate(meta, lo, n, c)
        if f is None or not f[2] or f[0] not in slots.at:
            continue
        at = int(np.ravel_multi_index(f[1], meta.chunk_shape, order=order))
        o = slots.at[f[0]] + at * es
        image[o:o + es] = raw[i]
    return image


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("seed", range(len(CASES)))
def test_scatter_equals_the_numpy_model_byte_for_byte(seed, far):
    """The cases and point kinds of the gather test without the duplicate, ~25 %
    of the slots NULL: every byte of the slot buffer (guard bytes and NULL
    slots' bytes included) against the model; the word as on the read side."""
    import torch
    rng, meta, es, order, pts, lo, n = setup_case(seed, far)
    pts[149] = [meta.shape[0] - 1] + pts[149][1:]
    keep = points_last(np.array(pts, np.uint64))
    pts = [c for c, k in zip(pts, keep) if k]  # no duplicates in this call
    P = len(pts)
    slots = Slots(rng, meta, lo, n, es)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    vals = rng.integers(0, 256, P * es, dtype=np.uint8).view(UINT[es])
    src = torch.from_numpy(vals.view(np.uint8).copy()).to(dev)
    first = word(dev)
    scatter_points(meta, es, table, lo, n, coords_tensor(pts, dev), src, first)
    torch.cuda.synchronize()
    assert np.array_equal(slots.buf.cpu().numpy(), slots_model(slots, meta, order, lo, n, pts, vals))
    outside = [i for i, f in enumerate(fate(meta, lo, n, c) for c in pts) if f is not None and not f[2]]
    assert bool(outside) == far and word_value(first) == (outside[0] if outside else U64_MAX)
    assert np.array_equal(src.cpu().numpy(), vals.view(np.uint8))  # the values are only read


def test_scatter_with_duplicates_leaves_one_value_and_points_last_the_last():
    import torch
    meta, _ = tiny_store()
    rng = np.random.default_rng(3)
    slots = Slots(rng, meta, [0, 0], [6, 6], 2, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    P = 3000
    pts = [[int(rng.integers(0, 12)), int(rng.integers(0, 12))] for _ in range(P)]  # 144 places, ~20 points each
    vals = (np.arange(P) + 1000).astype(np.uint16)
    src = torch.from_numpy(vals.view(np.uint8)).to(dev)
    first = word(dev)
    scatter_points(meta, 2, table, [0, 0], [6, 6], coords_tensor(pts, dev), src, first)
    torch.cuda.synchronize()
    got = slots.chunks(slots.buf.cpu().numpy())
    cand = {}
    for c, v in zip(pts, vals):
        cand.setdefault(tuple(c), []).append(int(v))
    for c, vs in cand.items():
        f = fate(meta, [0, 0], [6, 6], c)
        assert int(got[f[0]].reshape(meta.chunk_shape)[f[1]]) in vs, c
    # with the overwritten points dropped: exactly the last value, every other byte as before
    keep = points_last(np.array(pts, np.uint64))
    kept = [c for c, k in zip(pts, keep) if k]
    slots.reset()
    src2 = torch.from_numpy(vals[keep].view(np.uint8)).to(dev)
    scatter_points(meta, 2, table, [0, 0], [6, 6], coords_tensor(kept, dev), src2, first)
    torch.cuda.synchronize()
    assert len(kept) == len(cand)
    assert np.array_equal(slots.buf.cpu().numpy(), slots_model(slots, meta, "C", [0, 0], [6, 6], pts, vals))


def test_capture_and_replay_with_new_coordinates():
    """One captured zcg_read_points call (one stream, no parallel branch),
    replayed with new coordinates in the same buffer; the word is reset and
    lowered anew by every replay."""
    import torch
    meta, store = tiny_store()
    dev = store.dev
    rng = np.random.default_rng(12)
    P = 700
    sets = [[[int(rng.integers(0, 43)), int(rng.integers(0, 55))] for _ in range(P)] for _ in range(3)]
    table = torch.from_numpy(store.table([1, 0], [5, 6])).to(dev)  # chunk row 0 is outside the table
    coords = coords_tensor(sets[0], dev)
    out = torch.full((P * 2,), SENTINEL, dtype=torch.uint8, device=dev)
    first = word(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assemble_points(meta, 2, table, [1, 0], [5, 6], coords, out, first, True, 3)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assemble_points(meta, 2, table, [1, 0], [5, 6], coords, out, first, True, 3)
    for pts in sets[1:]:
        coords.copy_(coords_tensor(pts, dev))
        out.fill_(SENTINEL)
        first.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = oracle_values(meta, "C", pts, store.chunks.get, np.uint16, 1, 3, 0xA5A5)
        outside = [i for i, f in enumerate(fate(meta, [1, 0], [5, 6], c) for c in pts) if f is not None and not f[2]]
        want[outside] = 0xA5A5
        assert np.array_equal(out.cpu().numpy().view(np.uint16), want)
        assert word_value(first) == outside[0]  # the reset is part of the graph


@pytest.mark.parametrize("es,order", [(2, "C"), (8, "F")])
def test_coordinates_at_and_above_two_to_the_32(es, order):
    """Both division paths: an array of 2^33 + 100 x 40 elements whose few
    present chunks sit around index 2^33 along dimension 0 (the table is placed
    there by table_lo), so coordinates along dimension 0 take the 64-bit
    division and those along dimension 1 the multiplication; coordinates just
    below and above 2^32 meet in one wave.  test_points_equal_oracle_... has
    every extent below 2^32."""
    import torch
    rng = np.random.default_rng(es)
    shape, cs = [(1 << 33) + 100, 40], [61, 7]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    base = (1 << 33) - 150
    pts = [[base + int(rng.integers(0, 250)), int(rng.integers(0, 43))] for _ in range(300)]
    pts[7] = [shape[0] - 1, 39]
    pts[9] = [shape[0] + 3, 41]  # the overhang of the corner chunk
    lo, n = points_grid(meta, pts)
    assert lo[0] > (1 << 26) and n[0] <= 6
    pts[20] = [(1 << 32) - 1, 5]  # in the grid, outside the table, on either side of 2^32
    pts[21] = [1 << 32, 5]
    pts[30] = [U64_MAX, 3]
    store = Store(rng, meta, lo, n, es, order)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    dt = UINT[es]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    P = len(pts)
    out = torch.full((P * es,), SENTINEL, dtype=torch.uint8, device=dev)
    ref = torch.full((P * es,), SENTINEL, dtype=torch.uint8, device=dev)
    first = word(dev)
    assemble_points(meta, es, table, lo, n, coords_tensor(pts, dev), out, first, True, 0x77)
    status = torch.full((P,), -1, dtype=torch.int32, device=dev)
    vb = vboxes_tensor(pts, [[1, 1]] * P, [[1, 1]] * P, [ref.data_ptr() + i * es for i in range(P)])
    assemble_regions_v(meta, [1, 1], es, table, lo, n, vb, status, True, 0x77)
    torch.cuda.synchronize()
    outside = [i for i, f in enumerate(fate(meta, lo, n, c) for c in pts) if f is not None and not f[2]]
    assert outside[:2] == [20, 21]
    want = np.array([region_ref.read_ndarray(shape, cs, order, c, [1, 1], store.chunks.get, dt, 0x77).reshape(-1)[0]
                     for c in pts], dtype=dt)
    want[outside] = sent
    got = out.cpu().numpy()
    assert np.array_equal(got.view(dt), want)
    assert np.array_equal(got, ref.cpu().numpy()) and word_value(first) == 20
    assert [i for i, s in enumerate(status.cpu().tolist()) if s != _native.OK] == outside
