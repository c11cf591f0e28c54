"""Orthogonal selections on the GPU: zcg_read_ortho / zcg_write_ortho (an index
list per dimension, the result their Cartesian product) against
zcg_read_points on the expanded product, bit for bit, and against the numpy
oracle's hull (oracle/region_ref.py) indexed by np.ix_.  Whole buffers are
compared, with sentinel bytes around and between the view's elements."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes import SENTINEL, TYPESTR, UINT, Store  # noqa: E402
from test_gpu_points import (CASES, GAP, U64_MAX, coords_tensor, fate, oracle_values, slots_model,  # noqa: E402
                             word, word_value)
from test_gpu_write_boxes import Slots  # noqa: E402
from zarr_amd import ArrayMetadata, _native  # noqa: E402
from zarr_amd.region import (_strides, assemble_ortho, assemble_points, ortho_chunks, ortho_scratch_bytes,  # noqa: E402
                             points_last, scatter_ortho)

pytestmark = pytest.mark.gpu

SHAPE3, CS3 = [10, 9, 14], [4, 3, 5]


def meta3(typestr):
    """The 10 x 9 x 14 array in 4 x 3 x 5 chunks, C order."""
    meta = ArrayMetadata.new(SHAPE3, CS3, typestr)
    meta.chunk_memory_layout = "C"
    return meta


def list_tensor(a, dev):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).copy()).to(dev)


def words(nd, dev, start=0):
    import torch
    return torch.full((nd,), start, dtype=torch.int64, device=dev)


def words_value(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def product(lists):
    return [list(c) for c in itertools.product(*lists)]


class View:
    """A view of `counts` elements in a sentinel-filled buffer: `kind` 0 dense
    in the chunk memory order `order` (the fast dimension has stride 1), 1
    dense in the other order (a unit stride on a dimension that is not the
    chunks' fast one), 2 every stride times 3 and negative along the first and
    the last dimension (two sentinel elements between neighbours)."""

    def __init__(self, counts, order, es, kind):
        nd = len(counts)
        total = int(np.prod(counts))
        if kind == 0:
            self.strides, self.base, elems = _strides(counts, order), 0, total
        elif kind == 1:
            self.strides, self.base, elems = _strides(counts, "C" if order == "F" else "F"), 0, total
        else:
            dense = _strides(counts, "C")
            sign = [-1 if d in (0, nd - 1) else 1 for d in range(nd)]
            self.strides = [3 * s * g for s, g in zip(dense, sign)]
            self.base = sum((c - 1) * -s for c, s in zip(counts, self.strides) if s < 0)
            elems = 3 * total
        self.counts, self.es, self.bytes = counts, es, 2 * GAP + elems * es
        at = np.full(counts, self.base, dtype=np.int64)
        for d in range(nd):
            at += (np.arange(counts[d], dtype=np.int64) * self.strides[d]).reshape([-1 if k == d else 1 for k in range(nd)])
        self.at = at.reshape(-1)  # element offset of every position, C order
        assert self.at.min() >= 0 and self.at.max() < elems and len(set(self.at.tolist())) == total

    def empty(self, dev):
        import torch
        return torch.full((self.bytes,), SENTINEL, dtype=torch.uint8, device=dev)

    def place(self, dense):
        """The buffer that holds `dense` (the values in C order over the positions) and sentinels elsewhere."""
        buf = np.full(self.bytes, SENTINEL, np.uint8)
        buf[GAP:self.bytes - GAP].view(dense.dtype)[self.at] = dense.reshape(-1)
        return buf

    def ptr_tensor(self, buf):
        return buf[GAP + self.base * self.es:]


def same(got, want, what=None):
    """Whole-buffer equality; a failure names the first bytes that differ."""
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad.size), [(int(i), int(got[i]), int(want[i])) for i in bad[:12]])
    return True


def gather(meta, es, table, lo, n, lists, view, fill, fillv, dev, start=0):
    """assemble_ortho into a fresh sentinel buffer -> (its bytes, the outside words)."""
    import torch
    out = view.empty(dev)
    outside = words(len(lists), dev, start)
    assemble_ortho(meta, es, table, lo, n, [list_tensor(a, dev) for a in lists], view.ptr_tensor(out), view.strides,
                   outside, bool(fill), fillv)
    torch.cuda.synchronize()
    return out.cpu().numpy(), words_value(outside)


def points_dense(meta, es, table, lo, n, pts, fill, fillv, dev):
    """assemble_points on `pts` into sentinels -> (the values, the first-outside word)."""
    import torch
    out = torch.full((len(pts) * es,), SENTINEL, dtype=torch.uint8, device=dev)
    first = word(dev)
    assemble_points(meta, es, table, lo, n, coords_tensor(pts, dev), out, first, bool(fill), fillv)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(UINT[es]), word_value(first)


def outside_words(meta, lo, n, lists):
    """Per dimension the lowest position whose index visits a grid index outside lo .. lo+n."""
    res = []
    for d, L in enumerate(lists):
        cs, a = meta.chunk_shape[d], meta.shape[d]
        bad = [i for i, x in enumerate(L) if (x < a or x % cs) and not lo[d] <= x // cs < lo[d] + n[d]]
        res.append(bad[0] if bad else U64_MAX)
    return res


def draw_lists(rng, meta, per_dim):
    """Per dimension `per_dim` indices inside the array, unsorted, then: a
    duplicate, the array's last index, where the edge chunk overhangs the
    index just beyond the array, and the first index beyond the grid (which
    visits nothing).  With 8 dimensions each of the three extras goes to one
    dimension only, so the product stays small."""
    shape, chunk = meta.shape, meta.chunk_shape
    nd = len(shape)
    over = next(d for d in range(nd) if shape[d] % chunk[d])
    lists = []
    for d, (s, cs) in enumerate(zip(shape, chunk)):
        L = [int(x) for x in rng.integers(0, s, per_dim)]
        if nd < 8 or d == 0:
            L.insert(1, L[0])
        L.append(s - 1)
        if s % cs and (nd < 8 or d == over):
            L.insert(2, s)
        if d == 0 or (d != 1 and nd < 8):  # not along every dimension, or few elements are left with a chunk
            L.insert(0, -(-s // cs) * cs)
        lists.append(L)
    return lists


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_ortho_equals_points_on_the_product_and_the_oracle_hull(seed):
    """The 8 cases of the point tests (1, 2, 3 and 8 dimensions, element sizes
    1/2/4/8, C and F order), fill off and on, three views (View), lists with
    the entries of draw_lists, one touched chunk absent.  The table holds
    every visited chunk, so the words stay UINT64_MAX."""
    import torch
    rng = np.random.default_rng(71000 + seed)
    nd, cs, shape = CASES[seed]
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lists = draw_lists(rng, meta, {1: 40, 2: 9, 3: 6, 8: 1}[nd])
    counts = [len(L) for L in lists]
    pts = product(lists)
    lo, n, _, touched = ortho_chunks(meta, lists)
    store = Store(rng, meta, lo, n, es, order, absent_frac=0.0)
    gone = fate(meta, lo, n, [L[-1] for L in lists])[0]  # the chunk of the array's last index is absent
    del store.chunks[gone], store.ptr[gone]
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    dt = UINT[es]
    fillv = 0x1122334455667788 & ((1 << (8 * es)) - 1)
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    fates = [fate(meta, lo, n, c) for c in pts]
    assert any(f is None for f in fates) and all(f[2] for f in fates if f) and touched > 1
    # the oracle's hull under np.ix_, for the entries inside the array
    near = [[i for i, x in enumerate(L) if x < s] for L, s in zip(lists, shape)]
    off = [min(lists[d][i] for i in near[d]) for d in range(nd)]
    hshape = [max(lists[d][i] for i in near[d]) - off[d] + 1 for d in range(nd)]
    ix = np.ix_(*[[lists[d][i] - off[d] for i in near[d]] for d in range(nd)])
    for fill in (0, 1):
        want = oracle_values(meta, order, pts, store.chunks.get, dt, fill, fillv, sent)
        hull = np.full(tuple(hshape), sent, dtype=dt)
        if fill:
            hull = region_ref.read_ndarray(shape, cs, order, off, hshape, store.chunks.get, dt, fillv)
        else:
            region_ref.read_ndarray_into(shape, cs, order, off, hshape, store.chunks.get, hull)
        assert np.array_equal(want.reshape(counts)[np.ix_(*near)], hull[ix])
        got_pts, first = points_dense(meta, es, table, lo, n, pts, fill, fillv, dev)
        assert np.array_equal(got_pts, want) and first == U64_MAX
        for kind in (0, 1, 2):
            view = View(counts, order, es, kind)
            got, outside = gather(meta, es, table, lo, n, lists, view, fill, fillv, dev)
            assert same(got, view.place(want), (seed, fill, kind))
            assert outside == [U64_MAX] * nd


def edge_counts():
    res = []
    for es in (2, 8):
        V = 16 // es
        for c in sorted({1, V - 1, V, V + 1, 64 * V - 1, 64 * V, 64 * V + 1, 256 * V + 1}):
            res.append((es, c))
    return res


@pytest.mark.parametrize("es,count", edge_counts())
def test_fast_axis_counts_at_the_edges_of_a_piece_a_wave_and_a_workgroup(es, count):
    """`count` indices along the chunks' fast dimension, drawn with repetition
    from the 10 x 9 x 14 array and the overhang of its edge chunk, 3 x 2 along
    the slow ones; V = 16 / es elements make a 16-byte piece.  Fill on, the
    dense view (whole pieces are stored at once) and the strided one."""
    import torch
    rng = np.random.default_rng(100 * es + count)
    meta = meta3(TYPESTR[es])
    lists = [[int(x) for x in rng.integers(0, 12, 3)], [int(x) for x in rng.integers(0, 9, 2)],
             [int(x) for x in rng.integers(0, 15, count)]]
    store = Store(rng, meta, [0, 0, 0], [3, 3, 3], es, "C")
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    pts = product(lists)
    sent = np.frombuffer(bytes([SENTINEL]) * 8, UINT[es])[0]
    want = oracle_values(meta, "C", pts, store.chunks.get, UINT[es], 1, 0xBEEF, sent)
    for kind in (0, 2):
        view = View([3, 2, count], "C", es, kind)
        got, outside = gather(meta, es, table, [0, 0, 0], [3, 3, 3], lists, view, 1, 0xBEEF, dev)
        assert same(got, view.place(want), kind)
        assert outside == [U64_MAX] * 3


@pytest.mark.parametrize("es,order", [(2, "C"), (8, "F")])
def test_indices_at_and_above_two_to_the_32(es, order):
    """The array of 2^33 + 100 x 40 elements of the point tests, its table near
    grid index 2^27 along dimension 0: indices 2^32-1 and 2^32 side by side (in
    the grid, outside the table), 2^63 and 2^64-1, among indices around 2^33.
    Both division paths of the axis kernel; the word of dimension 0 names the
    first of them."""
    import torch
    rng = np.random.default_rng(es)
    shape, cs = [(1 << 33) + 100, 40], [61, 7]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    base = (1 << 33) - 150
    rows = [base + int(x) for x in rng.integers(0, 250, 40)] + [shape[0] - 1, shape[0] + 3]
    cols = [int(x) for x in rng.integers(0, 43, 9)] + [39, 41]
    lo, n, _, _ = ortho_chunks(meta, [rows, cols])
    assert lo[0] > (1 << 26) and n[0] <= 6
    rows[20:20] = [(1 << 32) - 1, 1 << 32]
    rows[30:30] = [1 << 63, U64_MAX]
    lists = [rows, cols]
    store = Store(rng, meta, lo, n, es, order)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    dt = UINT[es]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    pts = product(lists)
    fates = [fate(meta, lo, n, c) for c in pts]
    skipped = [i for i, f in enumerate(fates) if f is not None and not f[2]]
    assert skipped and outside_words(meta, lo, n, lists)[0] == 20
    want = np.array([region_ref.read_ndarray(shape, cs, order, c, [1, 1], store.chunks.get, dt, 0x77).reshape(-1)[0]
                     for c in pts], dtype=dt)
    want[skipped] = sent
    got_pts, first = points_dense(meta, es, table, lo, n, pts, 1, 0x77, dev)
    assert np.array_equal(got_pts, want) and first == skipped[0]
    view = View([len(rows), len(cols)], order, es, 0)
    got, outside = gather(meta, es, table, lo, n, lists, view, 1, 0x77, dev)
    assert same(got, view.place(want))
    assert outside == outside_words(meta, lo, n, lists) and outside[1] == U64_MAX


@pytest.mark.parametrize("fill", [0, 1])
def test_outside_words_of_a_table_pruned_along_two_dimensions(fill):
    """The table leaves out grid index 0 along dimensions 0 and 2: per dimension
    the lowest position of an index in a left-out chunk, UINT64_MAX along
    dimension 1; the elements of those positions keep their sentinels unless an
    index of theirs visits no chunk (the point rule: such an element is filled),
    all others are right."""
    import torch
    rng = np.random.default_rng(8)
    meta = meta3("<u4")
    lists = [[9, 5, 2, 8, 1, 12, 7], [0, 8, 4, 9], [13, 6, 11, 3, 14, 0, 9, 15]]
    lo, n = [1, 0, 1], [2, 3, 2]
    store = Store(rng, meta, [0, 0, 0], [3, 3, 3], 4, "C")
    dev = store.dev
    table = torch.from_numpy(store.table(lo, n)).to(dev)
    assert outside_words(meta, lo, n, lists) == [2, U64_MAX, 3]
    pts = product(lists)
    fates = [fate(meta, lo, n, c) for c in pts]
    skipped = [i for i, f in enumerate(fates) if f is not None and not f[2]]
    sent = np.uint32(0xA5A5A5A5)
    want = oracle_values(meta, "C", pts, store.chunks.get, np.uint32, fill, 0x01020304, sent)
    want[skipped] = sent
    got_pts, first = points_dense(meta, 4, table, lo, n, pts, fill, 0x01020304, dev)
    assert np.array_equal(got_pts, want) and first == skipped[0]
    for kind in (0, 2):
        view = View([7, 4, 8], "C", 4, kind)
        got, outside = gather(meta, 4, table, lo, n, lists, view, fill, 0x01020304, dev, start=7)
        assert same(got, view.place(want), kind)
        assert outside == [2, U64_MAX, 3]


def scatter(meta, es, slots, lo, n, lists, view, vals, dev):
    """scatter_ortho of `vals` (C order over the positions) from `view` -> the outside words."""
    import torch
    src = torch.from_numpy(view.place(vals)).to(dev)
    before = src.clone()
    outside = words(len(lists), dev)
    scatter_ortho(meta, es, torch.from_numpy(slots.table(lo, n)).to(dev), lo, n, [list_tensor(a, dev) for a in lists],
                  view.ptr_tensor(src), view.strides, outside)
    torch.cuda.synchronize()
    assert torch.equal(src, before)  # the values are only read
    return words_value(outside)


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_scatter_equals_the_numpy_model_byte_for_byte(seed):
    """The cases and lists of the gather test without the duplicates, ~25 % of
    the slots NULL, the strided view: every byte of the slot buffer (guard
    bytes and NULL slots' bytes included) against the point model.  Then a
    table pruned along dimension 0: the left-out chunks keep their bytes."""
    rng = np.random.default_rng(72000 + seed)
    nd, cs, shape = CASES[seed]
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lists = [sorted(set(L), key=L.index) for L in draw_lists(rng, meta, {1: 40, 2: 9, 3: 6, 8: 1}[nd])]
    counts = [len(L) for L in lists]
    lo, n, _, _ = ortho_chunks(meta, lists)
    slots = Slots(rng, meta, lo, n, es)
    pts = product(lists)
    vals = rng.integers(0, 256, len(pts) * es, dtype=np.uint8).view(UINT[es])
    for kind, plo, pn in ((2, lo, n), (0, [lo[0] + 1] + lo[1:], [n[0] - 1] + n[1:])):
        slots.reset()
        outside = scatter(meta, es, slots, plo, pn, lists, View(counts, order, es, kind), vals, slots.dev)
        model = slots_model(slots, meta, order, plo, pn, pts, vals)
        assert same(slots.buf.cpu().numpy(), model, (seed, kind))
        assert outside == outside_words(meta, plo, pn, lists)
    assert outside[0] != U64_MAX and outside[1:] == [U64_MAX] * (nd - 1)


def test_scatter_with_duplicates_leaves_one_value_and_points_last_the_last():
    rng = np.random.default_rng(4)
    meta = meta3("<u2")
    slots = Slots(rng, meta, [0, 0, 0], [3, 3, 3], 2, absent_frac=0.0)
    lists = [[int(x) for x in rng.integers(0, 6, 14)], [int(x) for x in rng.integers(0, 5, 9)],
             [int(x) for x in rng.integers(0, 8, 40)]]
    counts = [14, 9, 40]
    pts = product(lists)
    vals = (np.arange(len(pts)) + 1000).astype(np.uint16)
    scatter(meta, 2, slots, [0, 0, 0], [3, 3, 3], lists, View(counts, "C", 2, 0), vals, slots.dev)
    got = slots.chunks(slots.buf.cpu().numpy())
    cand = {}
    for c, v in zip(pts, vals):
        cand.setdefault(tuple(c), []).append(int(v))
    assert max(len(v) for v in cand.values()) > 20
    for c, vs in cand.items():
        f = fate(meta, [0, 0, 0], [3, 3, 3], c)
        assert int(got[f[0]].reshape(CS3)[f[1]]) in vs, c
    # with the earlier duplicates dropped per list: exactly the last value, every other byte as before
    keep = [points_last(np.array(L, np.uint64).reshape(-1, 1)) for L in lists]
    kept = [[x for x, k in zip(L, m) if k] for L, m in zip(lists, keep)]
    slots.reset()
    scatter(meta, 2, slots, [0, 0, 0], [3, 3, 3], kept, View([len(L) for L in kept], "C", 2, 2),
            vals.reshape(counts)[np.ix_(*[np.flatnonzero(m) for m in keep])].reshape(-1), slots.dev)
    assert len(product(kept)) == len(cand)
    model = slots_model(slots, meta, "C", [0, 0, 0], [3, 3, 3], pts, vals)
    assert same(slots.buf.cpu().numpy(), model)


def test_zero_counts_launch_nothing_and_bad_arguments_are_refused():
    import torch
    meta = meta3("<u2")
    store = Store(np.random.default_rng(1), meta, [0, 0, 0], [3, 3, 3], 2, "C")
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=dev)
    outside = words(3, dev, 5)
    scratch = torch.empty(ortho_scratch_bytes([2, 2, 2]), dtype=torch.uint8, device=dev)
    idx = list_tensor([1, 2], dev)
    ctx = _native.context(0)
    r = _native.Region()
    r.ndim, r.elem_size = 3, 2
    for d in range(3):
        r.array_shape[d], r.chunk_shape[d] = SHAPE3[d], CS3[d]
    lo, n = (ctypes.c_uint64 * 8)(0, 0, 0), (ctypes.c_uint64 * 8)(3, 3, 3)
    sel = _native.OSel()
    for d in range(3):
        sel.index[d], sel.count[d], sel.strides[d] = idx.data_ptr(), 2, [4, 2, 1][d]
    sel.base = out.data_ptr()

    def call(fn=ctx.lib.zcg_read_ortho, s=sel, scr=scratch, w=outside):
        return fn(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n), table.data_ptr(),
                  ctypes.addressof(s) if s is not None else None, scr.data_ptr() if scr is not None else None,
                  w.data_ptr() if w is not None else None, None)

    def untouched():
        torch.cuda.synchronize()
        return words_value(outside) == [5, 5, 5] and bool((out.cpu().numpy() == SENTINEL).all())

    for d in range(3):  # a zero count: ZCG_OK, not even the reset
        sel.count[d] = 0
        assert call() == _native.OK and call(ctx.lib.zcg_write_ortho) == _native.OK
        sel.count[d] = 2
    assert untouched()
    # NULL arguments
    assert call(s=None) == _native.INVALID_INPUT
    assert call(scr=None) == _native.INVALID_INPUT and call(w=None) == _native.INVALID_INPUT
    assert call(scr=scratch[8:]) == _native.INVALID_INPUT  # records are read with 16-byte loads
    sel.index[1] = None
    assert call() == _native.INVALID_INPUT
    sel.index[1] = idx.data_ptr()
    sel.base = None
    assert call() == _native.INVALID_INPUT and call(ctx.lib.zcg_write_ortho) == _native.INVALID_INPUT
    sel.base = out.data_ptr()
    # the point calls' codes for the descriptor
    for field, value in (("ndim", 0), ("ndim", 9), ("elem_size", 3)):
        keep = getattr(r, field)
        setattr(r, field, value)
        assert call() == _native.INVALID_INPUT
        setattr(r, field, keep)
    r.chunk_shape[1] = 0
    assert call() == _native.INVALID_INPUT
    r.chunk_shape[1] = CS3[1]
    # the limits: a list of 2^32 entries, a product of 2^60
    sel.count[2] = 1 << 32
    assert call() == _native.UNSUPPORTED and "2^32" in ctx.last_error()
    sel.count[0], sel.count[1], sel.count[2] = 1 << 20, 1 << 20, 1 << 20
    assert call() == _native.UNSUPPORTED and "2^60" in ctx.last_error()
    assert untouched()
    sel.count[0], sel.count[1], sel.count[2] = 2, 2, 2
    r.bbox_shape[0] = 1 << 40  # ignored
    assert call() == _native.OK
    torch.cuda.synchronize()
    assert words_value(outside) == [U64_MAX] * 3


def test_capture_and_replay_with_new_indices():
    """One captured zcg_read_ortho call (one stream, no parallel branch),
    replayed with each of three index sets in the same lists, the set it was
    captured with last; the words are reset and lowered anew by every replay."""
    import torch
    rng = np.random.default_rng(13)
    meta = meta3("<u2")
    store = Store(rng, meta, [0, 0, 0], [3, 3, 3], 2, "C")
    dev = store.dev
    lo, n = [1, 0, 0], [2, 3, 3]  # grid index 0 along dimension 0 is outside the table
    table = torch.from_numpy(store.table(lo, n)).to(dev)
    counts = [6, 5, 37]
    sets = [[[int(x) for x in rng.integers(0, s + 1, c)] for s, c in zip(SHAPE3, counts)] for _ in range(3)]
    for lists in sets:
        lists[0][3] = 1  # outside
    view = View(counts, "C", 2, 0)
    tens = [list_tensor(a, dev) for a in sets[0]]
    out = view.empty(dev)
    outside = words(3, dev)
    scratch = torch.empty(ortho_scratch_bytes(counts), dtype=torch.uint8, device=dev)

    def call():
        assemble_ortho(meta, 2, table, lo, n, tens, view.ptr_tensor(out), view.strides, outside, True, 3,
                       scratch=scratch)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for lists in sets[1:] + sets[:1]:  # two new sets, then the captured one again: three replays
        for t, a in zip(tens, lists):
            t.copy_(list_tensor(a, dev))
        out.fill_(SENTINEL)
        outside.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        pts = product(lists)
        want = oracle_values(meta, "C", pts, store.chunks.get, np.uint16, 1, 3, 0xA5A5)
        skipped = [i for i, f in enumerate(fate(meta, lo, n, c) for c in pts) if f is not None and not f[2]]
        want[skipped] = 0xA5A5
        assert same(out.cpu().numpy(), view.place(want))
        assert words_value(outside) == outside_words(meta, lo, n, lists) and words_value(outside)[0] <= 3
