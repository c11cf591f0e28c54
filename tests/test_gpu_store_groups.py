"""Every store-level box and point call through the corners of the one group
loop (run_groups, zcg_boxes.cpp): read_ndarrays / _v / _s and read_points as
host arrays and as device tensors, write_ndarrays / _v / _s and write_points
from host and from device input, against a numpy model of the array, with all
chunks in one group (slot_budget_bytes=0) and with a budget of one decoded chunk
(one group per box, chunks shared between groups), and the _v entries through
ctypes with host buffers that are not consecutive (the bounce path).

The store is <u2, 12 x 10 in chunks of 4 x 5: a grid of 3 x 2 = six chunks (40
bytes decoded), one of them absent, fill value 513.  The six boxes, and the
twelve points, visit all six chunks; two boxes overlap (two points coincide),
so the order counts on the write side, and one box is empty, where the call
has a shape per box (the one-shape calls cannot have a single empty box)."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from test_gpu_write_boxes import check_store_equals, chunk_files, copy_store  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Raw, SliceDataChunk, _native  # noqa: E402
from zarr_amd.region import (BoundingBox, read_ndarrays, read_ndarrays_s, read_ndarrays_v, read_points,  # noqa: E402
                             write_ndarrays, write_ndarrays_s, write_ndarrays_v, write_points)

pytestmark = pytest.mark.gpu

SHAPE, CS, GRID = [12, 10], [4, 5], [3, 2]
ABSENT = (1, 1)
FILL = 513
D = 40  # bytes of a decoded chunk
CODECS = {"raw": Raw(), "gzip": Gzip(6)}
STORES = [(c, o) for c in ("raw", "gzip") for o in ("C", "F")]

# one shape for all boxes: 0 and 1 overlap, 2 and 5 overlap
ONE_SHAPE = [5, 4]
ONE_OFFSETS = [[0, 0], [3, 2], [7, 6], [7, 0], [0, 6], [6, 5]]
# a shape per box: 0 and 1 overlap, 3 and 5 overlap, 4 is empty; 3 covers chunk (2, 1) whole
V_OFFSETS = [[0, 0], [3, 4], [9, 0], [8, 5], [2, 2], [7, 7]]
V_SHAPES = [[5, 6], [6, 3], [3, 5], [4, 5], [0, 3], [4, 3]]
# strided: sample counts and steps; 0 and 1 share sample (3, 4), 3 and 5 share (11, 7), 4 is empty
S_COUNTS = [[5, 3], [3, 3], [3, 5], [2, 3], [0, 3], [3, 1]]
S_STEPS = [[1, 2], [2, 1], [1, 1], [3, 2], [1, 1], [2, 3]]
# points: 1 and 7 coincide; (5, 6), (7, 9) and (4, 5) lie in the absent chunk
POINTS = np.array([[0, 0], [3, 4], [2, 9], [5, 1], [5, 6], [7, 9], [11, 0], [3, 4], [8, 4], [9, 7], [11, 9], [4, 5]],
                  np.uint64)


def sl(c):
    return tuple(slice(g * k, (g + 1) * k) for g, k in zip(c, CS))


def make_store(root, codec, order):
    """-> hierarchy, metadata, the chunks written (coord -> flat chunk) and the
    numpy model of the array (the absent chunk as fill value)."""
    meta = ArrayMetadata.new(SHAPE, CS, "<u2", CODECS[codec])
    meta.chunk_memory_layout = order
    meta.fill_value = FILL
    h = FilesystemHierarchy.open_or_create(str(root))
    h.create_array("a", meta)
    rng = np.random.default_rng(77)
    chunks = {c: rng.integers(1000, 60000, int(np.prod(CS))).astype(np.uint16)
              for c in itertools.product(*[range(g) for g in GRID]) if c != ABSENT}
    h.write_chunks("a", meta, [SliceDataChunk(list(c), d) for c, d in chunks.items()])
    full = np.full(SHAPE, FILL, np.uint16)
    for c, d in chunks.items():
        full[sl(c)] = d.reshape(CS, order=order)
    return h, meta, chunks, full


def box_slices(off, count, step=(1, 1)):
    return tuple(slice(o, o + (n - 1) * s + 1 if n else o, s) for o, n, s in zip(off, count, step))


def chunks_of(slices):
    """The chunks that hold an index of the (strided) box."""
    mask = np.zeros(SHAPE, bool)
    mask[slices] = True
    return {c for c in itertools.product(*[range(g) for g in GRID]) if mask[sl(c)].any()}


def test_the_inputs_are_what_the_docstring_says():
    every = set(itertools.product(*[range(g) for g in GRID]))
    assert set().union(*[chunks_of(box_slices(o, ONE_SHAPE)) for o in ONE_OFFSETS]) == every
    assert set().union(*[chunks_of(box_slices(o, s)) for o, s in zip(V_OFFSETS, V_SHAPES)]) == every
    assert set().union(*[chunks_of(box_slices(o, n, s)) for o, n, s in zip(V_OFFSETS, S_COUNTS, S_STEPS)]) == every
    assert {tuple(int(x) // k for x, k in zip(p, CS)) for p in POINTS} == every
    assert chunks_of(box_slices(V_OFFSETS[3], V_SHAPES[3])) == {(2, 1)} and V_SHAPES[3] == CS


def tensor_boxes(res):
    """(uint8 tensor, ...) of an as_tensor read -> its bytes: the boxes back to
    back, each dense in the chunk memory order."""
    return res[0].cpu().numpy().tobytes()


def dense_bytes(boxes, order):
    return b"".join(np.asarray(b).flatten(order=order).tobytes() for b in boxes)


@pytest.mark.parametrize("codec,order", STORES)
def test_every_read_call_equals_the_model_in_one_group_and_in_many(tmp_path, codec, order):
    import torch
    h, meta, chunks, full = make_store(tmp_path, codec, order)
    vboxes = [BoundingBox(o, s) for o, s in zip(V_OFFSETS, V_SHAPES)]
    sboxes = [BoundingBox(o, n) for o, n in zip(V_OFFSETS, S_COUNTS)]
    want_one = [full[box_slices(o, ONE_SHAPE)] for o in ONE_OFFSETS]
    want_v = [full[box_slices(o, s)] for o, s in zip(V_OFFSETS, V_SHAPES)]
    want_s = [full[box_slices(o, n, s)] for o, n, s in zip(V_OFFSETS, S_COUNTS, S_STEPS)]
    want_p = full[tuple(POINTS[:, d].astype(np.int64) for d in range(2))]
    assert (want_p == FILL).sum() == 3 and any((w == FILL).any() for w in want_one + want_v + want_s)
    assert want_v[4].size == 0 and want_s[4].size == 0
    for budget in (0, D):
        kw = {"slot_budget_bytes": budget}
        got = read_ndarrays(h, "a", meta, ONE_OFFSETS, ONE_SHAPE, np.uint16, **kw)
        assert got.shape == (6, 5, 4) and np.array_equal(got, np.stack(want_one)), budget
        t = read_ndarrays(h, "a", meta, ONE_OFFSETS, ONE_SHAPE, np.uint16, as_tensor=True, **kw)
        assert tensor_boxes(t) == dense_bytes(want_one, order), budget
        for want, got, t in (
                (want_v, read_ndarrays_v(h, "a", meta, vboxes, np.uint16, **kw),
                 read_ndarrays_v(h, "a", meta, vboxes, np.uint16, as_tensor=True, **kw)),
                (want_s, read_ndarrays_s(h, "a", meta, sboxes, S_STEPS, np.uint16, **kw),
                 read_ndarrays_s(h, "a", meta, sboxes, S_STEPS, np.uint16, as_tensor=True, **kw))):
            assert len(got) == 6
            for b in range(6):
                assert got[b].shape == want[b].shape and np.array_equal(got[b], want[b]), (budget, b)
            assert tensor_boxes(t) == dense_bytes(want, order), budget
            sizes = [w.size * 2 for w in want]
            assert list(t[1]) == [sum(sizes[:b]) for b in range(6)]
        got = read_points(h, "a", meta, POINTS, np.uint16, **kw)
        assert got.dtype == np.uint16 and np.array_equal(got, want_p), budget
        t = read_points(h, "a", meta, POINTS, np.uint16, as_tensor=True, **kw)
        assert t.view(torch.uint8).cpu().numpy().tobytes() == want_p.tobytes(), budget


def model_write(chunks, full, slices, arrays):
    """The boxes assigned in order -> (the array afterwards, the coordinates of
    the chunks that then have a file)."""
    full = full.copy()
    touched = set()
    for s, a in zip(slices, arrays):
        full[s] = a
        touched |= chunks_of(s)
    return full, set(chunks) | touched


def check_writes(tmp_path, h0, meta, chunks, full, slices, arrays, calls):
    """calls: name -> f(hierarchy, slot_budget_bytes).  Every call leaves the
    store's decoded content equal to the model at budget 0, and the same chunk
    files byte for byte with a budget of one chunk."""
    order = meta.chunk_memory_layout
    after, keys = model_write(chunks, full, slices, arrays)
    assert ABSENT in keys and not np.array_equal(after, full)
    want = {c: after[sl(c)].flatten(order=order) for c in keys}
    for name, call in calls.items():
        ha = copy_store(tmp_path / "s0", tmp_path / (name + "_one"))
        call(ha, 0)
        check_store_equals(ha, tmp_path / (name + "_one"), meta, np.uint16, want)
        hb = copy_store(tmp_path / "s0", tmp_path / (name + "_many"))
        call(hb, D)
        assert chunk_files(tmp_path / (name + "_many")) == chunk_files(tmp_path / (name + "_one")), name


@pytest.mark.parametrize("codec,order", STORES)
def test_every_write_call_leaves_the_model_in_one_group_and_in_many(tmp_path, codec, order):
    import torch
    h0, meta, chunks, full = make_store(tmp_path / "s0", codec, order)
    rng = np.random.default_rng(3)
    dev = torch.device("cuda", 0)

    def draw(shape):
        return rng.integers(1, 500, shape).astype(np.uint16)

    def on_device(a):  # 2-byte elements; the calls go by the element size
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev)

    one = draw([6, *ONE_SHAPE])
    flat = np.concatenate([one[b].flatten(order=order) for b in range(6)])
    check_writes(tmp_path, h0, meta, chunks, full, [box_slices(o, ONE_SHAPE) for o in ONE_OFFSETS], list(one), {
        "one_host": lambda h, budget: write_ndarrays(h, "a", meta, ONE_OFFSETS, one, slot_budget_bytes=budget),
        "one_dev": lambda h, budget: write_ndarrays(h, "a", meta, ONE_OFFSETS,
                                                    torch.from_numpy(flat.view(np.uint8).copy()).to(dev),
                                                    shape=ONE_SHAPE, slot_budget_bytes=budget)})

    varied = [draw(s) for s in V_SHAPES]
    check_writes(tmp_path, h0, meta, chunks, full, [box_slices(o, s) for o, s in zip(V_OFFSETS, V_SHAPES)], varied, {
        "v_host": lambda h, budget: write_ndarrays_v(h, "a", meta, V_OFFSETS, varied, slot_budget_bytes=budget)})

    strided = [draw(n) for n in S_COUNTS]
    check_writes(tmp_path, h0, meta, chunks, full,
                 [box_slices(o, n, s) for o, n, s in zip(V_OFFSETS, S_COUNTS, S_STEPS)], strided, {
        "s_host": lambda h, budget: write_ndarrays_s(h, "a", meta, V_OFFSETS, S_STEPS, strided,
                                                     slot_budget_bytes=budget),
        "s_dev": lambda h, budget: write_ndarrays_s(h, "a", meta, V_OFFSETS, S_STEPS,
                                                    [on_device(a) for a in strided], slot_budget_bytes=budget)})

    vals = draw(len(POINTS))
    assert vals[1] != vals[7]
    check_writes(tmp_path, h0, meta, chunks, full, [tuple(int(x) for x in p) for p in POINTS], list(vals), {
        "p_host": lambda h, budget: write_points(h, "a", meta, POINTS, vals, slot_budget_bytes=budget),
        "p_dev": lambda h, budget: write_points(h, "a", meta, POINTS, on_device(vals), slot_budget_bytes=budget)})


def scattered(shapes, order, fill=None):
    """One numpy array per box, allocated from the last box to the first, so
    that the buffers do not lie back to back in box order."""
    bufs = [None] * len(shapes)
    for b in reversed(range(len(shapes))):
        bufs[b] = np.zeros(max(int(np.prod(shapes[b])), 1) + 8 * b, np.uint16)  # never the size of the gap
        if fill is not None:
            bufs[b][: fill[b].size] = fill[b].flatten(order=order)
    ptrs = [a.ctypes.data for a in bufs]
    assert any(ptrs[b + 1] != ptrs[b] + 2 * int(np.prod(shapes[b])) for b in range(len(shapes) - 1))
    return bufs, (ctypes.c_void_p * len(shapes))(*ptrs)


@pytest.mark.parametrize("codec,order", STORES)
def test_host_buffers_that_are_not_consecutive_go_through_the_bounce_path(tmp_path, codec, order):
    """zcg_store_read_boxes_v and zcg_store_write_boxes_v by ctypes: the
    results are the Python wrappers' (which always pass consecutive buffers)."""
    h0, meta, chunks, full = make_store(tmp_path / "s0", codec, order)
    st, am, msg = _native.array_meta_from_json(meta.to_json())
    assert st == _native.OK, msg
    ctx = _native.context(0)
    offs = np.ascontiguousarray(np.array(V_OFFSETS, np.uint64))
    shp = np.ascontiguousarray(np.array(V_SHAPES, np.uint64))
    path = b"a"
    vboxes = [BoundingBox(o, s) for o, s in zip(V_OFFSETS, V_SHAPES)]
    want = read_ndarrays_v(h0, "a", meta, vboxes, np.uint16)
    for budget in (0, D):
        bufs, outs = scattered(V_SHAPES, order)
        r = ctx.lib.zcg_store_read_boxes_v(ctx.handle, ctypes.byref(am), os.fsencode(h0.base_path), path,
                                           shp.ctypes.data, offs.ctypes.data, ctypes.addressof(outs), 6, budget, 16)
        assert r == _native.OK, ctx.last_error()
        for b in range(6):
            got = bufs[b][: want[b].size].reshape(want[b].shape, order=order)
            assert np.array_equal(got, want[b]) and np.array_equal(got, full[box_slices(V_OFFSETS[b], V_SHAPES[b])]), b
            assert not bufs[b][want[b].size:].any(), b  # nothing past the box

    rng = np.random.default_rng(4)
    arrays = [rng.integers(1, 500, s).astype(np.uint16) for s in V_SHAPES]
    hw = copy_store(tmp_path / "s0", tmp_path / "wrapper")
    write_ndarrays_v(hw, "a", meta, V_OFFSETS, arrays)
    for budget in (0, D):
        root = tmp_path / f"ctypes_{budget}"
        hc = copy_store(tmp_path / "s0", root)
        bufs, ins = scattered(V_SHAPES, order, fill=arrays)
        r = ctx.lib.zcg_store_write_boxes_v(ctx.handle, ctypes.byref(am), os.fsencode(hc.base_path), path,
                                            shp.ctypes.data, offs.ctypes.data, ctypes.addressof(ins), 6, budget, 16)
        assert r == _native.OK, ctx.last_error()
        assert chunk_files(root) == chunk_files(tmp_path / "wrapper"), budget
