"""read_ndarrays_s (zcg_store_read_boxes_s[_device]): many strided boxes from a
store in one native call, against the oracle's read_ndarray of each box's hull
sliced [::step]; only the chunks that hold a sample are read."""
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
from test_gpu_write_boxes import random_store, snapshot, truncate  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Lz4, Raw, SliceDataChunk  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.region import (BoundingBox, _strides, read_ndarray, read_ndarrays_s, read_ndarrays_v,  # noqa: E402
                             region_s_chunks)

pytestmark = pytest.mark.gpu


def hull_of(counts, steps):
    return [(c - 1) * s + 1 if c else 0 for c, s in zip(counts, steps)]


def sliced_hull(meta, chunks, off, counts, steps, npdt, fill):
    H = region_ref.read_ndarray(meta.shape, meta.chunk_shape, meta.chunk_memory_layout, off, hull_of(counts, steps),
                                chunks.get, npdt, fill)
    return H[tuple(slice(None, None, int(s)) for s in steps)]


def touched_chunks(meta, off, counts, steps):
    lo, n, touched, count = region_s_chunks(meta, off, counts, steps)
    if not count:
        return []
    return list(itertools.product(*[[lo[d] + j for j in range(n[d]) if touched[d][j]] for d in range(len(lo))]))


def draw_boxes(rng, meta, B):
    """B strided boxes (0-8 samples per dimension, or 0-5 from three dimensions
    on; steps from 1 to twice the chunk extent plus 1), partly outside the
    array and overlapping, every touched chunk inside the array's chunk grid."""
    shape, cs = meta.shape, meta.chunk_shape
    nd = len(shape)
    boxes, steps = [], []
    while len(boxes) < B:
        off = [int(rng.integers(0, s + 3)) for s in shape]
        cnt = [int(rng.integers(0 if len(boxes) % 5 == 3 else 1, 9 if nd < 3 else 6)) for _ in range(nd)]
        stp = [int(rng.choice([1, 2, 3, c, c + 1, 2 * c + 1])) for c in cs]
        if all(meta.in_bounds(c) for c in touched_chunks(meta, off, cnt, stp)):
            boxes.append(BoundingBox(off, cnt))
            steps.append(stp)
    return boxes, steps


@pytest.mark.parametrize("seed", range(3))
def test_read_ndarrays_s_vs_the_sliced_hull(tmp_path, seed):
    """A raw, a gzip and an lz4 store with ~25 % absent chunks: read_ndarrays_s
    with 30 strided boxes equals the oracle's read_ndarray of each hull, sliced,
    as host arrays and as a device tensor; a slot budget of two chunks, which
    forces several groups, changes nothing.  One box is also compared with the
    package's own read_ndarray of the hull."""
    rng, h, meta, npdt, chunks = random_store(tmp_path, seed)
    B = 30
    boxes, steps = draw_boxes(rng, meta, B)
    assert len({c for bb, s in zip(boxes, steps) for c in touched_chunks(meta, bb.offset, bb.shape, s)}) > 2
    fill = 7 if meta.fill_value is not None else 0
    order = meta.chunk_memory_layout
    want = [sliced_hull(meta, chunks, bb.offset, bb.shape, s, npdt, fill) for bb, s in zip(boxes, steps)]
    es = npdt.itemsize
    for budget in (0, 2 * int(np.prod(meta.chunk_shape)) * es):
        got = read_ndarrays_s(h, "a", meta, boxes, steps, npdt, slot_budget_bytes=budget)
        assert len(got) == B
        for b in range(B):
            assert got[b].shape == tuple(boxes[b].shape) and got[b].dtype == npdt
            assert np.array_equal(got[b], want[b]), (seed, budget, b, boxes[b], steps[b])
        t, at, strides = read_ndarrays_s(h, "a", meta, boxes, steps, npdt, as_tensor=True, slot_budget_bytes=budget)
        raw = t.cpu().numpy()
        assert len(raw) == sum(w.nbytes for w in want)
        for b in range(B):
            assert strides[b] == _strides(boxes[b].shape, order)
            view = np.ndarray(tuple(boxes[b].shape), dtype=npdt, buffer=raw, offset=at[b],
                              strides=tuple(s * es for s in strides[b]))
            assert np.array_equal(view, want[b]), (seed, budget, b)
    # one step vector for all boxes; and the package's own dense read of a hull, sliced
    one = steps[0]
    got = read_ndarrays_s(h, "a", meta, boxes[:4], one, npdt)
    for b in range(4):
        assert np.array_equal(got[b], sliced_hull(meta, chunks, boxes[b].offset, boxes[b].shape, one, npdt, fill))
    b = next(b for b in range(B) if 0 not in boxes[b].shape)
    hull = BoundingBox(boxes[b].offset, hull_of(boxes[b].shape, steps[b]))
    if all(meta.in_bounds(c) for c in region_ref.bounded_coord_iter(meta.shape, meta.chunk_shape, hull.offset,
                                                                    hull.shape)):
        dense = read_ndarray(h, "a", meta, hull, npdt)
        assert np.array_equal(dense[tuple(slice(None, None, s) for s in steps[b])], want[b])
    assert read_ndarrays_s(h, "a", meta, [], [1] * meta.get_ndim(), npdt) == []


def grid_store(tmp_path, comp):
    """A 40 x 48 i4 array in 4 x 6 chunks, every chunk present."""
    meta = ArrayMetadata.new([40, 48], [4, 6], "<i4", comp)
    meta.chunk_memory_layout = "C"
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    rng = np.random.default_rng(12)
    chunks = {c: rng.integers(0, 100000, 24).astype(np.int32) for c in itertools.product(range(10), range(8))}
    h.write_chunks("a", meta, [SliceDataChunk(list(c), d) for c, d in chunks.items()])
    return h, meta, chunks


@pytest.mark.parametrize("steps", [[8, 12], [4, 12], [9, 7]])
@pytest.mark.parametrize("comp", [Gzip(6), Lz4(65536)], ids=["gzip", "lz4"])
def test_untouched_chunk_files_are_never_opened(tmp_path, comp, steps):
    """Every chunk file in the hull's range that holds no sample is overwritten
    with bytes that are no stream of the codec.  The strided read (steps of at
    least the chunk extent) still succeeds and is exact, as host arrays and as
    a device tensor; the dense read of the hull raises: the files matter to the
    dense path only."""
    h, meta, chunks = grid_store(tmp_path, comp)
    off, counts = [1, 2], [4, 4]
    hull = BoundingBox(off, hull_of(counts, steps))
    touched = set(touched_chunks(meta, off, counts, steps))
    in_range = region_ref.bounded_coord_iter(meta.shape, meta.chunk_shape, hull.offset, hull.shape)
    untouched = [c for c in in_range if c not in touched]
    assert touched and untouched and touched <= set(in_range)
    want = sliced_hull(meta, chunks, off, counts, steps, np.int32, 0)
    for c in untouched:
        with open(h.chunk_path("a", meta, list(c)), "wb") as f:
            f.write(b"\xff" * 37)
    got = read_ndarrays_s(h, "a", meta, [BoundingBox(off, counts)], steps, np.int32)
    assert np.array_equal(got[0], want)
    t, at, strides = read_ndarrays_s(h, "a", meta, [BoundingBox(off, counts)], [steps], np.int32, as_tensor=True)
    assert np.array_equal(t.cpu().numpy().view(np.int32).reshape(counts), want)
    with pytest.raises(ZarrIOError):
        read_ndarrays_v(h, "a", meta, [hull], np.int32)


def test_corrupt_touched_chunk_raises_its_status_and_names_the_chunk(tmp_path):
    h, meta, chunks = grid_store(tmp_path, Gzip(6))
    truncate(h.chunk_path("a", meta, [2, 4]))
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [2, 4], np.int32)
    box, steps = BoundingBox([1, 2], [4, 4]), [8, 12]
    assert (2, 4) in touched_chunks(meta, box.offset, box.shape, steps)
    with pytest.raises(ZarrIOError) as ei:
        read_ndarrays_s(h, "a", meta, [BoundingBox([0, 0], [2, 2]), box], [[1, 1], steps], np.int32)
    assert ei.value.kind == single.value.kind and "chunk [2, 4]" in str(ei.value)


def test_only_a_touched_chunk_outside_the_grid_is_invalid_input(tmp_path):
    """Shape 10, chunk 4: the grid has chunks 0 .. 2.  A box whose first sample
    is element 13 touches chunk 3, where the reference panics (storage.rs:217):
    InvalidInput before any file is read.  The hull's range of a box without
    samples at that offset still names chunk 3, which holds no sample: no
    error, and nothing is read."""
    meta = ArrayMetadata.new([10], [4], "<i2")
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    h.write_chunks("a", meta, [SliceDataChunk([0], np.arange(4, dtype=np.int16))])
    truncate(h.chunk_path("a", meta, [0]))  # a read would fail with another status
    before = snapshot(tmp_path)
    with pytest.raises(ZarrIOError) as ei:
        read_ndarrays_s(h, "a", meta, [BoundingBox([0], [3]), BoundingBox([13], [2])], [[1], [3]], np.int16)
    assert ei.value.kind == "InvalidInput" and "chunk [3]" in str(ei.value)
    lo, n, touched, count = region_s_chunks(meta, [13], [0], [3])
    assert (lo, n, touched, count) == ([3], [1], [[0]], 0)
    got = read_ndarrays_s(h, "a", meta, [BoundingBox([13], [0]), BoundingBox([5], [2])], [[3], [4]], np.int16)
    assert got[0].shape == (0,) and got[1].tolist() == [0, 0]  # elements 5 and 9: absent chunks, filled
    assert snapshot(tmp_path) == before


def test_plain_c_caller_reads_two_strided_boxes(tmp_path):
    """tests/c_abi_s/boxes_s_c.c, built by its own Makefile, reads 2x2x3
    samples with steps 2,3,2 and 2x3x2 samples with steps 1,2,4 of the zarrita
    fixture with one zcg_store_read_boxes_s call."""
    c_abi = os.path.join(ROOT, "tests", "c_abi_s")
    r = subprocess.run(["make", "-s", "-C", c_abi], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(c_abi, "boxes_s_c")
    store = os.path.join(ROOT, "tests", "golden", "zarrita")
    outf = str(tmp_path / "boxes.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "boxes_s_c: ok (2 boxes" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(outf, "<i2")
    chunks = {g: v for g, _, v in zarrita_chunks()}
    at = 0
    for off, cnt, stp in (([0, 1, 0], [2, 2, 3], [2, 3, 2]), ([2, 0, 1], [2, 3, 2], [1, 2, 4])):
        hull = region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", off, hull_of(cnt, stp), chunks.get, np.int16, 0)
        want = hull[::stp[0], ::stp[1], ::stp[2]]
        assert np.array_equal(got[at:at + want.size].reshape(cnt), want), off
        at += want.size
    assert at == got.size
