"""read_points / write_points (zcg_store_read_points[_device],
zcg_store_write_points[_device]): a[coords] and a[coords] = values on a store in
one native call, against the oracle (oracle/region_ref.py), a numpy model and
the box calls with 1-element boxes; only the chunks that hold a point are
opened."""
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
from test_gpu_write_boxes import check_store_equals, chunk_files, copy_store, snapshot, truncate  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Raw, SliceDataChunk  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.region import BoundingBox, read_ndarray, read_ndarrays_v, read_points, write_points  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, CS, GRID = [10, 9, 14], [4, 3, 5], [3, 3, 3]  # edge chunks overhang along dimensions 0 and 2
ABSENT = (1, 1, 1)
FILL = 7
CODECS = {"gzip": Gzip(6), "raw": Raw()}


def make_store(root, codec, order="C"):
    meta = ArrayMetadata.new(SHAPE, CS, "<i4", CODECS[codec])
    meta.chunk_memory_layout = order
    meta.fill_value = FILL
    h = FilesystemHierarchy.open_or_create(str(root))
    h.create_array("a", meta)
    rng = np.random.default_rng(31)
    chunks = {c: rng.integers(100, 100000, int(np.prod(CS))).astype(np.int32)
              for c in itertools.product(*[range(g) for g in GRID]) if c != ABSENT}
    h.write_chunks("a", meta, [SliceDataChunk(list(c), d) for c, d in chunks.items()])
    return h, meta, chunks


def draw(rng, P, hi=(12, 10, 16)):
    """Points over the array, the edge chunks' overhang (indices 10, 11 along
    dimension 0 and 14 along dimension 2) and the first index past the grid
    along dimensions 1 and 2 (9 and 15: no chunk)."""
    return np.stack([rng.integers(0, h, P) for h in hi], axis=1).astype(np.uint64)


def oracle_read(meta, chunks, pts):
    hull = region_ref.read_ndarray(SHAPE, CS, meta.chunk_memory_layout, [0, 0, 0], [12, 10, 16], chunks.get, np.int32,
                                   FILL)
    return hull[tuple(pts[:, d].astype(np.int64) for d in range(3))]


def chunk_of(c):
    return tuple(int(x) // k for x, k in zip(c, CS))


@pytest.mark.parametrize("codec,order", [("gzip", "C"), ("raw", "F")])
def test_read_points_vs_oracle_and_one_element_boxes(tmp_path, codec, order):
    """300 points, duplicates among them, over 26 present chunks and the absent
    one: read_points equals the oracle's read of the hull indexed at the points
    and read_ndarrays_v with 1-element boxes (for the points such a box may be
    built for), as a host array and as a device tensor, in the tuple-of-arrays
    form too; a slot budget of one chunk (27 groups) gives the same bytes."""
    h, meta, chunks = make_store(tmp_path, codec, order)
    rng = np.random.default_rng(8)
    pts = draw(rng, 300)
    pts[7] = pts[3]
    pts[11] = [5, 4, 6]  # the absent chunk
    assert chunk_of(pts[11]) == ABSENT and len({chunk_of(c) for c in pts}) >= 27
    want = oracle_read(meta, chunks, pts)
    assert (want == FILL).sum() >= 1 and len(set(want.tolist())) > 100
    D = int(np.prod(CS)) * 4
    for budget in (0, D):
        got = read_points(h, "a", meta, pts, np.int32, slot_budget_bytes=budget)
        assert got.shape == (300,) and got.dtype == np.int32
        assert np.array_equal(got, want), budget
        t = read_points(h, "a", meta, pts, np.int32, as_tensor=True, slot_budget_bytes=budget)
        assert np.array_equal(t.cpu().numpy().view(np.int32), want), budget
    got = read_points(h, "a", meta, tuple(pts[:, d].astype(np.int64) for d in range(3)), np.int32)
    assert np.array_equal(got, want)
    boxes = read_ndarrays_v(h, "a", meta, [BoundingBox(list(map(int, c)), [1, 1, 1]) for c in pts], np.int32)
    assert np.array_equal(np.array([b.reshape(-1)[0] for b in boxes], np.int32), want)
    assert read_points(h, "a", meta, np.zeros((0, 3), np.uint64), np.int32).shape == (0,)


@pytest.mark.parametrize("codec", ["gzip", "raw"])
def test_only_touched_chunk_files_are_opened_and_a_corrupt_one_is_named(tmp_path, codec):
    h, meta, chunks = make_store(tmp_path, codec)
    rng = np.random.default_rng(5)
    pts = np.array([c for c in draw(rng, 200) if chunk_of(c) not in ((2, 0, 1), (0, 2, 2))], np.uint64)
    for c in ((2, 0, 1), (0, 2, 2)):  # untouched: no stream of any codec, and short for raw
        with open(h.chunk_path("a", meta, list(c)), "wb") as f:
            f.write(b"\xff" * 37)
    want = oracle_read(meta, chunks, pts)
    assert np.array_equal(read_points(h, "a", meta, pts, np.int32), want)
    assert np.array_equal(read_points(h, "a", meta, pts, np.int32, slot_budget_bytes=1), want)
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [2, 0, 1], np.int32)
    bad = np.concatenate([pts, np.array([[9, 1, 7]], np.uint64)])
    assert chunk_of(bad[-1]) == (2, 0, 1)
    for kw in ({}, {"as_tensor": True}):
        with pytest.raises(ZarrIOError) as ei:
            read_points(h, "a", meta, bad, np.int32, **kw)
        assert ei.value.kind == single.value.kind and "chunk [2, 0, 1]" in str(ei.value)


def test_a_point_in_a_chunk_outside_the_grid_is_invalid_input(tmp_path):
    """Index 13 along dimension 0 lies in chunk 3 of a grid of 3, where the
    reference panics (storage.rs:217) and the box calls refuse the 1-element
    box: InvalidInput before any file is touched, the point named.  Index 12,
    a chunk boundary, visits no chunk: filled, and dropped by a write."""
    h, meta, chunks = make_store(tmp_path, "gzip")
    truncate(h.chunk_path("a", meta, [0, 0, 0]))  # a read would fail with another status
    before = snapshot(tmp_path)
    pts = np.array([[1, 1, 1], [13, 0, 0]], np.uint64)
    with pytest.raises(ZarrIOError) as ei:
        read_points(h, "a", meta, pts, np.int32)
    assert ei.value.kind == "InvalidInput" and "point 1" in str(ei.value) and "chunk [3, 0, 0]" in str(ei.value)
    with pytest.raises(ZarrIOError) as ei:
        write_points(h, "a", meta, pts, np.array([1, 2], np.int32))
    assert ei.value.kind == "InvalidInput" and "point 1" in str(ei.value)
    with pytest.raises(ZarrIOError) as eb:
        read_ndarrays_v(h, "a", meta, [BoundingBox([13, 0, 0], [1, 1, 1])], np.int32)
    assert eb.value.kind == "InvalidInput"
    assert read_points(h, "a", meta, [[12, 0, 0]], np.int32).tolist() == [FILL]
    write_points(h, "a", meta, [[12, 0, 0]], np.array([5], np.int32))
    assert snapshot(tmp_path) == before


def model_write(meta, chunks, pts, vals):
    """a[coords] = values in order on the array over its nominal grid (absent
    chunks as fill value) -> coord -> flat chunk, for the touched chunks."""
    order = meta.chunk_memory_layout
    full = np.full([g * k for g, k in zip(GRID, CS)], FILL, np.int32)
    sl = lambda c: tuple(slice(g * k, (g + 1) * k) for g, k in zip(c, CS))  # noqa: E731
    for c, d in chunks.items():
        full[sl(c)] = d.reshape(CS, order=order)
    touched = set()
    for c, v in zip(pts, vals):
        full[tuple(int(x) for x in c)] = v
        touched.add(chunk_of(c))
    return full, {c: full[sl(c)].flatten(order=order) for c in touched}


@pytest.mark.parametrize("codec,order", [("gzip", "C"), ("raw", "F")])
def test_write_points_equals_the_numpy_model_in_order(tmp_path, codec, order):
    """250 points with many duplicates (the later value wins), the overhang and
    the absent chunk among them, chunk (2, 0, 1) and two more untouched:
    afterwards the chunk files are the old key set plus the absent chunk, every
    one decodes to the model, the full read_ndarray equals the model, and the
    untouched files keep their bytes and mtime.  A budget of one chunk and the
    device form leave byte-identical stores."""
    h, meta, chunks = make_store(tmp_path / "a", codec, order)
    rng = np.random.default_rng(21)
    skip = ((2, 0, 1), (0, 2, 2), (1, 0, 0))
    pts = np.array([c for c in draw(rng, 400, hi=(12, 9, 15)) if chunk_of(c) not in skip][:250], np.uint64)
    pts[100:140] = pts[20:60]  # duplicates, far apart in the list
    pts[249] = pts[0]
    pts[60] = [5, 4, 6]  # the absent chunk starts as fill value
    vals = rng.integers(-50000, -1, 250).astype(np.int32)
    full, touched = model_write(meta, chunks, pts, vals)
    assert ABSENT in touched and not set(skip) & set(touched)
    want = {**chunks, **touched}
    h2 = copy_store(tmp_path / "a", tmp_path / "b")
    h3 = copy_store(tmp_path / "a", tmp_path / "c")
    quiet = {c: os.stat(h.chunk_path("a", meta, list(c))).st_mtime_ns for c in skip}
    old = chunk_files(tmp_path / "a")
    write_points(h, "a", meta, pts, vals)
    check_store_equals(h, tmp_path / "a", meta, np.int32, want)
    got = read_ndarray(h, "a", meta, BoundingBox([0, 0, 0], SHAPE), np.int32)
    assert np.array_equal(got, full[:SHAPE[0], :SHAPE[1], :SHAPE[2]])
    new = chunk_files(tmp_path / "a")
    for c in skip:
        p = h.chunk_path("a", meta, list(c))
        rel = os.path.relpath(p, str(tmp_path / "a"))
        assert os.stat(p).st_mtime_ns == quiet[c] and new[rel] == old[rel]
    assert np.array_equal(read_points(h, "a", meta, pts, np.int32), full[tuple(pts[:, d].astype(np.int64) for d in range(3))])
    # several groups; the device form
    import torch
    write_points(h2, "a", meta, pts, vals, slot_budget_bytes=1)
    assert chunk_files(tmp_path / "b") == new
    write_points(h3, "a", meta, tuple(pts[:, d] for d in range(3)), torch.from_numpy(vals).cuda())
    assert chunk_files(tmp_path / "c") == new
    write_points(h3, "a", meta, np.zeros((0, 3), np.uint64), np.zeros(0, np.int32))
    assert chunk_files(tmp_path / "c") == new


def test_a_corrupt_touched_chunk_stops_the_write_before_any_file_changes(tmp_path):
    h, meta, chunks = make_store(tmp_path, "gzip")
    truncate(h.chunk_path("a", meta, [1, 2, 0]))
    with pytest.raises(ZarrIOError) as single:
        h.read_chunk("a", meta, [1, 2, 0], np.int32)
    before = snapshot(tmp_path)
    pts = np.array([[0, 0, 0], [5, 7, 2], [9, 8, 13]], np.uint64)
    with pytest.raises(ZarrIOError) as ei:
        write_points(h, "a", meta, pts, np.array([1, 2, 3], np.int32))
    assert ei.value.kind == single.value.kind and "chunk [1, 2, 0]" in str(ei.value)
    assert snapshot(tmp_path) == before  # one group: reads precede writes


def test_a_chunk_of_one_element_is_not_read_before_it_is_written(tmp_path):
    meta = ArrayMetadata.new([4, 3], [1, 1], "<i2", Gzip(6))
    h = FilesystemHierarchy.open_or_create(str(tmp_path))
    h.create_array("a", meta)
    h.write_chunks("a", meta, [SliceDataChunk([i, j], np.array([10 * i + j], np.int16)) for i in range(4) for j in range(3)])
    truncate(h.chunk_path("a", meta, [2, 1]))  # corrupt, and covered by its point
    write_points(h, "a", meta, [[2, 1], [0, 0], [2, 1]], np.array([-1, -2, -3], np.int16))
    got = read_ndarray(h, "a", meta, BoundingBox([0, 0], [4, 3]), np.int16)
    want = np.array([[10 * i + j for j in range(3)] for i in range(4)], np.int16)
    want[2, 1], want[0, 0] = -3, -2
    assert np.array_equal(got, want)


def test_plain_c_caller_reads_seven_points(tmp_path):
    """tests/c_abi_p/points_c.c, built by its own Makefile, reads seven elements
    of the zarrita fixture with one zcg_store_read_points call."""
    c_abi = os.path.join(ROOT, "tests", "c_abi_p")
    r = subprocess.run(["make", "-s", "-C", c_abi], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(c_abi, "points_c")
    store = os.path.join(ROOT, "tests", "golden", "zarrita")
    outf = str(tmp_path / "points.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "points_c: ok (7 points, grid range 8 chunks, 6 kept, keep[2] = 0)" in r.stdout, r.stdout
    got = np.fromfile(outf, "<i2")
    chunks = {g: v for g, _, v in zarrita_chunks()}
    pts = [[0, 0, 0], [3, 4, 5], [1, 2, 3], [2, 3, 4], [1, 2, 3], [0, 6, 1], [3, 0, 2]]
    want = [region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", c, [1, 1, 1], chunks.get, np.int16, 0).reshape(-1)[0]
            for c in pts]
    assert got.tolist() == [int(x) for x in want]
