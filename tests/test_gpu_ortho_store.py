"""read_ortho / write_ortho (zcg_store_read_ortho[_device],
zcg_store_write_ortho[_device]): a[np.ix_(...)] and a[np.ix_(...)] = values on
the store of the point tests in one native call, against the oracle's hull
(oracle/region_ref.py) under np.ix_, a numpy model and the point calls on the
expanded product; only the touched chunks are opened."""
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
from test_gpu_points_store import ABSENT, CS, FILL, SHAPE, chunk_of, make_store, model_write, oracle_read  # noqa: E402
from test_gpu_write_boxes import check_store_equals, chunk_files, copy_store, snapshot, truncate  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.region import (_sel_arg, ortho_chunks, read_ortho, read_points, write_ortho,  # noqa: E402
                             write_points)

pytestmark = pytest.mark.gpu

D = int(np.prod(CS)) * 4  # bytes of a decoded chunk


def product(lists):
    return np.array(list(itertools.product(*[[int(x) for x in L] for L in lists])), np.uint64).reshape(-1, len(lists))


def selections():
    """Every form of a selection entry: integer arrays and lists (unsorted,
    duplicates, the overhang of the edge chunks, indices 9 and 15 that visit no
    chunk), slices (a negative step, a step across chunks), a boolean mask, an
    int."""
    mask = np.zeros(9, bool)
    mask[[0, 4, 5, 8]] = True
    return [
        (np.array([9, 2, 11, 2, 5, 10]), [4, 8, 0, 9], [14, 3, 15, 7, 0, 12, 3]),
        (slice(8, None, -3), mask, 6),
        (slice(None), np.array([1], np.uint8), slice(2, 14, 5)),
    ]


@pytest.mark.parametrize("codec,order", [("gzip", "C"), ("raw", "F")])
def test_read_ortho_vs_oracle_hull_and_read_points_on_the_product(tmp_path, codec, order):
    """Three selections, as a host array and as a device tensor, under budgets
    of 0 (one group: every dimension whole), four chunks (the last dimension
    whole, the one before it cut), three chunks (the last dimension cut, the
    others one touched index at a time) and one chunk."""
    h, meta, chunks = make_store(tmp_path, codec, order)
    hull = region_ref.read_ndarray(SHAPE, CS, order, [0, 0, 0], [12, 10, 16], chunks.get, np.int32, FILL)
    for sel in selections():
        lists = _sel_arg(sel, SHAPE)
        counts = [len(L) for L in lists]
        want = hull[np.ix_(*[L.astype(np.int64) for L in lists])]
        pts = product(lists)
        assert np.array_equal(want.reshape(-1), oracle_read(meta, chunks, pts))
        assert np.array_equal(read_points(h, "a", meta, pts, np.int32).reshape(counts), want)
        for budget in (0, 4 * D, 3 * D, D):
            got = read_ortho(h, "a", meta, sel, np.int32, slot_budget_bytes=budget)
            assert got.shape == tuple(counts) and got.dtype == np.int32
            assert np.array_equal(got, want), budget
            t = read_ortho(h, "a", meta, sel, np.int32, as_tensor=True, slot_budget_bytes=budget)
            assert tuple(t.shape) == tuple(counts) and np.array_equal(t.cpu().numpy(), want), budget
    lists = _sel_arg(selections()[0], SHAPE)
    assert ortho_chunks(meta, lists)[3] == 27 and (hull[np.ix_(*[L.astype(np.int64) for L in lists])] == FILL).any()
    assert read_ortho(h, "a", meta, ([1, 2], [], [3]), np.int32).shape == (2, 0, 1)


@pytest.mark.parametrize("codec", ["gzip", "raw"])
def test_only_touched_chunk_files_are_opened_and_a_corrupt_one_is_named(tmp_path, codec):
    h, meta, chunks = make_store(tmp_path, codec)
    for c in ((2, 0, 1), (2, 2, 2)):  # untouched: no stream of any codec, and short for raw
        with open(h.chunk_path("a", meta, list(c)), "wb") as f:
            f.write(b"\xff" * 37)
    sel = ([7, 0, 5, 3], slice(None), [13, 2, 6, 9])  # no row of the chunks (2, *, *)
    lists = _sel_arg(sel, SHAPE)
    want = oracle_read(meta, chunks, product(lists)).reshape(4, 9, 4)
    for budget in (0, D):
        assert np.array_equal(read_ortho(h, "a", meta, sel, np.int32, slot_budget_bytes=budget), want)
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [2, 0, 1], np.int32)
    bad = ([7, 0, 9, 3],) + sel[1:]
    for kw in ({}, {"as_tensor": True}):
        with pytest.raises(ZarrIOError) as ei:
            read_ortho(h, "a", meta, bad, np.int32, **kw)
        assert ei.value.kind == single.value.kind and "chunk [2, 0, 1]" in str(ei.value)


def test_an_index_in_a_chunk_outside_the_grid_is_invalid_input(tmp_path):
    """Index 13 along dimension 0 lies in chunk 3 of a grid of 3: InvalidInput
    before any file is touched, dimension and position named.  Index 12, a
    chunk boundary, visits no chunk: filled, and dropped by a write."""
    h, meta, chunks = make_store(tmp_path, "gzip")
    truncate(h.chunk_path("a", meta, [0, 0, 0]))  # a read would fail with another status
    before = snapshot(tmp_path)
    sel = ([1, 13], [1], [1, 2])
    with pytest.raises(ZarrIOError) as ei:
        read_ortho(h, "a", meta, sel, np.int32)
    assert ei.value.kind == "InvalidInput" and "dimension 0, position 1" in str(ei.value)
    with pytest.raises(ZarrIOError) as ei:
        write_ortho(h, "a", meta, sel, np.zeros((2, 1, 2), np.int32))
    assert ei.value.kind == "InvalidInput" and "dimension 0, position 1" in str(ei.value)
    assert read_ortho(h, "a", meta, ([12], [0], [0, 15]), np.int32).tolist() == [[[FILL, FILL]]]
    write_ortho(h, "a", meta, ([12], [0], [0, 1]), np.array([5, 6], np.int32).reshape(1, 1, 2))
    write_ortho(h, "a", meta, ([1], [], [0, 1]), np.zeros((1, 0, 2), np.int32))
    assert snapshot(tmp_path) == before


@pytest.mark.parametrize("codec,order", [("gzip", "C"), ("raw", "F")])
def test_write_ortho_equals_the_model_and_write_points_on_the_product(tmp_path, codec, order):
    """Lists with duplicates (per list the last occurrence wins), the overhang
    and the absent chunk, the chunks (*, 2, *) untouched: afterwards the chunk
    files are the old key set plus the absent chunk, every one decodes to the
    model, and the untouched files keep their bytes and mtime.  write_points on
    the product in C order, budgets of one and three chunks and the device form
    leave byte-identical stores."""
    import torch
    h, meta, chunks = make_store(tmp_path / "a", codec, order)
    rng = np.random.default_rng(22)
    sel = ([9, 2, 5, 2, 11], [4, 0, 4, 3], [14, 3, 7, 0, 3])
    counts = [5, 4, 5]
    pts = product(sel)
    vals = rng.integers(-50000, -1, counts).astype(np.int32)
    full, touched = model_write(meta, chunks, pts, vals.reshape(-1))
    assert ABSENT in touched and len(touched) == 18 == ortho_chunks(meta, sel)[3]
    want = {**chunks, **touched}
    copies = {k: copy_store(tmp_path / "a", tmp_path / k) for k in "bcde"}
    skip = [c for c in chunks if c[1] == 2]
    quiet = {c: os.stat(h.chunk_path("a", meta, list(c))).st_mtime_ns for c in skip}
    old = chunk_files(tmp_path / "a")
    write_ortho(h, "a", meta, sel, vals)
    check_store_equals(h, tmp_path / "a", meta, np.int32, want)
    new = chunk_files(tmp_path / "a")
    for c in skip:
        p = h.chunk_path("a", meta, list(c))
        rel = os.path.relpath(p, str(tmp_path / "a"))
        assert os.stat(p).st_mtime_ns == quiet[c] and new[rel] == old[rel]
    assert np.array_equal(read_ortho(h, "a", meta, sel, np.int32),
                          full[np.ix_(*[np.array(L, np.int64) for L in sel])])
    write_points(copies["b"], "a", meta, pts, vals.reshape(-1))
    assert chunk_files(tmp_path / "b") == new
    write_ortho(copies["c"], "a", meta, sel, vals, slot_budget_bytes=D)
    assert chunk_files(tmp_path / "c") == new
    write_ortho(copies["d"], "a", meta, sel, vals, slot_budget_bytes=3 * D)
    assert chunk_files(tmp_path / "d") == new
    write_ortho(copies["e"], "a", meta, sel, torch.from_numpy(vals).cuda())
    assert chunk_files(tmp_path / "e") == new


def test_a_covered_chunk_is_not_read_and_a_corrupt_partly_covered_one_stops_the_write(tmp_path):
    h, meta, chunks = make_store(tmp_path, "gzip")
    truncate(h.chunk_path("a", meta, [0, 0, 0]))  # corrupt, and covered by the selection
    sel = ([3, 1, 0, 2], slice(0, 3), slice(4, None, -1))
    vals = np.arange(4 * 3 * 5, dtype=np.int32).reshape(4, 3, 5) - 9000
    write_ortho(h, "a", meta, sel, vals)
    full, touched = model_write(meta, chunks, product(_sel_arg(sel, SHAPE)), vals.reshape(-1))
    assert list(touched) == [(0, 0, 0)]
    check_store_equals(h, tmp_path, meta, np.int32, {**chunks, **touched})
    truncate(h.chunk_path("a", meta, [1, 2, 0]))
    with pytest.raises(ZarrIOError) as single:
        h.read_chunk("a", meta, [1, 2, 0], np.int32)
    before = snapshot(tmp_path)
    with pytest.raises(ZarrIOError) as ei:
        write_ortho(h, "a", meta, ([0, 5, 9], [0, 7], [2]), np.zeros((3, 2, 1), np.int32))
    assert ei.value.kind == single.value.kind and "chunk [1, 2, 0]" in str(ei.value)
    assert snapshot(tmp_path) == before  # one group: reads precede writes


def test_plain_c_caller_reads_an_orthogonal_selection(tmp_path):
    """tests/c_abi_o/ortho_c.c, built by its own Makefile, reads 2 x 3 x 3
    elements of the zarrita fixture with one zcg_store_read_ortho call."""
    c_abi = os.path.join(ROOT, "tests", "c_abi_o")
    r = subprocess.run(["make", "-s", "-C", c_abi], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(c_abi, "ortho_c")
    store = os.path.join(ROOT, "tests", "golden", "zarrita")
    outf = str(tmp_path / "ortho.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "ortho_c: ok (18 elements, 8 touched chunks, scratch 256 bytes)" in r.stdout, r.stdout
    got = np.fromfile(outf, "<i2")
    chunks = {g: v for g, _, v in zarrita_chunks()}
    pts = itertools.product([3, 0], [4, 1, 6], [5, 2, 2])
    want = [region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", list(c), [1, 1, 1], chunks.get, np.int16, 0).reshape(-1)[0]
            for c in pts]
    assert got.tolist() == [int(x) for x in want]
