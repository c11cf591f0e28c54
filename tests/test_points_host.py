"""The host-only parts of the point calls: zcg_points_grid against
zcg_regions_v_grid with shapes of 1, zcg_points_last against a dict, the
header and the exports, and the argument handling of the Python layer.  No
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, ZarrIOError, _native
from zarr_amd.region import _coords_arg, points_grid, points_last, read_points, regions_v_grid, write_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = (1 << 64) - 1
NEW_SYMBOLS = ("zcg_points_grid", "zcg_points_last", "zcg_read_points", "zcg_write_points",
               "zcg_store_read_points_device", "zcg_store_read_points",
               "zcg_store_write_points_device", "zcg_store_write_points")


def meta_for(shape, cs):
    return ArrayMetadata.new(shape, cs, "<u2")


def grid_both(meta, coords):
    nd = meta.get_ndim()
    c = np.array(coords, dtype=np.uint64).reshape(-1, nd)
    return points_grid(meta, c), regions_v_grid(meta, c, np.ones_like(c))


def random_points(rng, shape, cs, P):
    """Interior points, the array's last index, the first index beyond it (an
    edge chunk's overhang where the extent is no multiple of the chunk's), points
    beyond the grid, and 2^64-1."""
    nd = len(shape)
    pts = []
    for _ in range(P):
        kind = int(rng.integers(0, 6))
        p = []
        for d in range(nd):
            edge = -(-shape[d] // cs[d]) * cs[d]  # the grid's nominal end
            p.append([int(rng.integers(0, shape[d])), shape[d] - 1, shape[d], int(rng.integers(edge, edge + 3 * cs[d] + 2)),
                      U64_MAX, int(rng.integers(0, shape[d]))][kind if rng.integers(0, 3) else 0])
        pts.append(p)
    return pts


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
@pytest.mark.parametrize("seed", range(8))
def test_points_grid_equals_v_grid_with_shapes_of_one(nd, seed):
    rng = np.random.default_rng(4100 + 17 * nd + seed)
    shape = [int(rng.integers(1, 50)) for _ in range(nd)]
    cs = [int(rng.choice([1, 2, 5, 7, int(rng.integers(1, 12))])) for _ in range(nd)]
    meta = meta_for(shape, cs)
    P = [1, 2, 9, 40][seed % 4]
    got, want = grid_both(meta, random_points(rng, shape, cs, P))
    assert got == want


def test_points_grid_fixed_cases():
    meta = meta_for([10, 9], [4, 3])
    # the last index, and the overhang of the edge chunk along dim 0 (elements 8 .. 11)
    assert grid_both(meta, [[9, 8]]) == (([2, 2], [1, 1]),) * 2
    assert grid_both(meta, [[10, 0], [11, 8]]) == (([2, 0], [1, 3]),) * 2
    # interior points far apart: the bounding range
    assert grid_both(meta, [[0, 8], [9, 0]]) == (([0, 0], [3, 3]),) * 2
    # no point visits a chunk: beyond the grid at a multiple of the chunk extent, 9 = 3 * 3 along dim 1
    assert grid_both(meta, [[12, 0], [0, 9], [400, 300]]) == (([0, 0], [0, 0]),) * 2
    L = _native.load_library()
    r = _native.Region()
    r.ndim, r.elem_size = 2, 2
    for d, (a, c) in enumerate(zip([10, 9], [4, 3])):
        r.array_shape[d], r.chunk_shape[d] = a, c
    lo, n = (ctypes.c_uint64 * 8)(7, 7), (ctypes.c_uint64 * 8)(7, 7)
    c = np.array([[12, 0], [0, 9]], np.uint64)
    assert L.zcg_points_grid(ctypes.byref(r), c.ctypes.data, 2, ctypes.addressof(lo), ctypes.addressof(n)) == 0
    assert list(lo[:2]) == [0, 0] and list(n[:2]) == [0, 0]
    # n_points = 0, with and without a coordinate array
    lo, n = (ctypes.c_uint64 * 8)(7, 7), (ctypes.c_uint64 * 8)(7, 7)
    assert L.zcg_points_grid(ctypes.byref(r), c.ctypes.data, 0, ctypes.addressof(lo), ctypes.addressof(n)) == 0
    assert list(lo[:2]) == [0, 0] and list(n[:2]) == [0, 0]
    assert L.zcg_points_grid(ctypes.byref(r), None, 0, ctypes.addressof(lo), ctypes.addressof(n)) == 0
    assert points_grid(meta, np.zeros((0, 2), np.uint64)) == ([0, 0], [0, 0])
    # 2^64-1 with in-grid points beside it, and alone
    for pts in ([[U64_MAX, 2]], [[3, 3], [U64_MAX, U64_MAX]], [[U64_MAX, U64_MAX]]):
        got, want = grid_both(meta, pts)
        assert got == want
    meta1 = meta_for([10, 9], [1, 1])  # a chunk extent of 1: 2^64-1 is a multiple of it and visits nothing
    assert grid_both(meta1, [[U64_MAX, 2], [4, 5]]) == (([4, 5], [1, 1]),) * 2


def last_model(coords):
    last = {}
    for i, c in enumerate(coords):
        last[tuple(int(x) for x in c)] = i
    keep = np.zeros(len(coords), bool)
    keep[list(last.values())] = True
    return keep


@pytest.mark.parametrize("nd", [1, 2, 8])
def test_points_last_equals_a_dict(nd):
    rng = np.random.default_rng(77 + nd)
    for P, span in ((1, 5), (50, 1000), (200, 3), (1000, 4)):
        c = rng.integers(0, span, size=(P, nd)).astype(np.uint64)
        c[rng.integers(0, P)] = U64_MAX
        assert np.array_equal(points_last(c), last_model(c)), (P, span)


def test_points_last_fixed_cases():
    c = np.arange(12, dtype=np.uint64).reshape(6, 2)
    assert points_last(c).all()  # no duplicates
    same = np.tile(np.array([[3, 4]], np.uint64), (7, 1))
    assert list(points_last(same)) == [False] * 6 + [True]  # all duplicates: the last one
    c[5] = c[0]  # a pair that is first and last
    assert list(points_last(c)) == [False, True, True, True, True, True]
    # dimensions that differ only in one place are different points
    assert points_last(np.array([[1, 2], [2, 1], [1, 2 + (1 << 32)]], np.uint64)).all()
    L = _native.load_library()
    keep = np.full(4, 9, np.uint8)
    assert L.zcg_points_last(c.ctypes.data, 0, 2, keep.ctypes.data) == 0 and (keep == 9).all()
    assert L.zcg_points_last(c.ctypes.data, 6, 2, None) == 0  # NULL keep
    assert L.zcg_points_last(c.ctypes.data, 6, 0, keep.ctypes.data) == 0
    assert L.zcg_points_last(c.ctypes.data, 6, 9, keep.ctypes.data) == 0
    keep6 = np.zeros(6, np.uint8)
    assert L.zcg_points_last(c.ctypes.data, 6, 2, keep6.ctypes.data) == 5
    assert points_last(np.zeros((0, 3), np.uint64)).shape == (0,)


def test_points_last_is_not_quadratic():
    """2^18 points, all equal and all different: a pairwise compare would take minutes."""
    P = 1 << 18
    assert points_last(np.zeros((P, 3), np.uint64)).sum() == 1
    assert points_last(np.arange(3 * P, dtype=np.uint64).reshape(P, 3)).all()


def test_new_names_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zchunk_gpu.h")).read()
    L = _native.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    for cite in ("ndarray.rs:153-268", "ndarray.rs:276-385", "ndarray.rs:410-432", "ndarray.rs:434-446"):
        assert cite in header[header.index("many single elements by coordinate"):header.index("zcg_read_points(")]
    assert L.zcg_abi_version() == 1  # symbols were added, nothing else changed


def test_calls_refuse_missing_arguments_without_a_gpu():
    L = _native.load_library()
    st, am, msg = _native.array_meta_from_json(meta_for([10, 10], [4, 4]).to_json())
    assert st == _native.OK, msg
    c = np.array([[1, 2]], np.uint64)
    buf = np.zeros(1, np.uint16)
    m, bad = ctypes.byref(am), _native.INVALID_INPUT
    assert L.zcg_store_read_points(None, m, b"/r", b"a", c.ctypes.data, 1, buf.ctypes.data, 0, 1) == bad
    assert L.zcg_store_read_points_device(None, m, b"/r", b"a", c.ctypes.data, 1, 1, buf.ctypes.data, 0, 1) == bad
    assert L.zcg_store_write_points(None, m, b"/r", b"a", c.ctypes.data, 1, buf.ctypes.data, 0, 1) == bad
    assert L.zcg_store_write_points_device(None, None, b"/r", b"a", c.ctypes.data, 1, buf.ctypes.data, 0, 1) == bad
    assert L.zcg_read_points(None, None, None, None, None, None, 0, None, None, None) == bad
    assert L.zcg_write_points(None, None, None, None, None, None, 3, None, None, None) == bad


def test_python_coordinate_forms():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 100, size=(20, 3))
    both = _coords_arg(c, 3), _coords_arg((c[:, 0], c[:, 1], c[:, 2]), 3)
    assert both[0].dtype == np.uint64 and both[0].flags.c_contiguous and np.array_equal(*both)
    assert np.array_equal(both[0], c.astype(np.uint64))
    meta = meta_for([100, 100, 100], [7, 5, 64])
    assert points_grid(meta, c) == points_grid(meta, tuple(c.T))
    assert np.array_equal(points_last(c), points_last(c.astype(np.uint64)))
    big = np.array([[U64_MAX, 1 << 63, 5]], np.uint64)
    assert [int(x) for x in _coords_arg(big, 3)[0]] == [U64_MAX, 1 << 63, 5]
    assert _coords_arg([], 3).shape == (0, 3) and _coords_arg(([], [], []), 3).shape == (0, 3)
    neg = c.copy()
    neg[7, 1] = -1
    for form in (neg, tuple(neg.T), neg.tolist()):
        with pytest.raises(ValueError):
            _coords_arg(form, 3)
        with pytest.raises(ValueError):
            points_grid(meta, form)
        with pytest.raises(ValueError):
            read_points(None, "a", meta, form, np.uint16)
        with pytest.raises(ValueError):
            write_points(None, "a", meta, form, np.zeros(20, np.uint16))
    with pytest.raises(ZarrIOError):
        _coords_arg(c, 2)  # the wrong number of dimensions
    with pytest.raises(ZarrIOError):
        _coords_arg((c[:, 0], c[:, 1]), 3)
    with pytest.raises(TypeError):
        _coords_arg(c.astype(np.float64), 3)
