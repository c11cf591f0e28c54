"""Orthogonal selections, the host side (no GPU): zcg_ortho_chunks against the
brute-force product through zcg_points_grid, zcg_ortho_scratch_bytes, the layout
of zcg_osel against its ctypes mirror, and how zarr_amd.region turns a
selection into index lists."""
import ctypes
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, ZarrIOError, _native
from zarr_amd.region import _sel_arg, ortho_chunks, ortho_scratch_bytes, points_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, CS = [10, 9, 14], [4, 3, 5]

# duplicates, unsorted order, the overhang of the edge chunks (10, 11 along dimension 0; 14 along dimension 2) and
# indices that visit no chunk (12 along dimension 0, 9 along 1, 15 along 2)
SELECTIONS = [
    ([7, 1, 7, 11, 10, 3], [8, 0, 0, 4], [14, 2, 13, 2, 6]),
    ([9, 12, 0], [9, 5, 2], [15, 11, 0, 12]),
    ([5], [7, 7, 7], [3]),
    ([1, 9], [], [0, 5, 10]),            # one empty list
    ([1, 9], [9, 9], [0, 5, 10]),        # one list that visits nothing
    ([12], [9], [15]),
    ([2, 6, 11], [1, 4, 7], [4, 9, 14]),  # every chunk
]


def visits(d, c):
    return c < SHAPE[d] or c % CS[d] != 0


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("sel", SELECTIONS)
def test_ortho_chunks_equals_the_product_through_points_grid(sel, order):
    meta = ArrayMetadata.new(SHAPE, CS, "<u2")
    meta.chunk_memory_layout = order
    lo, n, touched, count = ortho_chunks(meta, sel)
    product = [list(c) for c in itertools.product(*sel)]
    want_lo, want_n = points_grid(meta, np.array(product, np.uint64).reshape(-1, 3)) if product else ([0] * 3, [0] * 3)
    assert (lo, n) == (want_lo, want_n)
    sets = [{c // CS[d] for c in sel[d] if visits(d, c)} for d in range(3)]
    chunks = {tuple(c[d] // CS[d] for d in range(3)) for c in product if all(visits(d, c[d]) for d in range(3))}
    assert count == len(chunks) == int(np.prod([len(s) for s in sets]))
    if count == 0:
        assert lo == [0, 0, 0] and n == [0, 0, 0]
    assert touched == [[1 if lo[d] + j in sets[d] else 0 for j in range(n[d])] for d in range(3)]
    assert ortho_chunks(meta, sel, want_touched=False) == (lo, n, None, count)


def test_ortho_chunks_refuses_bad_arguments_with_zero():
    L = _native.load_library()
    r = _native.Region()
    r.ndim = 0
    assert L.zcg_ortho_chunks(ctypes.byref(r), None, None, None, None, None) == 0
    r.ndim = 2
    assert L.zcg_ortho_chunks(ctypes.byref(r), None, None, None, None, None) == 0
    assert L.zcg_ortho_chunks(None, None, None, None, None, None) == 0


def test_scratch_bytes_grow_with_every_count_and_stay_aligned():
    rng = np.random.default_rng(5)
    for nd in (1, 3, 8):
        counts = [int(x) for x in rng.integers(0, 2000, nd)]
        base = ortho_scratch_bytes(counts)
        assert base % 8 == 0 and base >= 32 * sum(counts)
        for d in range(nd):
            for more in (1, 7, 100000):
                grown = list(counts)
                grown[d] += more
                assert ortho_scratch_bytes(grown) >= base and ortho_scratch_bytes(grown) % 8 == 0
    assert ortho_scratch_bytes([(1 << 32) - 1] * 8) >= 32 * 8 * ((1 << 32) - 1)


def test_osel_layout_matches_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zchunk_gpu.h"
int main(){printf("%zu %zu %zu %zu %zu\n", sizeof(zcg_osel), offsetof(zcg_osel, index), offsetof(zcg_osel, count),
 offsetof(zcg_osel, strides), offsetof(zcg_osel, base));return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    S = _native.OSel
    assert [int(x) for x in out] == [ctypes.sizeof(S), S.index.offset, S.count.offset, S.strides.offset,
                                     S.base.offset]


def test_selection_forms():
    mask = np.zeros(9, bool)
    mask[[1, 4, 8]] = True
    lists = _sel_arg((slice(8, None, -3), mask, 5), SHAPE)
    assert [a.tolist() for a in lists] == [[8, 5, 2], [1, 4, 8], [5]]
    assert all(a.dtype == np.uint64 and a.flags.c_contiguous for a in lists)
    lists = _sel_arg([slice(None), [3, 3, 0], np.array([13, 2], np.int32)], SHAPE)
    assert [a.tolist() for a in lists] == [list(range(10)), [3, 3, 0], [13, 2]]
    lists = _sel_arg((slice(-3, None), slice(2, 2), []), SHAPE)  # numpy's resolution; empty lists
    assert [a.tolist() for a in lists] == [[7, 8, 9], [], []]
    assert _sel_arg((np.uint64(11), 0, 14), SHAPE)[0].tolist() == [11]  # beyond the array: the kernels' business
    with pytest.raises(IndexError):
        _sel_arg((0, np.ones(8, bool), 0), SHAPE)  # a mask of the wrong length
    with pytest.raises(ValueError):
        _sel_arg((0, [1, -1], 0), SHAPE)
    with pytest.raises(ValueError):
        _sel_arg((-1, 0, 0), SHAPE)
    with pytest.raises(TypeError):
        _sel_arg((0, [0.5], 0), SHAPE)
    with pytest.raises(ZarrIOError):
        _sel_arg((0, 0), SHAPE)
