"""Host side of the batched box reads (no GPU): zcg_box's layout against the
ctypes mirror, and zcg_regions_grid against the union of the oracle's
bounded_coord_iter ranges."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from zarr_amd import _native  # noqa: E402


def test_box_layout_matches_header(tmp_path):
    """sizeof / offsetof of zcg_box from a gcc-compiled probe of the header."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zchunk_gpu.h"
int main(){printf("%zu %zu %zu\n", sizeof(zcg_box), offsetof(zcg_box, offset), offsetof(zcg_box, out));return 0;}
'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_native.Box), _native.Box.offset.offset, _native.Box.out.offset]
    assert ctypes.sizeof(_native.Box) == 8 * _native.MAX_DIMS + 8


def regions_grid(shape, cs, offsets, bshape):
    L = _native.load_library()
    nd = len(shape)
    r = _native.Region()
    r.ndim, r.elem_size = nd, 1
    for d in range(nd):
        r.array_shape[d], r.chunk_shape[d], r.bbox_shape[d] = shape[d], cs[d], bshape[d]
        r.bbox_offset[d] = 12345  # ignored
    offs = np.ascontiguousarray(np.asarray(offsets, np.uint64).reshape(-1, nd))
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*([77] * _native.MAX_DIMS))
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*([77] * _native.MAX_DIMS))
    cnt = L.zcg_regions_grid(ctypes.byref(r), offs.ctypes.data if len(offs) else None, len(offs),
                             ctypes.addressof(lo), ctypes.addressof(n))
    return int(cnt), [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]


def test_regions_grid_is_the_union_of_bounded_coord_iter():
    rng = np.random.default_rng(2024)
    empty = nonempty = beyond = 0
    for case in range(200):
        nd = int(rng.integers(1, 5))
        shape = [int(rng.integers(1, 40)) for _ in range(nd)]
        cs = [int(rng.integers(1, 9)) for _ in range(nd)]
        bshape = [int(rng.integers(0 if case % 7 == 0 else 1, 12)) for _ in range(nd)]
        B = 0 if case % 23 == 0 else int(rng.integers(1, 10))
        # offsets inside, partly outside (up to shape + 3) and wholly outside the array
        offsets = [[int(rng.integers(0, s + 4)) + (50 if rng.random() < 0.1 else 0) for s in shape] for _ in range(B)]
        coords = set()
        for off in offsets:
            cc = region_ref.bounded_coord_iter(shape, cs, off, bshape)
            coords |= set(cc)
            beyond += any(o >= s for o, s in zip(off, shape))
        cnt, lo, n = regions_grid(shape, cs, offsets, bshape)
        if not coords:
            empty += 1
            assert cnt == 0 and lo == [0] * nd and n == [0] * nd, (case, cnt, lo, n)
            continue
        nonempty += 1
        wlo = [min(c[d] for c in coords) for d in range(nd)]
        whi = [max(c[d] for c in coords) + 1 for d in range(nd)]
        assert lo == wlo and n == [h - l for h, l in zip(whi, wlo)], (case, lo, n, wlo, whi)
        assert cnt == int(np.prod(n))
    assert empty >= 5 and nonempty >= 100 and beyond >= 20


def test_regions_grid_single_box_equals_region_grid():
    """One box: the union is zcg_region_grid's own range."""
    from zarr_amd import ArrayMetadata
    from zarr_amd.region import BoundingBox, region_grid
    meta = ArrayMetadata.new([10, 33], [4, 5], "<i2")
    for off, shp in (([3, 7], [5, 9]), ([13, 0], [2, 2]), ([9, 31], [4, 4])):
        lo, n = region_grid(meta, BoundingBox(off, shp))
        cnt, ulo, un = regions_grid(meta.shape, meta.chunk_shape, [off], shp)
        assert cnt == int(np.prod(n))
        if cnt:
            assert (ulo, un) == (lo, n)
