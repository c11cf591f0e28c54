"""The host-only parts of the strided box calls: zcg_region_s_chunks and
zcg_regions_s_grid against a brute-force enumeration of the sample indices,
zcg_sbox's layout, and the argument errors of read_ndarrays_s.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, ZarrIOError, _native
from zarr_amd.region import (BoundingBox, read_ndarrays_s, region_grid, region_s_chunks, regions_s_grid,
                             regions_v_grid)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def meta_for(shape, cs):
    return ArrayMetadata.new(shape, cs, "<u2")


def hull_of(shape, step):
    return [(s - 1) * k + 1 if s else 0 for s, k in zip(shape, step)]


def chunks_ref(meta, offset, shape, step):
    """The definition, sample by sample: the hull's grid range; per dimension
    the grid indices inside that range whose nominal bounds hold a sample; the
    product of their numbers, 0 when the hull misses the array."""
    lo, n = region_grid(meta, BoundingBox(offset, hull_of(shape, step)))
    touched = []
    for d in range(len(offset)):
        idx = offset[d] + np.arange(shape[d], dtype=object) * step[d]
        cells = {int(i) // meta.chunk_shape[d] for i in idx}
        touched.append([1 if lo[d] + j in cells else 0 for j in range(n[d])])
    count = 0 if 0 in n else int(np.prod([sum(t) for t in touched], dtype=object))
    return lo, n, touched, count


def check_box(meta, offset, shape, step):
    want = chunks_ref(meta, offset, shape, step)
    got = region_s_chunks(meta, offset, shape, step)
    assert (got[0], got[1], got[2], got[3]) == want, (offset, shape, step)
    lo, n, touched, count = region_s_chunks(meta, offset, shape, step, want_touched=False)  # touched = NULL
    assert touched is None and (lo, n, count) == (want[0], want[1], want[3])
    return want


@pytest.mark.parametrize("seed", range(60))
def test_s_chunks_and_s_grid_equal_the_enumeration_of_samples(seed):
    """1-4 dimensions, 0-12 boxes with 0-9 samples per dimension, steps from 1
    to beyond the array, offsets partly beyond the array: every box against the
    enumeration, and the union of the hulls' ranges."""
    rng = np.random.default_rng(9300 + seed)
    nd = 1 + seed % 4
    B = [0, 1, 3, 12][(seed // 4) % 4]
    shape = [int(rng.integers(1, 80)) for _ in range(nd)]
    cs = [int(rng.integers(1, 9)) for _ in range(nd)]
    meta = meta_for(shape, cs)
    offsets = [[int(rng.integers(0, s + 8)) for s in shape] for _ in range(B)]
    shapes = [[int(rng.integers(0, 10)) for _ in range(nd)] for _ in range(B)]
    steps = [[int(rng.choice([1, 2, 3, c, c + 1, 2 * c + 1, int(rng.integers(1, 100))])) for c in cs]
             for _ in range(B)]
    ulo, uhi = None, None
    for off, shp, stp in zip(offsets, shapes, steps):
        blo, bn, _, _ = check_box(meta, off, shp, stp)
        if 0 in bn:
            continue
        bhi = [a + k for a, k in zip(blo, bn)]
        ulo = blo if ulo is None else [min(a, b) for a, b in zip(ulo, blo)]
        uhi = bhi if uhi is None else [max(a, b) for a, b in zip(uhi, bhi)]
    lo, n = regions_s_grid(meta, offsets, shapes, steps)
    if ulo is None:
        assert (lo, n) == ([0] * nd, [0] * nd)
    else:
        assert (lo, n) == (ulo, [h - a for a, h in zip(ulo, uhi)])


def test_s_chunks_fixed_cases():
    meta = meta_for([100, 64], [8, 16])
    # step 1: touched is the whole range
    lo, n, touched, count = check_box(meta, [5, 3], [40, 50], [1, 1])
    assert touched == [[1] * n[0], [1] * n[1]] and count == n[0] * n[1] == 6 * 4
    # a step of the chunk extent: one sample per chunk, every chunk of the range
    lo, n, touched, count = check_box(meta, [5, 3], [6, 3], [8, 16])
    assert touched == [[1] * 6, [1] * 3] and count == 18
    # the chunk extent plus 1, from a chunk's last element: samples 7, 16, 25, 34 -> chunks 0, 2, 3, 4
    lo, n, touched, count = check_box(meta, [7, 0], [4, 1], [9, 1])
    assert (lo[0], n[0], touched[0], count) == (0, 5, [1, 0, 1, 1, 1], 4)
    # a step larger than the array: the second sample lies outside, the range is clipped to the array
    lo, n, touched, count = check_box(meta, [2, 1], [3, 2], [500, 70])
    assert (lo, n, touched, count) == ([0, 0], [13, 4], [[1] + [0] * 12, [1, 0, 0, 0]], 1)
    # partly outside: the overhanging edge chunk 12 (elements 96 .. 103) holds the sample at 102
    lo, n, touched, count = check_box(meta, [90, 60], [5, 2], [3, 3])
    assert (lo, n, touched, count) == ([11, 3], [2, 1], [[1, 1], [1]], 2)
    # wholly outside: no chunk, whatever the other dimension is
    assert check_box(meta, [104, 0], [3, 3], [2, 2])[3] == 0
    # zero sample counts
    lo, n, touched, count = check_box(meta, [5, 3], [0, 4], [2, 2])
    assert sum(touched[0]) == 0 and count == 0
    assert regions_s_grid(meta, [[5, 3]], [[0, 4]], [[2, 2]]) == regions_v_grid(meta, [[5, 3]], [[0, 7]])
    # a step of 0 is refused by the read calls: no range, no chunk, and nothing added to a union
    assert region_s_chunks(meta, [5, 3], [4, 4], [0, 2]) == ([0, 0], [0, 0], [[], []], 0)
    assert regions_s_grid(meta, [[5, 3], [40, 20]], [[4, 4], [2, 2]], [[0, 2], [3, 3]]) == ([5, 1], [1, 1])


def test_s_chunks_of_a_huge_step_and_a_huge_array_need_no_long_loop():
    """Counts come in closed form: 2^40 chunks in a range with touched = NULL,
    and steps next to 2^63, return at once."""
    meta = meta_for([1 << 44, 1 << 62], [16, 1 << 20])
    lo, n, touched, count = region_s_chunks(meta, [3, 5], [1 << 30, 2], [1 << 10, 1 << 61], want_touched=False)
    assert (lo, n) == ([0, 0], [((3 + ((1 << 30) - 1) * (1 << 10)) >> 4) + 1, ((5 + (1 << 61)) >> 20) + 1])
    assert count == (1 << 30) * 2
    lo, n, touched, count = region_s_chunks(meta, [0, 0], [1 << 41, 1], [1, 1], want_touched=False)
    assert (n, count) == ([1 << 37, 1], 1 << 37)


@pytest.mark.parametrize("seed", range(10))
def test_s_grid_with_all_steps_one_equals_v_grid(seed):
    rng = np.random.default_rng(700 + seed)
    nd = 1 + seed % 4
    shape = [int(rng.integers(1, 60)) for _ in range(nd)]
    cs = [int(rng.integers(1, 9)) for _ in range(nd)]
    meta = meta_for(shape, cs)
    B = 1 + 3 * seed
    offsets = [[int(rng.integers(0, s + 8)) for s in shape] for _ in range(B)]
    shapes = [[int(rng.integers(0, 13)) for _ in range(nd)] for _ in range(B)]
    assert regions_s_grid(meta, offsets, shapes, [[1] * nd] * B) == regions_v_grid(meta, offsets, shapes)


def test_scratch_bytes_are_monotonic_and_non_zero():
    L = _native.load_library()
    sizes = [L.zcg_regions_s_scratch_bytes(n) for n in (0, 1, 2, 63, 64, 65, 1025, 1 << 20, (1 << 32) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s > 0 for s in sizes[1:])
    assert sizes[-1] >= 8 * (1 << 32)  # a prefix word per box


def test_sbox_layout_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zchunk_gpu.h"
int main(void){printf("%zu %zu %zu %zu %zu\n", sizeof(zcg_sbox), offsetof(zcg_sbox, shape),
 offsetof(zcg_sbox, step), offsetof(zcg_sbox, strides), offsetof(zcg_sbox, base));return 0;}
'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    S = _native.SBox
    assert [int(x) for x in out] == [ctypes.sizeof(S), S.shape.offset, S.step.offset, S.strides.offset,
                                     S.base.offset]


def test_read_ndarrays_s_argument_errors_need_no_gpu():
    """A step of 0, a steps array of the wrong shape, a box of the wrong rank
    and a wrong element type are refused before any native call."""
    meta = meta_for([10, 10], [4, 4])
    boxes = [BoundingBox([0, 0], [2, 2]), BoundingBox([1, 1], [3, 2]), BoundingBox([2, 2], [1, 1])]

    def refused(kind, bxs, steps, t=np.uint16):
        with pytest.raises(ZarrIOError) as e:
            read_ndarrays_s(None, "a", meta, bxs, steps, t)
        assert e.value.kind == kind, e.value

    refused("InvalidInput", boxes, [2, 0])
    refused("InvalidInput", boxes, [[1, 1], [1, 0], [1, 1]])
    refused("InvalidInput", boxes, [1, 1, 1])
    refused("InvalidInput", boxes, [[1, 1], [1, 1]])
    refused("InvalidInput", boxes, 3)
    refused("InvalidInput", boxes, [[1.5, "x"]] * 3)
    refused("InvalidData", [BoundingBox([0], [2])], [1, 1])
    with pytest.raises(ZarrIOError):
        read_ndarrays_s(None, "a", meta, boxes, [1, 1], np.float32)


def test_store_and_device_calls_refuse_missing_arguments_without_a_gpu():
    L = _native.load_library()
    st, am, msg = _native.array_meta_from_json(meta_for([10, 10], [4, 4]).to_json())
    assert st == _native.OK, msg
    keep = ((ctypes.c_uint64 * 2)(2, 2), (ctypes.c_uint64 * 2)(1, 1), (ctypes.c_uint64 * 2)(0, 0),
            (ctypes.c_void_p * 1)(0))
    shp, stp, off, buf = [ctypes.addressof(k) for k in keep]
    m = ctypes.byref(am)
    bad = _native.INVALID_INPUT
    assert L.zcg_store_read_boxes_s(None, m, b"/r", b"a", shp, stp, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_read_boxes_s_device(None, m, b"/r", b"a", shp, stp, None, 1, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_read_boxes_s(None, None, None, b"a", shp, stp, off, buf, 1, 0, 1) == bad
    assert L.zcg_read_regions_s(None, None, None, None, None, None, 0, None, None, None) == bad
    assert L.zcg_read_regions_s(None, None, None, None, None, None, 3, None, None, None) == bad
