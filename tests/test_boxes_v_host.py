"""The host-only parts of the batched calls for boxes of differing shapes:
zcg_regions_v_grid, zcg_regions_v_waves, zcg_regions_v_scratch_bytes, the
store calls' argument errors that need no GPU, and zcg_vbox's layout.  No
GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, _native
from zarr_amd.region import BoundingBox, region_grid, regions_v_grid, regions_v_waves, regions_waves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = (1 << 64) - 1


def waves_ref(offsets, shapes):
    """The rule as the header states it, quadratic: box 0 is in wave 0; box b
    opens a new wave iff its extent (offset .. offset + shape, ends saturating
    at 2^64-1) shares at least one element in every dimension with a box of
    the current wave.  A box with a zero extent intersects nothing."""
    B = len(offsets)
    if B == 0:
        return 0, []
    nd = len(offsets[0])
    lo = [[int(o) for o in off] for off in offsets]
    hi = [[min(int(o) + int(s), U64_MAX) for o, s in zip(off, shp)] for off, shp in zip(offsets, shapes)]
    wave_of, cur, start = [], 0, 0
    for b in range(B):
        hit = False
        for a in range(start, b):
            if all(max(lo[a][d], lo[b][d]) < min(hi[a][d], hi[b][d]) for d in range(nd)):
                hit = True
                break
        if hit:
            cur += 1
            start = b
        wave_of.append(cur)
    return cur + 1, wave_of


def meta_for(nd, cs, shape=None):
    return ArrayMetadata.new(shape or [1 << 20] * nd, cs, "<u2")


@pytest.mark.parametrize("seed", range(40))
def test_v_grid_is_the_union_of_the_boxes_grids(seed):
    """1-4 dimensions, 0-30 boxes with extents 0-12 at offsets partly beyond
    the array: the range is the union of zcg_region_grid's per box, boxes that
    visit no chunk left out; the count is the product of the extents."""
    rng = np.random.default_rng(4100 + seed)
    nd = 1 + seed % 4
    B = [0, 1, 2, 9, 30][(seed // 4) % 5]
    shape = [int(rng.integers(1, 60)) for _ in range(nd)]
    cs = [int(rng.integers(1, 9)) for _ in range(nd)]
    meta = meta_for(nd, cs, shape)
    offsets = [[int(rng.integers(0, s + 8)) for s in shape] for _ in range(B)]
    shapes = [[int(rng.integers(0, 13)) for _ in range(nd)] for _ in range(B)]
    lo, n = regions_v_grid(meta, offsets, shapes)
    ulo, uhi = None, None
    for off, shp in zip(offsets, shapes):
        blo, bn = region_grid(meta, BoundingBox(off, shp))
        if 0 in bn:
            continue
        bhi = [a + k for a, k in zip(blo, bn)]
        ulo = blo if ulo is None else [min(a, b) for a, b in zip(ulo, blo)]
        uhi = bhi if uhi is None else [max(a, b) for a, b in zip(uhi, bhi)]
    if ulo is None:
        assert (lo, n) == ([0] * nd, [0] * nd)
    else:
        assert (lo, n) == (ulo, [h - a for a, h in zip(ulo, uhi)])


@pytest.mark.parametrize("seed", range(40))
def test_v_waves_equal_the_brute_force_rule(seed):
    """1-4 dimensions, B in {0, 1, 2, 50, 400}, per-box extents 0-9 (zero
    extents in about one box in eight), one box in sixteen several times the
    others' size, offsets in a small window so that boxes overlap, touch and
    repeat, or next to 2^64 so that the ends saturate."""
    rng = np.random.default_rng(8800 + seed)
    nd = 1 + seed % 4
    B = [0, 1, 2, 50, 400][(seed // 4) % 5]
    cs = [int(rng.integers(1, 10)) for _ in range(nd)]
    shapes = []
    for b in range(B):
        big = 5 if b % 16 == 3 else 1
        shp = [int(rng.integers(1, 10)) * big for _ in range(nd)]
        if rng.random() < 0.125:
            shp[int(rng.integers(0, nd))] = 0
        shapes.append(shp)
    win = [int(5 * max(2, round((B or 1) ** (1.0 / nd)) * (1 + seed % 3))) + 1 for _ in range(nd)]
    base = [U64_MAX - w // 2 if seed % 5 == 4 else int(rng.integers(0, 1000)) for w in win]
    offsets = [[min(U64_MAX, b + int(rng.integers(0, w))) for b, w in zip(base, win)] for _ in range(B)]
    for k in range(1, B, 7):  # duplicates, and boxes that only touch an earlier one
        j = int(rng.integers(0, k))
        offsets[k] = list(offsets[j])
        if k % 2 == 0:
            d = int(rng.integers(0, nd))
            offsets[k][d] = min(U64_MAX, offsets[j][d] + shapes[j][d])
    n, wave_of = regions_v_waves(meta_for(nd, cs), offsets, shapes)
    assert (n, wave_of) == waves_ref(offsets, shapes)
    assert all(a <= b for a, b in zip(wave_of, wave_of[1:]))


@pytest.mark.parametrize("seed", range(12))
def test_v_waves_with_one_shape_repeated_equal_regions_waves(seed):
    rng = np.random.default_rng(600 + seed)
    nd = 1 + seed % 3
    shape = [int(rng.integers(0 if seed % 5 == 4 else 1, 9)) for _ in range(nd)]
    cs = [int(rng.integers(1, 7)) for _ in range(nd)]
    offsets = [[int(rng.integers(0, 40)) for _ in range(nd)] for _ in range(120)]
    meta = meta_for(nd, cs)
    assert regions_v_waves(meta, offsets, [shape] * len(offsets)) == regions_waves(meta, offsets, shape)


def test_v_waves_fixed_cases():
    meta = meta_for(2, [4, 4])
    # a zero-extent box between two that overlap: it intersects nothing and stays in the current wave
    assert regions_v_waves(meta, [[0, 0], [1, 1], [2, 2]], [[4, 4], [0, 3], [9, 1]]) == (2, [0, 0, 1])
    # touching boxes of different shapes share a wave; a small box inside a large one does not
    assert regions_v_waves(meta, [[0, 0], [3, 0], [0, 5]], [[3, 5], [20, 1], [1, 7]]) == (1, [0, 0, 0])
    assert regions_v_waves(meta, [[0, 0], [50, 60]], [[100, 100], [1, 1]]) == (2, [0, 1])
    assert regions_v_waves(meta, [], []) == (0, [])
    # ends that saturate at 2^64-1
    assert regions_v_waves(meta, [[U64_MAX, 0], [U64_MAX, 0]], [[3, 5], [9, 9]]) == (1, [0, 0])
    assert regions_v_waves(meta, [[U64_MAX - 1, 0], [U64_MAX - 6, 1]], [[3, 5], [7, 2]]) == (2, [0, 1])


def test_scratch_bytes_are_monotonic_and_non_zero():
    L = _native.load_library()
    sizes = [L.zcg_regions_v_scratch_bytes(n) for n in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 32) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s > 0 for s in sizes[1:])
    assert sizes[-1] >= 8 * (1 << 32)  # a prefix word per box


def test_vbox_layout_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zchunk_gpu.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(zcg_vbox), offsetof(zcg_vbox, shape),
 offsetof(zcg_vbox, strides), offsetof(zcg_vbox, base));return 0;}
'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    V = _native.VBox
    assert [int(x) for x in out] == [ctypes.sizeof(V), V.shape.offset, V.strides.offset, V.base.offset]


def test_store_calls_refuse_missing_arguments_without_a_gpu():
    """No context, no metadata, no root: InvalidInput from each of the four
    store calls before the GPU or a file is touched."""
    L = _native.load_library()
    st, am, msg = _native.array_meta_from_json(meta_for(2, [4, 4], [10, 10]).to_json())
    assert st == _native.OK, msg
    keep = ((ctypes.c_uint64 * 2)(2, 2), (ctypes.c_uint64 * 2)(0, 0), (ctypes.c_void_p * 1)(0))
    shp, off, buf = [ctypes.addressof(k) for k in keep]
    m = ctypes.byref(am)
    bad = _native.INVALID_INPUT
    assert L.zcg_store_read_boxes_v(None, m, b"/r", b"a", shp, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_write_boxes_v(None, m, b"/r", b"a", shp, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_read_boxes_v_device(None, m, b"/r", b"a", shp, None, 1, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_write_boxes_v_device(None, m, b"/r", b"a", shp, None, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_read_boxes_v(None, None, None, b"a", shp, off, buf, 1, 0, 1) == bad
    assert L.zcg_store_write_boxes_v(None, None, None, b"a", shp, off, buf, 1, 0, 1) == bad
    # the device-level calls: no context
    assert L.zcg_read_regions_v(None, None, None, None, None, None, 0, None, None, None) == bad
    assert L.zcg_write_regions_v(None, None, None, None, None, None, 3, None, None, None) == bad
