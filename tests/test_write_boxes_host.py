"""zcg_regions_waves, the host-only planning step of the batched box write:
the greedy split of a box list into consecutive runs of pairwise disjoint
boxes, against a brute-force numpy restatement of the rule.  No GPU."""
import time

import numpy as np
import pytest

from zarr_amd import ArrayMetadata
from zarr_amd.region import regions_waves

U64_MAX = (1 << 64) - 1


def waves_ref(offsets, shape):
    """The rule as the header states it: box 0 is in wave 0; box b opens a new
    wave iff its extent (offset .. offset + shape, ends saturating at 2^64-1)
    shares at least one element in every dimension with a box of the current
    wave.  A zero extent in `shape`: nothing intersects, one wave."""
    B = len(offsets)
    if B == 0:
        return 0, []
    if 0 in shape:
        return 1, [0] * B
    lo = np.array(offsets, dtype=object).reshape(B, len(shape))
    hi = np.array([[min(int(o) + int(s), U64_MAX) for o, s in zip(off, shape)] for off in offsets], dtype=object)
    wave_of, cur, start = [], 0, 0
    for b in range(B):
        hit = False
        for a in range(start, b):
            if all(max(lo[a][d], lo[b][d]) < min(hi[a][d], hi[b][d]) for d in range(len(shape))):
                hit = True
                break
        if hit:
            cur += 1
            start = b
        wave_of.append(cur)
    return cur + 1, wave_of


def meta_for(nd, cs):
    return ArrayMetadata.new([1 << 20] * nd, cs, "<u2")


@pytest.mark.parametrize("seed", range(40))
def test_waves_equal_the_brute_force_rule(seed):
    """1-4 dimensions, B in {0, 1, 2, 50, 400}, box extents 1-9 (and, for some
    seeds, a zero extent), offsets in a small window so that boxes overlap,
    touch and repeat, or next to 2^64 so that the ends saturate."""
    rng = np.random.default_rng(7700 + seed)
    nd = 1 + seed % 4
    B = [0, 1, 2, 50, 400][(seed // 4) % 5]
    shape = [int(rng.integers(1, 10)) for _ in range(nd)]
    if seed % 9 == 8:
        shape[int(rng.integers(0, nd))] = 0
    cs = [int(rng.integers(1, 10)) for _ in range(nd)]
    # a window sized so that a fair share of the pairs intersect
    win = [int(s * max(2, round((B or 1) ** (1.0 / nd)) * (1 + seed % 3))) + 1 for s in shape]
    base = [U64_MAX - w // 2 if seed % 5 == 4 else int(rng.integers(0, 1000)) for w in win]
    offsets = [[min(U64_MAX, b + int(rng.integers(0, w))) for b, w in zip(base, win)] for _ in range(B)]
    for k in range(1, B, 7):  # duplicates, and boxes that only touch an earlier one
        src = offsets[int(rng.integers(0, k))]
        if k % 2:
            offsets[k] = list(src)
        else:
            d = int(rng.integers(0, nd))
            offsets[k] = list(src)
            offsets[k][d] = min(U64_MAX, src[d] + shape[d])
    n, wave_of = regions_waves(meta_for(nd, cs), offsets, shape)
    n_ref, ref = waves_ref(offsets, shape)
    assert (n, list(wave_of)) == (n_ref, ref)
    assert all(a <= b for a, b in zip(wave_of, wave_of[1:]))


def test_touching_boxes_share_a_wave_and_duplicates_do_not():
    meta = meta_for(2, [4, 4])
    assert regions_waves(meta, [[0, 0], [3, 0], [0, 5], [3, 5]], [3, 5]) == (1, [0, 0, 0, 0])
    assert regions_waves(meta, [[0, 0], [0, 0], [0, 0]], [3, 5]) == (3, [0, 1, 2])
    assert regions_waves(meta, [[0, 0], [2, 4], [9, 9], [2, 4]], [3, 5]) == (3, [0, 1, 1, 2])
    assert regions_waves(meta, [], [3, 5]) == (0, [])
    assert regions_waves(meta, [[0, 0], [0, 0]], [3, 0]) == (1, [0, 0])
    # an end that saturates at 2^64-1: the last element is never shared
    assert regions_waves(meta, [[U64_MAX, 0], [U64_MAX, 0]], [3, 5]) == (1, [0, 0])
    assert regions_waves(meta, [[U64_MAX - 1, 0], [U64_MAX - 2, 1]], [3, 5]) == (2, [0, 1])


def test_disjoint_boxes_cost_no_quadratic_time():
    """20 000 pairwise disjoint boxes are one wave, within a second or two: a
    box is compared with its neighbours only."""
    side = 142  # 142 * 142 >= 20 000
    offsets = [[7 * i, 5 * j] for i in range(side) for j in range(side)][:20000]
    offs = np.asarray(offsets, np.uint64)
    meta = meta_for(2, [16, 3])
    t0 = time.perf_counter()
    n, wave_of = regions_waves(meta, offs, [7, 5])
    dt = time.perf_counter() - t0
    assert n == 1 and not any(wave_of)
    assert dt < 2.0, dt
    # the same boxes, each shifted to overlap its predecessor: 20 000 waves
    n2, w2 = regions_waves(meta, [[i, i] for i in range(20000)], [7, 5])
    assert n2 == 20000 and list(w2) == list(range(20000))
