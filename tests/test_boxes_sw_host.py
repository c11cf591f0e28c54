"""The host-only parts of the strided box write: zcg_regions_s_waves against a
brute-force model that materialises every box's sample set, the argument
errors of write_ndarrays_s and of the two store calls, and the cover rule (when
a touched chunk is not read before the scatter) restated in Python against
zcg_region_s_chunks' touched sets.  No GPU."""
import ctypes
import itertools
import os
import time

import numpy as np
import pytest

from zarr_amd import ArrayMetadata, ZarrIOError, _native
from zarr_amd.region import region_s_chunks, regions_s_waves, regions_v_waves, write_ndarrays_s

U64_MAX = (1 << 64) - 1
STEPS = [1, 2, 3, 4, 6, 7, 64, 65]


def meta_for(nd, cs):
    return ArrayMetadata.new([1 << 20] * nd, cs, "<u2")


def samples(off, cnt, step):
    """Per dimension the set of array indices a box samples; a step of 0 or a
    zero count makes every set empty (such a box intersects nothing)."""
    if 0 in step or 0 in cnt:
        return [set() for _ in off]
    return [{o + i * s for i in range(c)} for o, c, s in zip(off, cnt, step)]


def waves_ref(offsets, counts, steps):
    """Greedy and consecutive: box b opens a new wave iff it shares a sample,
    in every dimension, with a box of the current wave."""
    sets = [samples(o, c, s) for o, c, s in zip(offsets, counts, steps)]
    wave_of, cur, start = [], 0, 0
    for b in range(len(offsets)):
        if any(all(x & y for x, y in zip(sets[a], sets[b])) for a in range(start, b)):
            cur += 1
            start = b
        wave_of.append(cur)
    return (cur + 1 if offsets else 0), wave_of


@pytest.mark.parametrize("seed", range(200))
def test_s_waves_equal_the_brute_force_model(seed):
    """1-3 dimensions, up to 24 boxes, offsets below 64, 0-9 samples per
    dimension, steps from {1, 2, 3, 4, 6, 7, 64, 65}, and now and then a step of
    0; duplicates of earlier boxes so that later waves open."""
    rng = np.random.default_rng(88000 + seed)
    nd = 1 + seed % 3
    B = int(rng.integers(0, 25))
    cs = [int(rng.integers(1, 10)) for _ in range(nd)]
    offsets = [[int(rng.integers(0, 64)) for _ in range(nd)] for _ in range(B)]
    counts = [[int(rng.integers(0, 10)) for _ in range(nd)] for _ in range(B)]
    steps = [[int(rng.choice(STEPS)) for _ in range(nd)] for _ in range(B)]
    for b in range(B):
        if rng.random() < 0.06:
            steps[b][int(rng.integers(0, nd))] = 0
        if b and rng.random() < 0.15:
            a = int(rng.integers(0, b))
            offsets[b], counts[b], steps[b] = list(offsets[a]), list(counts[a]), list(steps[a])
    got = regions_s_waves(meta_for(nd, cs), offsets, counts, steps)
    assert got == waves_ref(offsets, counts, steps), (offsets, counts, steps)


def test_s_waves_fixed_cases():
    meta = meta_for(2, [4, 4])
    # even and odd planes of one hull share no sample: one wave
    assert regions_s_waves(meta, [[0, 0], [1, 0]], [[8, 16]] * 2, [[2, 1]] * 2) == (1, [0, 0])
    assert regions_s_waves(meta, [[0, 0], [0, 1], [1, 0], [1, 1]], [[8, 8]] * 4, [[2, 2]] * 4) == (1, [0] * 4)
    # the same offset twice: the second box opens a wave
    assert regions_s_waves(meta, [[3, 5], [3, 5]], [[8, 8]] * 2, [[2, 3]] * 2) == (2, [0, 1])
    # gcd-compatible progressions (steps 4 and 6, offsets 0 and 2: common indices 8, 20, ...) whose
    # first common index lies past the first box's last sample (4): one wave; one more sample: two
    assert regions_s_waves(meta, [[0, 0], [2, 0]], [[2, 1], [9, 1]], [[4, 1], [6, 1]]) == (1, [0, 0])
    assert regions_s_waves(meta, [[0, 0], [2, 0]], [[3, 1], [9, 1]], [[4, 1], [6, 1]]) == (2, [0, 1])
    # incompatible residues never meet, however long the boxes
    assert regions_s_waves(meta, [[0, 0], [3, 0]], [[1 << 20, 1], [1 << 20, 1]], [[6, 1], [4, 1]]) == (1, [0, 0])
    # the step of a dimension with one sample is irrelevant, a step of 0 and a zero extent intersect nothing
    assert regions_s_waves(meta, [[5, 5], [5, 5]], [[1, 1]] * 2, [[7, 9], [1000, 3]]) == (2, [0, 1])
    assert regions_s_waves(meta, [[5, 5], [5, 5], [5, 5]], [[2, 2]] * 3, [[1, 1], [0, 1], [1, 1]]) == (2, [0, 0, 1])
    assert regions_s_waves(meta, [[5, 5], [5, 5], [5, 5]], [[2, 2], [0, 2], [2, 2]], [[1, 1]] * 3) == (2, [0, 0, 1])
    assert regions_s_waves(meta, [], [], []) == (0, [])


def test_s_waves_near_the_end_of_the_index_space_need_no_long_loop():
    """Steps near 2^63 and offsets near 2^64: a pair with a hull end beyond
    2^64 - 1 is compared by the hulls' intervals with saturated ends, which
    takes two boxes whose hulls overlap for intersecting even where the samples
    do not meet; pairs whose hulls fit are compared exactly.  No loop over
    samples: counts of 2^40 return at once."""
    meta = meta_for(1, [16])
    big = (1 << 63) - 5
    t0 = time.perf_counter()
    # hulls 10 .. 10 + big + 1 and 11 .. : both fit, residues differ by 1 with a common step: exact, one wave
    assert regions_s_waves(meta, [[10], [11]], [[2], [2]], [[big], [big]]) == (1, [0, 0])
    # the second hull's end passes 2^64 - 1 (the first, 2^63 .. 2^64 - 4, fits): the intervals with
    # saturated ends overlap -> a new wave, although the samples do not meet; a first hull that ends
    # below the second one's offset stays in the wave
    assert regions_s_waves(meta, [[1 << 63], [U64_MAX - 20]], [[2], [2]], [[big], [big]]) == (2, [0, 1])
    assert regions_s_waves(meta, [[10], [U64_MAX - 20]], [[2], [2]], [[big], [big]]) == (1, [0, 0])
    # both ends saturate; the intervals [2^64 - 40, 2^64 - 1) and [2^64 - 30, 2^64 - 1) overlap
    assert regions_s_waves(meta, [[U64_MAX - 39], [U64_MAX - 29]], [[2], [2]], [[big], [big]]) == (2, [0, 1])
    # long progressions, exact: step 2^20 from 0 and from 1 never meet; from 2^20 they do
    n = 1 << 40
    assert regions_s_waves(meta, [[0], [1]], [[n], [n]], [[1 << 20], [1 << 20]]) == (1, [0, 0])
    assert regions_s_waves(meta, [[0], [1 << 20]], [[n], [n]], [[1 << 20], [3 << 20]]) == (2, [0, 1])
    assert time.perf_counter() - t0 < 1.0


@pytest.mark.parametrize("seed", range(50))
def test_s_waves_with_all_steps_one_equal_v_waves(seed):
    rng = np.random.default_rng(4100 + seed)
    nd = 1 + seed % 4
    B = int(rng.integers(1, 60))
    cs = [int(rng.integers(1, 9)) for _ in range(nd)]
    win = 6 + seed % 30
    base = U64_MAX - win // 2 if seed % 10 == 9 else 0
    offsets = [[min(U64_MAX, base + int(rng.integers(0, win))) for _ in range(nd)] for _ in range(B)]
    shapes = [[int(rng.integers(0, 7)) for _ in range(nd)] for _ in range(B)]
    meta = meta_for(nd, cs)
    assert regions_s_waves(meta, offsets, shapes, [[1] * nd] * B) == regions_v_waves(meta, offsets, shapes)


def files_under(root):
    return [os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs]


class _Hier:
    def __init__(self, base_path):
        self.base_path = base_path


def test_write_ndarrays_s_argument_errors_need_no_gpu(tmp_path):
    """A step of 0, a steps array of the wrong shape, an array of the wrong
    rank or element type, arrays and offsets that differ in number and a hull
    of 2^32 are refused before any native call that needs a context; nothing
    is created under the root."""
    meta = ArrayMetadata.new([10, 10], [4, 4], "<u2")
    h = _Hier(str(tmp_path))
    a = [np.zeros((2, 2), np.uint16), np.zeros((3, 2), np.uint16), np.zeros((1, 1), np.uint16)]
    offs = [[0, 0], [1, 1], [2, 2]]

    def refused(kind, offsets, steps, arrays):
        with pytest.raises(ZarrIOError) as e:
            write_ndarrays_s(h, "a", meta, offsets, steps, arrays)
        assert e.value.kind == kind, e.value

    refused("InvalidInput", offs, [2, 0], a)
    refused("InvalidInput", offs, [[1, 1], [1, 0], [1, 1]], a)
    refused("InvalidInput", offs, [1, 1, 1], a)
    refused("InvalidInput", offs, [[1, 1], [1, 1]], a)
    refused("InvalidInput", offs, 3, a)
    refused("InvalidData", offs, [1, 1], a[:2])
    refused("InvalidData", offs, [1, 1], [a[0], np.zeros((3,), np.uint16), a[2]])
    refused("InvalidInput", offs, [1, 1], [x.astype(np.float32) for x in a])
    refused("Unsupported", offs, [[1, 1], [(1 << 31) - 1, 1], [1, 1]], a)  # 2 * (2^31 - 1) + 4 >= 2^32
    big = ArrayMetadata.new([1 << 40, 10], [4, 4], "<u2")
    with pytest.raises(ZarrIOError) as e:
        write_ndarrays_s(h, "a", big, [[0, 0]], [[1 << 32, 1]], [np.zeros((2, 2), np.uint16)])
    assert e.value.kind == "Unsupported"
    assert files_under(tmp_path) == []


def test_store_calls_refuse_their_arguments_without_a_context(tmp_path):
    """NULL arguments, a step of 0, a raw element type, ndim != chunk_ndim and
    a hull of 2^32: both store calls answer from the arguments alone, and
    zcg_write_regions_s and zcg_regions_s_waves refuse NULLs."""
    L = _native.load_library()
    root = os.fsencode(str(tmp_path))

    def fresh():
        st, am, msg = _native.array_meta_from_json(ArrayMetadata.new([10, 10], [4, 4], "<u2").to_json())
        assert st == _native.OK, msg
        return am

    def args(shape=(2, 2), step=(1, 2)):
        keep = ((ctypes.c_uint64 * 2)(*shape), (ctypes.c_uint64 * 2)(*step), (ctypes.c_uint64 * 2)(0, 0),
                (ctypes.c_void_p * 1)(0))
        return keep, [ctypes.addressof(k) for k in keep]

    def both(am, shp, stp, off, buf, n=1):
        m = ctypes.byref(am) if am is not None else None
        return (L.zcg_store_write_boxes_s(None, m, root, b"a", shp, stp, off, buf, n, 0, 1),
                L.zcg_store_write_boxes_s_device(None, m, root, b"a", shp, stp, None, off, buf, n, 0, 1))

    bad, uns = _native.INVALID_INPUT, _native.UNSUPPORTED
    keep, (shp, stp, off, buf) = args()
    assert both(fresh(), shp, stp, off, buf) == (bad, bad)  # no context
    assert both(None, shp, stp, off, buf) == (bad, bad)
    assert both(fresh(), None, stp, off, buf) == (bad, bad)
    assert both(fresh(), shp, None, off, buf) == (bad, bad)
    assert both(fresh(), shp, stp, None, buf) == (bad, bad)
    keep0, (shp0, stp0, off0, buf0) = args(step=(1, 0))
    assert both(fresh(), shp0, stp0, off0, buf0) == (bad, bad)
    am = fresh()
    am.dtype_kind = 4  # ZCG_DT_RAW
    assert both(am, shp, stp, off, buf) == (bad, bad)
    am = fresh()
    am.chunk_ndim = 3
    assert both(am, shp, stp, off, buf) == (_native.INVALID_DATA,) * 2
    keep1, (shp1, stp1, off1, buf1) = args(step=((1 << 32) - 4, 1))  # hull + chunk extent = 2^32
    assert both(fresh(), shp1, stp1, off1, buf1) == (uns, uns)
    keep2, (shp2, stp2, off2, buf2) = args(shape=(1, 2), step=((1 << 40), 1))  # one sample: its step is irrelevant
    assert both(fresh(), shp2, stp2, off2, buf2) == (bad, bad)  # in order, then no context
    assert L.zcg_write_regions_s(None, None, None, None, None, None, 0, None, None, None) == bad
    assert L.zcg_write_regions_s(None, None, None, None, None, None, 3, None, None, None) == bad
    wave = (ctypes.c_uint32 * 1)()
    assert L.zcg_regions_s_waves(None, off, shp, stp, 1, ctypes.addressof(wave)) == 0
    st, am, msg = _native.array_meta_from_json(ArrayMetadata.new([10, 10], [4, 4], "<u2").to_json())
    r = _native.Region()
    r.ndim = 2
    r.chunk_shape[0] = r.chunk_shape[1] = 4
    assert L.zcg_regions_s_waves(ctypes.byref(r), off, shp, None, 1, ctypes.addressof(wave)) == 0
    assert L.zcg_regions_s_waves(ctypes.byref(r), off, shp, stp, 1, ctypes.addressof(wave)) == 1
    assert files_under(tmp_path) == []


def covered_ref(cs, off, cnt, step, coord):
    """The cover rule, from its definition: every index of the chunk's nominal
    bounds, along every dimension, is a sample of the box."""
    for d in range(len(cs)):
        idx = {off[d] + i * step[d] for i in range(cnt[d])}
        if not all(x in idx for x in range(coord[d] * cs[d], (coord[d] + 1) * cs[d])):
            return False
    return True


def covered_rule(cs, off, cnt, step, coord):
    """The rule as the planner applies it to a TOUCHED chunk: per dimension a
    chunk extent of 1, or step 1 (a lone sample has none) and the run of
    samples across the chunk's bounds."""
    for d in range(len(cs)):
        if cs[d] == 1:
            continue
        k = step[d] if cnt[d] > 1 else 1
        if k != 1 or coord[d] * cs[d] < off[d] or (coord[d] + 1) * cs[d] > off[d] + cnt[d]:
            return False
    return True


@pytest.mark.parametrize("seed", range(100))
def test_cover_rule_on_touched_chunks(seed):
    """On zcg_region_s_chunks' touched chunks of a random box, the planner's
    closed form agrees with the definition; chunk extents of 1 and steps of 1
    are frequent, so both answers occur."""
    rng = np.random.default_rng(5600 + seed)
    nd = 1 + seed % 3
    cs = [int(rng.choice([1, 1, 2, 3, 5])) for _ in range(nd)]
    shape = [int(rng.integers(20, 60)) for _ in range(nd)]
    meta = ArrayMetadata.new(shape, cs, "<u2")
    off = [int(rng.integers(0, 12)) for _ in range(nd)]
    cnt = [int(rng.integers(1, 12)) for _ in range(nd)]
    step = [int(rng.choice([1, 1, 1, 2, 3, c, c + 1])) for c in cs]
    lo, n, touched, count = region_s_chunks(meta, off, cnt, step)
    coords = list(itertools.product(*[[lo[d] + j for j in range(n[d]) if touched[d][j]] for d in range(nd)]))
    assert len(coords) == count
    for c in coords:
        assert covered_rule(cs, off, cnt, step, c) == covered_ref(cs, off, cnt, step, c), (cs, off, cnt, step, c)
