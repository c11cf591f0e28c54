"""Strided boxes on the GPU: zcg_read_regions_s (a sample count, a step per
dimension and a view per box, one shared chunk table) against a numpy model —
the oracle's read_ndarray / read_ndarray_into (oracle/region_ref.py) on the
box's dense hull, sliced [::step] — and, with every step 1, against
zcg_read_regions_v."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes import SENTINEL, TYPESTR, UINT, Store  # noqa: E402
from test_gpu_boxes_v import Views, bound_of, fast_dim, tiny_store  # noqa: E402
from test_gpu_boxes_v import mixed_case as dense_mixed_case  # noqa: E402
from zarr_amd import ArrayMetadata, _native  # noqa: E402
from zarr_amd.region import (assemble_regions_s, assemble_regions_v, region_s_chunks, regions_s_grid,  # noqa: E402
                             regions_s_scratch_bytes, regions_v_grid, sboxes_tensor, vboxes_tensor)

pytestmark = pytest.mark.gpu


def hull_of(counts, steps):
    return [(c - 1) * s + 1 if c else 0 for c, s in zip(counts, steps)]


def model(shape, cs, order, off, counts, steps, get, dt, fill, fillv, sent):
    """What box (off, counts, steps) must hold: the oracle's read of the dense
    hull — filled, or into an array that holds the view's prior content (the
    sentinel) — sliced [::step]."""
    hull = hull_of(counts, steps)
    if fill:
        H = region_ref.read_ndarray(shape, cs, order, off, hull, get, dt, fillv)
    else:
        H = np.full(tuple(hull), sent, dtype=dt)
        region_ref.read_ndarray_into(shape, cs, order, off, hull, get, H)
    w = H[tuple(slice(None, None, int(s)) for s in steps)]
    assert list(w.shape) == list(counts)
    return w


def pruned_table(store, meta, offsets, counts, steps):
    """The store's table with the entry of every chunk that no box touches set
    to NULL: a wrong chunk index then shows as missing data."""
    keep = set()
    for off, cnt, stp in zip(offsets, counts, steps):
        if 0 in stp:
            continue
        lo, n, touched, count = region_s_chunks(meta, off, cnt, stp)
        if count:
            keep |= set(itertools.product(*[[lo[d] + j for j in range(n[d]) if touched[d][j]]
                                            for d in range(len(lo))]))
    t = store.table()
    for i, c in enumerate(store.coords):
        if c not in keep:
            t[i] = 0
    return t, keep


def expected_buffer(views, B, boxes_ok, make):
    """The whole output buffer: sentinel everywhere but in the sampled elements of the boxes in boxes_ok."""
    want = np.full(views.size, SENTINEL, np.uint8)
    for b in range(B):
        if b in boxes_ok:
            w, dt = make(b)
            if w.size:
                views.view(want, b, dt)[...] = w
    return want


def mixed_case(seed):
    """The boxes every case mixes into one call, with V = 16 / elem_size and
    the chunk fast extent cf in {61, 100, 257}.  (fast count, fast step): (1, 1),
    (V-1, 2), (32V-1, 3), (32V, V), (32V+1, V+1), (one row piece + 5, 2), the
    same with step 1 and with step 3 from a small offset, (32V, 1), (32V+1, 2),
    (5, cf), (7, cf+1), (3, 2cf+5); slow steps drawn from 1, 2, the chunk extent
    and the chunk extent plus 1; for ndim > 1 a tile-walk box (fast count 3V+1,
    fast step 2) of more than one tile; a zero-extent box between two others; a
    box partly and a box wholly outside the array; a duplicate of an earlier
    box; for ndim > 1 a tile-walk box of the dense walk (fast count 31V-1, fast
    step 1, every slow dimension every second index) of more than one tile,
    whose rows of 496 - es bytes make the 16-byte pieces cross row ends."""
    rng = np.random.default_rng(47000 + seed)
    es = [1, 2, 4, 8][seed % 4]
    order = "F" if seed % 3 == 1 else "C"
    V = 16 // es
    if seed == 9:  # the 8-dimensional case
        nd, aslow, cslow = 8, [2, 3, 2, 2, 2, 2, 2], [1, 2, 2, 1, 2, 1, 2]
        cfast = 257
    else:
        nd = 1 + seed % 4
        aslow = {1: [], 2: [96], 3: [10, 11], 4: [5, 6, 5]}[nd]
        cslow = [int(rng.integers(1, 5)) for _ in aslow]
        cfast = [61, 100, 257][seed % 3]
    afast = 3 * 4096 // es + 64
    piece = 4096 // es  # one row piece: 4 x 64 lanes x 16 bytes

    def dims(slow, fast):  # per array dim: the fast dimension is the first in F order, the last in C order
        return [fast] + list(slow) if order == "F" else list(slow) + [fast]

    shape, cs = dims(aslow, afast), dims(cslow, cfast)
    fd = fast_dim(nd, order)

    def box(fast, fstep, off_fast=None, slow=None, slow_steps=None):
        scnt, sstep = [], []
        for a, c in zip(aslow, cslow):
            k = int(rng.integers(1, min(3, a) + 1))
            s = int(rng.choice([1, 2, c, c + 1]))
            if (k - 1) * s + 1 > a:
                s = 1
            scnt.append(k)
            sstep.append(s)
        if slow is not None:
            scnt, sstep = list(slow), list(slow_steps) if slow_steps is not None else [1] * len(slow)
        cnt, stp = dims(scnt, fast), dims(sstep, fstep)
        hull = hull_of(cnt, stp)
        assert hull[fd] <= afast
        off = [int(rng.integers(0, max(1, s - h + 1))) for s, h in zip(shape, hull)]
        if off_fast is not None:
            off[fd] = off_fast
        return off, cnt, stp

    boxes = [box(1, 1), box(V - 1, 2), box(32 * V - 1, 3)]
    zoff, zcnt, zstp = box(5, 2)
    zcnt[int(rng.integers(0, nd))] = 0
    boxes.append((zoff, zcnt, zstp))
    boxes += [box(32 * V, V), box(32 * V + 1, V + 1), box(piece + 5, 2), box(piece + 5, 1),
              box(piece + 5, 3, off_fast=int(rng.integers(0, 50))), box(32 * V, 1), box(32 * V + 1, 2),
              box(5, cfast), box(7, cfast + 1), box(3, 2 * cfast + 5)]
    if nd > 1:
        boxes.append(box(3 * V + 1, 2, slow=aslow))
        if nd < 8:
            assert int(np.prod(boxes[-1][1])) * es > 4096
    poff, pcnt, pstp = box(V + 2, 3)
    boxes.append(([s - 1 for s in shape], pcnt, pstp))  # partly outside: one sample per dimension is inside
    woff, wcnt, wstp = box(2 * V, 2)
    d = int(rng.integers(0, nd))
    woff[d] = (shape[d] // cs[d] + 2) * cs[d]  # wholly outside, at a chunk boundary: it visits no chunk
    boxes.append((woff, wcnt, wstp))
    boxes.append(tuple(list(x) for x in boxes[2]))  # a duplicate, into its own output
    if nd > 1:  # after the duplicate: the boxes above keep their draws
        boxes.append(box(31 * V - 1, 1, slow=[(a + 1) // 2 for a in aslow], slow_steps=[2] * len(aslow)))
        if nd < 8:
            assert int(np.prod(boxes[-1][1])) * es > 4096
    offsets, counts, steps = [b[0] for b in boxes], [b[1] for b in boxes], [b[2] for b in boxes]
    absent = 0.25 if seed % 2 == 0 else 0.0
    return rng, es, order, shape, cs, offsets, counts, steps, absent


@pytest.mark.parametrize("seed", range(10))
def test_regions_s_equal_the_sliced_hull_of_the_oracle(seed):
    """10 seeds: 1-4 dimensions and one 8-dimensional case, element sizes
    1/2/4/8, C and F order, with (even seeds) and without absent chunks, fill
    on and off; the boxes of mixed_case in one call, their views dense, doubled
    or with a negative slow stride; table entries of chunks that hold no sample
    are NULL.  The whole buffer, sentinel bytes around and between the views
    included, must equal the model byte for byte."""
    import torch
    rng, es, order, shape, cs, offsets, counts, steps, absent = mixed_case(seed)
    nd, B = len(shape), len(offsets)
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lo, n = regions_s_grid(meta, offsets, counts, steps)
    store = Store(rng, meta, lo, n, es, order, absent_frac=absent)
    dev = store.dev
    table_h, keep = pruned_table(store, meta, offsets, counts, steps)
    assert len(keep) and (nd == 1 or len(keep) < len(store.coords))  # something is pruned
    table = torch.from_numpy(table_h).to(dev)
    fillv = 0x1122334455667788 & ((1 << (8 * es)) - 1)
    dt = UINT[es]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dt)[0]
    views = Views(counts, es, order, shift=seed)
    bound = bound_of(counts, nd)
    for fill in (0, 1):
        out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
        status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        sb = sboxes_tensor(offsets, counts, steps, views.strides, views.bases(out))
        assemble_regions_s(meta, bound, es, table, lo, n, sb, status, bool(fill), fillv)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        got = out.cpu().numpy()
        want = expected_buffer(views, B, range(B), lambda b: (
            model(shape, cs, order, offsets[b], counts[b], steps[b], store.chunks.get, dt, fill, fillv, sent), dt))
        for b in range(B):
            assert np.array_equal(views.view(got, b, dt), views.view(want, b, dt)), (seed, fill, b, offsets[b],
                                                                                    counts[b], steps[b])
        assert np.array_equal(got, want), (seed, fill)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 9])
def test_all_steps_one_is_byte_identical_to_regions_v(seed):
    """The dense mixed case of the _v tests through both calls."""
    import torch
    rng, es, order, shape, cs, offsets, shapes, absent = dense_mixed_case(seed)
    nd, B = len(shape), len(offsets)
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    lo, n = regions_v_grid(meta, offsets, shapes)
    assert regions_s_grid(meta, offsets, shapes, [[1] * nd] * B) == (lo, n)
    store = Store(rng, meta, lo, n, es, order, absent_frac=absent)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    views = Views(shapes, es, order, shift=seed)
    bound = bound_of(shapes, nd)
    for fill in (0, 1):
        outs = []
        for strided in (False, True):
            out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
            status = torch.full((B,), -1, dtype=torch.int32, device=dev)
            if strided:
                bx = sboxes_tensor(offsets, shapes, [[1] * nd] * B, views.strides, views.bases(out))
                assemble_regions_s(meta, bound, es, table, lo, n, bx, status, bool(fill), 0x77)
            else:
                bx = vboxes_tensor(offsets, shapes, views.strides, views.bases(out))
                assemble_regions_v(meta, bound, es, table, lo, n, bx, status, bool(fill), 0x77)
            torch.cuda.synchronize()
            assert status.cpu().tolist() == [_native.OK] * B
            outs.append(out.cpu().numpy())
        assert not (outs[0] == SENTINEL).all()
        assert np.array_equal(outs[0], outs[1]), (seed, fill)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1024, 1025])
def test_box_counts_at_the_edges_of_the_scan_and_the_search(B):
    """B tiny strided boxes (0-4 x 0-5 samples, steps 1-3 x 1-10, so some have
    a zero extent and some fast steps exceed the chunk extent 9), dense views,
    in one call: wave and workgroup edges of the plan kernel's prefix scan and
    of the walk's unit search."""
    import torch
    meta, store = tiny_store()
    shape, cs = meta.shape, meta.chunk_shape
    rng = np.random.default_rng(900 + B)
    counts = [[int(rng.integers(0, 5)), int(rng.integers(0, 6))] for _ in range(B)]
    steps = [[int(rng.integers(1, 4)), int(rng.integers(1, 11))] for _ in range(B)]
    offsets = [[int(rng.integers(0, 30)), int(rng.integers(0, 12))] for _ in range(B)]
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    views = Views(counts, 2, "C", modes=(0,))
    out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sb = sboxes_tensor(offsets, counts, steps, views.strides, views.bases(out))
    assemble_regions_s(meta, [4, 5], 2, table, store.lo, store.n, sb, status, True, 0xBEEF)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * B
    want = expected_buffer(views, B, range(B), lambda b: (
        model(shape, cs, "C", offsets[b], counts[b], steps[b], store.chunks.get, np.uint16, 1, 0xBEEF, 0), np.uint16))
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("fast", [20, 200])
def test_refused_boxes_in_the_middle_of_a_call(fast):
    """Between good boxes (tile walk and row walk, fast step 3): a step of 0, a
    count above the bound, a hull whose grid range is outside the table, and
    two hulls that reach 2^32 (count 2 with a step next to 2^32, and a step
    above 2^32).  Each gets its status, its output stays all sentinel, the
    neighbours are exact, and every status word is written."""
    import torch
    rng = np.random.default_rng(fast)
    shape, cs = [40, 1000], [4, 16]
    meta = ArrayMetadata.new(shape, cs, "<u4")
    meta.chunk_memory_layout = "C"
    offsets = [[3, 10], [5, 30], [6, 40], [2, 50], [7, 50], [30, 700], [1, 2], [4, 4], [1, 90]]
    counts = [[5, fast], [3, fast], [2, fast - 3], [6, fast], [4, 0], [3, fast - 5], [2, 2], [2, 2], [5, fast - 1]]
    steps = [[2, 3], [1, 0], [5, 1], [1, 1], [1, 2], [1, 3], [1, (1 << 32) - 10], [(1 << 40) + 1, 1], [3, 4]]
    good = [0, 2, 4, 8]
    bound = bound_of([counts[b] for b in good], 2)
    assert counts[3][0] == bound[0] + 1  # box 3 is above the bound, in a slow dimension
    g = lambda xs: [xs[b] for b in good]  # noqa: E731
    lo, n = regions_s_grid(meta, g(offsets), g(counts), g(steps))  # box 5 lies outside
    assert lo[0] + n[0] <= 30 // 4
    store = Store(rng, meta, lo, n, 4, "C", absent_frac=0.0)
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    views = Views(counts, 4, "C", modes=(0,))
    out = torch.full((views.size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((len(offsets),), -1, dtype=torch.int32, device=dev)
    sb = sboxes_tensor(offsets, counts, steps, views.strides, views.bases(out))
    assemble_regions_s(meta, bound, 4, table, lo, n, sb, status, True, 9)
    torch.cuda.synchronize()
    bad, uns, ok = _native.INVALID_INPUT, _native.UNSUPPORTED, _native.OK
    assert status.cpu().tolist() == [ok, bad, ok, bad, ok, bad, uns, uns, ok]
    want = expected_buffer(views, len(offsets), good, lambda b: (
        model(shape, cs, "C", offsets[b], counts[b], steps[b], store.chunks.get, np.uint32, 1, 9, 0), np.uint32))
    assert np.array_equal(out.cpu().numpy(), want)


def test_capture_and_replay_with_new_offsets_counts_steps_and_bases():
    """One captured zcg_read_regions_s call (one graph, no parallel branches),
    replayed twice with new offsets, sample counts, steps, strides and bases in
    d_boxes, all inside the bound: the kernels read them when they run."""
    import torch
    rng = np.random.default_rng(16)
    shape, cs, bound = [50, 900], [7, 9], [6, 290]  # rows of 256 samples and more go a wave per row piece
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    B = 5

    def draw():
        counts = [[int(rng.integers(0, bound[0] + 1)), int(rng.choice([1, 11, 255, 256, 290]))] for _ in range(B)]
        steps = [[int(rng.choice([1, 2, 7, 8])), int(rng.choice([1, 2, 3]))] for _ in range(B)]
        offsets = [[int(rng.integers(0, 8)), int(rng.integers(0, 30))] for _ in range(B)]
        return offsets, counts, steps

    sets = [draw() for _ in range(3)]
    store = Store(rng, meta, [0, 0], [8, 100], 2, "C")
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    size = max(Views(s[1], 2, "C", shift=i).size for i, s in enumerate(sets))
    out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(regions_s_scratch_bytes(B), dtype=torch.uint8, device=dev)
    v0 = Views(sets[0][1], 2, "C")
    sb = sboxes_tensor(sets[0][0], sets[0][1], sets[0][2], v0.strides, v0.bases(out))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assemble_regions_s(meta, bound, 2, table, store.lo, store.n, sb, status, True, 3, scratch=scratch)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assemble_regions_s(meta, bound, 2, table, store.lo, store.n, sb, status, True, 3, scratch=scratch)
    for i, (offsets, counts, steps) in enumerate(sets[1:], 1):
        views = Views(counts, 2, "C", shift=i)
        sb.copy_(sboxes_tensor(offsets, counts, steps, views.strides, views.bases(out)))
        out.fill_(SENTINEL)
        status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        got = out.cpu().numpy()
        for b in range(B):
            w = model(shape, cs, "C", offsets[b], counts[b], steps[b], store.chunks.get, np.uint16, 1, 3, 0)
            assert np.array_equal(views.view(got, b, np.uint16), w), (i, b)


def test_trivial_calls():
    """n_boxes = 0 returns Ok and writes nothing.  A zero bound: boxes with a
    zero count are Ok, a box with a count above it is InvalidInput, every
    status word is written and no element is.  A bound whose extent plus the
    chunk extent reaches 2^32 is Unsupported, and nothing is launched."""
    import torch
    meta, store = tiny_store()
    dev = store.dev
    table = torch.from_numpy(store.table()).to(dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    assemble_regions_s(meta, [3, 3], 2, table, store.lo, store.n, None, status, True, 0)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-1, -1]
    sb = sboxes_tensor([[1, 1], [2, 2]], [[0, 2], [1, 3]], [[2, 2], [1, 3]], [[3, 1], [3, 1]],
                       [out.data_ptr(), out.data_ptr() + 2048])
    assemble_regions_s(meta, [0, 3], 2, table, store.lo, store.n, sb, status, True, 0)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK, _native.INVALID_INPUT]
    status.fill_(-1)
    with pytest.raises(_native.NativeUnavailable):
        assemble_regions_s(meta, [3, (1 << 32) - 8], 2, table, store.lo, store.n, sb, status, True, 0)  # chunk 9
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and status.cpu().tolist() == [-1, -1]
    assert ctypes.sizeof(_native.SBox) == 4 * 8 * 8 + 8
