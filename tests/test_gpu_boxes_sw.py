"""Strided box scatter on the GPU: zcg_write_regions_s (a sample count, a step
per dimension and an input view per box, one shared chunk table) against the
oracle's model — read_ndarray of the box's hull from the slots, H[::step] = box,
write_ndarray of the hull, kept for the touched chunks that have a slot
(oracle/region_ref.py) — applied box by box in order.  Every other slot byte,
the guard bytes around every slot and the input buffer must be unchanged."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes import SENTINEL, TYPESTR, UINT  # noqa: E402
from test_gpu_boxes_s import hull_of, mixed_case, pruned_table  # noqa: E402
from test_gpu_boxes_v import Views, band_boxes, bound_of  # noqa: E402
from test_gpu_write_boxes import Slots  # noqa: E402
from zarr_amd import ArrayMetadata, _native  # noqa: E402
from zarr_amd.region import (assemble_regions_s, region_s_chunks, regions_s_grid, regions_s_scratch_bytes,  # noqa: E402
                             regions_s_waves, regions_v_grid, sboxes_tensor, scatter_regions_s, scatter_regions_v,
                             vboxes_tensor)

pytestmark = pytest.mark.gpu

REC = ctypes.sizeof(_native.SBox)
UNMAPPED = 0x00007FFFDEAD0000  # an address no allocation of the test holds


def touched_coords(meta, off, counts, steps):
    if 0 in steps:
        return []
    lo, n, touched, count = region_s_chunks(meta, off, counts, steps)
    if not count:
        return []
    return list(itertools.product(*[[lo[d] + j for j in range(n[d]) if touched[d][j]] for d in range(len(lo))]))


def apply_box(meta, order, chunks, off, counts, steps, box):
    """The model for one box on `chunks` (coord -> flat elements of the chunks
    that have a slot): hull read, samples overlaid, hull written, and of the
    result only the touched chunks that have a slot are kept."""
    if 0 in counts or 0 in steps:
        return
    shape, cs = meta.shape, meta.chunk_shape
    hull = hull_of(counts, steps)
    H = region_ref.read_ndarray(shape, cs, order, off, hull, chunks.get, box.dtype, 0)
    H[tuple(slice(None, None, int(s)) for s in steps)] = box
    tmp = dict(chunks)
    region_ref.write_ndarray(shape, cs, order, off, H, tmp, 0)
    for c in touched_coords(meta, off, counts, steps):
        if c in chunks:
            chunks[c] = tmp[c]


def image_of(slots, chunks):
    """The slot buffer the model expects: the initial image with the present chunks replaced."""
    img = slots.image.copy()
    for c, o in slots.at.items():
        img[o:o + slots.D] = np.ascontiguousarray(chunks[c]).view(np.uint8)
    return img


def scatter_in_waves(meta, bound, es, table, lo, n, offsets, counts, steps, sb, status, scratch):
    """One zcg_write_regions_s call per wave of zcg_regions_s_waves, in order on one stream."""
    nw, wave_of = regions_s_waves(meta, offsets, counts, steps)
    b0, B = 0, len(offsets)
    while b0 < B:
        b1 = b0 + 1
        while b1 < B and wave_of[b1] == wave_of[b0]:
            b1 += 1
        scatter_regions_s(meta, bound, es, table, lo, n, sb[b0 * REC:b1 * REC], status[b0:b1], scratch=scratch)
        b0 = b1
    return nw


class Case:
    """mixed_case(seed) set up for a scatter: slots with guard bytes, a random
    input buffer with the boxes' views, the table with untouched entries set
    to `untouched`."""

    def __init__(self, seed, untouched=0, absent=None):
        import torch
        rng, es, order, shape, cs, offsets, counts, steps, absent_frac = mixed_case(seed)
        self.es, self.order, self.offsets, self.counts, self.steps = es, order, offsets, counts, steps
        self.nd, self.B, self.dt = len(shape), len(offsets), UINT[es]
        self.meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
        self.meta.chunk_memory_layout = order
        self.lo, self.n = regions_s_grid(self.meta, offsets, counts, steps)
        self.slots = Slots(rng, self.meta, self.lo, self.n, es, absent_frac=absent_frac if absent is None else absent)
        self.dev = self.slots.dev
        table_h, self.keep = pruned_table(self.slots, self.meta, offsets, counts, steps)
        full = self.slots.table()
        self.null_touched = sum(1 for i, c in enumerate(self.slots.coords) if c in self.keep and full[i] == 0)
        if untouched:
            for i, c in enumerate(self.slots.coords):
                if c not in self.keep:
                    table_h[i] = untouched
        self.table = torch.from_numpy(table_h).to(self.dev)
        self.views = Views(counts, es, order, shift=seed)
        self.src_h = rng.integers(0, 256, self.views.size, dtype=np.uint8)
        self.src = torch.from_numpy(self.src_h).to(self.dev)
        self.bound = bound_of(counts, self.nd)
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device=self.dev)
        self.scratch = torch.empty(regions_s_scratch_bytes(self.B), dtype=torch.uint8, device=self.dev)
        self.sb = sboxes_tensor(offsets, counts, steps, self.views.strides, self.views.bases(self.src))

    def run(self):
        import torch
        nw = scatter_in_waves(self.meta, self.bound, self.es, self.table, self.lo, self.n, self.offsets, self.counts,
                              self.steps, self.sb, self.status, self.scratch)
        torch.cuda.synchronize()
        return nw

    def want(self):
        chunks = self.slots.chunks()
        for b in range(self.B):
            apply_box(self.meta, self.order, chunks, self.offsets[b], self.counts[b], self.steps[b],
                      self.views.view(self.src_h, b, self.dt))
        return image_of(self.slots, chunks)


@pytest.mark.parametrize("seed", range(10))
def test_regions_sw_equal_the_model_box_by_box(seed):
    """10 seeds: 1-4 dimensions and one 8-dimensional case, element sizes
    1/2/4/8, C and F order, with (even seeds) and without NULL slots; the boxes
    of test_gpu_boxes_s.mixed_case, their input views dense, doubled or with a
    negative slow stride, scattered in the waves of zcg_regions_s_waves; table
    entries of chunks that hold no sample are NULL.  The whole slot buffer,
    guard bytes and NULL slots included, must equal the model byte for byte,
    and the input buffer is only read."""
    C = Case(seed)
    assert len(C.keep) and (C.nd == 1 or len(C.keep) < len(C.slots.coords))
    nw = C.run()
    assert nw > 1  # the duplicate opens a wave
    assert C.status.cpu().tolist() == [_native.OK] * C.B
    got = C.slots.buf.cpu().numpy()
    want = C.want()
    assert not np.array_equal(want, C.slots.image)
    for c, o in C.slots.at.items():
        assert np.array_equal(got[o:o + C.slots.D], want[o:o + C.slots.D]), (seed, c)
    assert np.array_equal(got, want), seed
    assert np.array_equal(C.src.cpu().numpy(), C.src_h)


@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("vstride", [1, 2])
def test_bytes_between_two_samples_keep_their_content(step, vstride):
    """u8, fast step 2 and 3, input views with a fast stride of 1 and 2, a
    long row (row pieces), a short one (tiles) and a one-sample box: the
    unsampled bytes between two samples keep their prior random content, the
    samples hold the view's values."""
    import torch
    rng = np.random.default_rng(100 * step + vstride)
    shape, cs = [6, 3000], [2, 61]
    meta = ArrayMetadata.new(shape, cs, "u1")
    meta.chunk_memory_layout = "C"
    offsets = [[0, 5], [2, 0], [4, 77], [5, 1]]
    counts = [[2, 700], [1, 100], [1, 1], [1, 515]]
    steps = [[1, step], [1, step], [1, step], [1, step]]
    B = len(offsets)
    lo, n = regions_s_grid(meta, offsets, counts, steps)
    slots = Slots(rng, meta, lo, n, 1, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    # box b's view: rows of 2 * count bytes, every vstride-th byte an element
    at, strides = [64], []
    for c in counts:
        strides.append([2 * c[1], vstride])
        at.append(at[-1] + 2 * c[0] * c[1] + 64)
    src_h = rng.integers(0, 256, at[-1], dtype=np.uint8)
    src = torch.from_numpy(src_h).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sb = sboxes_tensor(offsets, counts, steps, strides, [src.data_ptr() + a for a in at[:-1]])
    scatter_regions_s(meta, bound_of(counts, 2), 1, table, lo, n, sb, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * B
    got = slots.buf.cpu().numpy()
    before, after = slots.chunks(), slots.chunks(got)
    arr = lambda ch: np.block([[ch[(i, j)].reshape(cs) for j in range(lo[1], lo[1] + n[1])]  # noqa: E731
                               for i in range(lo[0], lo[0] + n[0])])
    A0, A1 = arr(before), arr(after)
    want = A0.copy()
    sampled = np.zeros(A0.shape, bool)
    for b in range(B):
        view = np.ndarray(tuple(counts[b]), np.uint8, buffer=src_h, offset=at[b], strides=tuple(strides[b]))
        r0, c0 = offsets[b][0] - lo[0] * cs[0], offsets[b][1] - lo[1] * cs[1]
        sl = (slice(r0, r0 + counts[b][0]), slice(c0, c0 + (counts[b][1] - 1) * step + 1, step))
        want[sl] = view
        sampled[sl] = True
    assert np.array_equal(A1[sampled], want[sampled])
    assert np.array_equal(A1[~sampled], A0[~sampled])  # the neighbours
    chunks = slots.chunks()
    for c, o in slots.at.items():  # guard bytes
        chunks[c] = after[c]
    assert np.array_equal(got, image_of(slots, chunks))
    assert np.array_equal(src.cpu().numpy(), src_h)


@pytest.mark.parametrize("seed", [0, 2])
def test_untouched_entries_are_never_dereferenced_and_null_touched_ones_drop_their_samples(seed):
    """The mixed case with ~25 % NULL slots: the entry of every chunk no box
    touches holds an address that is not mapped, and the result is the model's;
    samples whose touched chunk is NULL are dropped, the other slots exact."""
    C = Case(seed, untouched=UNMAPPED, absent=0.25)
    assert C.null_touched > 0 and (C.nd == 1 or len(C.keep) < len(C.slots.coords))
    C.run()
    assert C.status.cpu().tolist() == [_native.OK] * C.B
    assert np.array_equal(C.slots.buf.cpu().numpy(), C.want()), seed


@pytest.mark.parametrize("fast", [20, 200])
def test_refused_boxes_in_the_middle_of_a_call(fast):
    """One call (tile walk and row walk) of four good boxes that share no
    sample, and between them: a step of 0, a count above the bound, a hull
    whose grid range is outside the table, and two hulls that reach 2^32.  Each
    gets its status word, writes nothing, and the others are exact."""
    import torch
    rng = np.random.default_rng(fast)
    shape, cs = [40, 1000], [4, 16]
    meta = ArrayMetadata.new(shape, cs, "<u4")
    meta.chunk_memory_layout = "C"
    offsets = [[3, 10], [5, 30], [4, 40], [2, 50], [7, 50], [30, 700], [1, 2], [4, 4], [12, 90]]
    counts = [[5, fast], [3, fast], [2, fast - 3], [6, fast], [4, 0], [3, fast - 5], [2, 2], [2, 2], [5, fast - 1]]
    steps = [[2, 3], [1, 0], [2, 1], [1, 1], [1, 2], [1, 3], [1, (1 << 32) - 10], [(1 << 40) + 1, 1], [3, 4]]
    good = [0, 2, 4, 8]
    B = len(offsets)
    g = lambda xs: [xs[b] for b in good]  # noqa: E731
    bound = bound_of(g(counts), 2)
    assert counts[3][0] == bound[0] + 1
    assert regions_s_waves(meta, g(offsets), g(counts), g(steps))[0] == 1
    lo, n = regions_s_grid(meta, g(offsets), g(counts), g(steps))  # box 5 lies outside
    assert lo[0] + n[0] <= 30 // 4
    slots = Slots(rng, meta, lo, n, 4, absent_frac=0.0)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    views = Views(counts, 4, "C", modes=(0,))
    src_h = rng.integers(0, 256, views.size, dtype=np.uint8)
    src = torch.from_numpy(src_h).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sb = sboxes_tensor(offsets, counts, steps, views.strides, views.bases(src))
    scatter_regions_s(meta, bound, 4, table, lo, n, sb, status)
    torch.cuda.synchronize()
    bad, uns, ok = _native.INVALID_INPUT, _native.UNSUPPORTED, _native.OK
    assert status.cpu().tolist() == [ok, bad, ok, bad, ok, bad, uns, uns, ok]
    chunks = slots.chunks()
    for b in good:
        apply_box(meta, "C", chunks, offsets[b], counts[b], steps[b], views.view(src_h, b, np.uint32))
    want = image_of(slots, chunks)
    assert not np.array_equal(want, slots.image)
    assert np.array_equal(slots.buf.cpu().numpy(), want)


def test_capture_and_replay_with_new_offsets_counts_steps_and_bases():
    """One captured zcg_write_regions_s call (one graph, no parallel branches),
    replayed twice with new offsets, sample counts, steps, strides and bases in
    d_boxes, all inside the bound: the kernels read them when they run.  Box b
    stays in its own band of rows, so the boxes of a call share no sample."""
    import torch
    rng = np.random.default_rng(26)
    shape, cs, bound = [50, 900], [7, 9], [4, 290]  # rows of 256 samples and more go a wave per row piece
    meta = ArrayMetadata.new(shape, cs, "<u2")
    meta.chunk_memory_layout = "C"
    B = 5

    def draw():
        counts = [[int(rng.integers(0, bound[0] + 1)), int(rng.choice([1, 11, 255, 256, 290]))] for _ in range(B)]
        steps = [[int(rng.choice([1, 2])), int(rng.choice([1, 2, 3]))] for _ in range(B)]
        offsets = [[10 * b + int(rng.integers(0, 3)), int(rng.integers(0, 30))] for b in range(B)]
        return offsets, counts, steps

    sets = [draw() for _ in range(3)]
    slots = Slots(rng, meta, [0, 0], [8, 100], 2)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    size = max(Views(s[1], 2, "C", shift=i).size for i, s in enumerate(sets))
    src_h = rng.integers(0, 256, size, dtype=np.uint8)
    src = torch.from_numpy(src_h).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(regions_s_scratch_bytes(B), dtype=torch.uint8, device=dev)
    v0 = Views(sets[0][1], 2, "C")
    sb = sboxes_tensor(sets[0][0], sets[0][1], sets[0][2], v0.strides, v0.bases(src))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        scatter_regions_s(meta, bound, 2, table, slots.lo, slots.n, sb, status, scratch=scratch)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        scatter_regions_s(meta, bound, 2, table, slots.lo, slots.n, sb, status, scratch=scratch)
    for i, (offsets, counts, steps) in enumerate(sets[1:], 1):
        assert regions_s_waves(meta, offsets, counts, steps)[0] == 1
        views = Views(counts, 2, "C", shift=i)
        sb.copy_(sboxes_tensor(offsets, counts, steps, views.strides, views.bases(src)))
        slots.reset()
        status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        chunks = slots.chunks()
        for b in range(B):
            apply_box(meta, "C", chunks, offsets[b], counts[b], steps[b], views.view(src_h, b, np.uint16))
        want = image_of(slots, chunks)
        assert not np.array_equal(want, slots.image)
        assert np.array_equal(slots.buf.cpu().numpy(), want), i


def test_assemble_returns_what_scatter_wrote():
    """Round trip for one mixed case without NULL slots: zcg_read_regions_s of
    the scattered slots, fill off, into a copy of the input buffer leaves that
    copy equal to the input in every box that no later box overwrites (a sample
    that lands nowhere keeps the copy's value, which is the input's)."""
    import torch
    C = Case(1, absent=0.0)
    C.run()
    assert C.status.cpu().tolist() == [_native.OK] * C.B
    out = C.src.clone()
    status = torch.full((C.B,), -1, dtype=torch.int32, device=C.dev)
    rb = sboxes_tensor(C.offsets, C.counts, C.steps, C.views.strides, C.views.bases(out))
    assemble_regions_s(C.meta, C.bound, C.es, C.table, C.lo, C.n, rb, status, False, 0)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK] * C.B
    got = out.cpu().numpy()
    pair = lambda a, b, xs: [xs[a], xs[b]]  # noqa: E731
    kept = [b for b in range(C.B)
            if all(regions_s_waves(C.meta, pair(b, c, C.offsets), pair(b, c, C.counts), pair(b, c, C.steps))[0] == 1
                   for c in range(b + 1, C.B))]
    assert len(kept) >= C.B // 2 and C.B - 1 in kept and 2 not in kept  # box 2 has a duplicate
    for b in kept:
        assert np.array_equal(C.views.view(got, b, C.dt), C.views.view(C.src_h, b, C.dt)), b
    assert not np.array_equal(C.views.view(got, 2, C.dt), C.views.view(C.src_h, 2, C.dt))


@pytest.mark.parametrize("seed", range(4))
def test_all_steps_one_is_byte_identical_to_write_regions_v(seed):
    """Pairwise disjoint dense boxes of the mixed shapes (test_gpu_boxes_v's
    band_boxes), element sizes 1/2/4/8, C and F order, ~25 % NULL slots: the
    slot buffer after zcg_write_regions_s with every step 1 equals the one
    zcg_write_regions_v leaves."""
    import torch
    rng = np.random.default_rng(53000 + seed)
    es = [1, 2, 4, 8][seed]
    order = "F" if seed % 2 else "C"
    rows = 4096 // ((3 * (16 // es) + 1) * es) + 7
    shape, offsets, shapes = band_boxes(rng, es, order, rows)
    cs = [61, 3] if order == "F" else [3, 61]
    meta = ArrayMetadata.new(shape, cs, TYPESTR[es])
    meta.chunk_memory_layout = order
    B = len(offsets)
    lo, n = regions_v_grid(meta, offsets, shapes)
    slots = Slots(rng, meta, lo, n, es)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    views = Views(shapes, es, order, shift=seed)
    src = torch.from_numpy(rng.integers(0, 256, views.size, dtype=np.uint8)).to(dev)
    images = []
    for strided in (False, True):
        slots.reset()
        status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if strided:
            bx = sboxes_tensor(offsets, shapes, [[1, 1]] * B, views.strides, views.bases(src))
            scatter_regions_s(meta, bound_of(shapes, 2), es, table, lo, n, bx, status)
        else:
            bx = vboxes_tensor(offsets, shapes, views.strides, views.bases(src))
            scatter_regions_v(meta, bound_of(shapes, 2), es, table, lo, n, bx, status)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [_native.OK] * B
        images.append(slots.buf.cpu().numpy())
    assert not np.array_equal(images[0], slots.image)
    assert np.array_equal(images[0], images[1]), seed


def test_trivial_calls():
    """n_boxes = 0 returns Ok and writes nothing; a zero bound writes every
    status word and no slot byte; a bound whose extent plus the chunk extent
    reaches 2^32 is Unsupported and nothing is launched."""
    import torch
    rng = np.random.default_rng(5)
    meta = ArrayMetadata.new([40, 50], [7, 9], "<u2")
    meta.chunk_memory_layout = "C"
    slots = Slots(rng, meta, [0, 0], [6, 6], 2)
    dev = slots.dev
    table = torch.from_numpy(slots.table()).to(dev)
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    scatter_regions_s(meta, [3, 3], 2, table, slots.lo, slots.n, None, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-1, -1]
    sb = sboxes_tensor([[1, 1], [2, 2]], [[0, 2], [1, 3]], [[2, 2], [1, 3]], [[3, 1], [3, 1]],
                       [src.data_ptr(), src.data_ptr() + 2048])
    scatter_regions_s(meta, [0, 3], 2, table, slots.lo, slots.n, sb, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_native.OK, _native.INVALID_INPUT]
    status.fill_(-1)
    with pytest.raises(_native.NativeUnavailable):
        scatter_regions_s(meta, [3, (1 << 32) - 8], 2, table, slots.lo, slots.n, sb, status)
    torch.cuda.synchronize()
    assert np.array_equal(slots.buf.cpu().numpy(), slots.image) and status.cpu().tolist() == [-1, -1]
