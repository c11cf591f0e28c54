"""write_ndarrays_s (zcg_store_write_boxes_s[_device]): many strided boxes
written to a store in one native call, against the oracle's model applied box
by box in order — read_ndarray of the hull (filled), the samples overlaid,
write_ndarray of the hull, kept for the chunks that hold a sample
(oracle/region_ref.py).  Only those chunks are read, encoded and written."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_ref  # noqa: E402  (oracle: checker only)

from test_gpu_boxes_s_store import hull_of, touched_chunks  # noqa: E402
from test_gpu_write_boxes import check_store_equals, chunk_files, copy_store, snapshot, truncate  # noqa: E402
from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, Raw, SliceDataChunk  # noqa: E402
from zarr_amd.chunk import ZarrIOError  # noqa: E402
from zarr_amd.region import BoundingBox, read_ndarrays_v, write_ndarrays_s, write_ndarrays_v  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, CS, FILL = [18, 20, 24], [4, 6, 8], 9  # u16 chunks of 384 bytes; edge chunks overhang in two dimensions
GRID = [5, 4, 3]


def tiny_store(root, comp, absent_frac=0.25, seed=0):
    meta = ArrayMetadata.new(SHAPE, CS, "<u2", comp)
    meta.chunk_memory_layout = "C"
    meta.fill_value = FILL
    h = FilesystemHierarchy.open_or_create(str(root))
    h.create_array("a", meta)
    rng = np.random.default_rng(640 + seed)
    chunks = {}
    for c in itertools.product(*[range(g) for g in GRID]):
        if rng.random() >= absent_frac:
            chunks[c] = rng.integers(0, 60000, int(np.prod(CS))).astype(np.uint16)
    h.write_chunks("a", meta, [SliceDataChunk(list(c), d) for c, d in chunks.items()])
    return rng, h, meta, chunks


def apply_box(meta, want, off, counts, steps, array):
    """The model for one box on the dict coord -> chunk elements: touched
    chunks that are absent appear (fill around the samples), untouched ones
    are left as they are."""
    if 0 in counts:
        return
    H = region_ref.read_ndarray(meta.shape, meta.chunk_shape, "C", off, hull_of(counts, steps), want.get, np.uint16,
                                FILL)
    H[tuple(slice(None, None, int(s)) for s in steps)] = array
    tmp = dict(want)
    region_ref.write_ndarray(meta.shape, meta.chunk_shape, "C", off, H, tmp, FILL)
    for c in touched_chunks(meta, off, counts, steps):
        want[c] = tmp[c]


def draw_boxes(rng, meta, B):
    """B strided boxes (0-5 samples per dimension; steps 1, 2, 3, the chunk
    extent, that plus 1 and twice that plus 1), partly outside the array and
    overlapping, every touched chunk inside the array's chunk grid."""
    offsets, counts, steps = [], [], []
    while len(offsets) < B:
        off = [int(rng.integers(0, s + 3)) for s in meta.shape]
        cnt = [int(rng.integers(0 if len(offsets) % 5 == 3 else 1, 6)) for _ in meta.shape]
        stp = [int(rng.choice([1, 1, 2, 3, c, c + 1, 2 * c + 1])) for c in meta.chunk_shape]
        if all(meta.in_bounds(c) for c in touched_chunks(meta, off, cnt, stp)):
            offsets.append(off)
            counts.append(cnt)
            steps.append(stp)
    return offsets, counts, steps


def whole_array(h, meta):
    return read_ndarrays_v(h, "a", meta, [BoundingBox([0, 0, 0], SHAPE)], np.uint16)[0]


def array_of(meta, chunks):
    return region_ref.read_ndarray(meta.shape, meta.chunk_shape, "C", [0, 0, 0], SHAPE, chunks.get, np.uint16, FILL)


@pytest.mark.parametrize("comp", [Gzip(6), Raw()], ids=["gzip", "raw"])
def test_write_ndarrays_s_vs_the_model_box_by_box(tmp_path, comp):
    """24 overlapping strided boxes on a store with ~25 % absent chunks: the
    chunk files are the model's key set (absent touched chunks appear, absent
    untouched ones stay absent), every file decodes to the model's chunk, the
    whole array read back by read_ndarrays_v is the model's, and the files of
    untouched chunks keep their bytes.  A slot budget of two chunks (several
    groups that share chunks) and device tensors with strides of their own
    leave the same files."""
    import torch
    rng, h0, meta, chunks = tiny_store(tmp_path / "s0", comp)
    B = 24
    offsets, counts, steps = draw_boxes(rng, meta, B)
    arrays = [rng.integers(0, 60000, cnt).astype(np.uint16) for cnt in counts]
    want = {c: v.copy() for c, v in chunks.items()}
    for b in range(B):
        apply_box(meta, want, offsets[b], counts[b], steps[b], arrays[b])
    touched = {c for b in range(B) for c in touched_chunks(meta, offsets[b], counts[b], steps[b])}
    assert set(want) - set(chunks) and set(want) - touched  # some chunks appear, some stay untouched
    before = chunk_files(tmp_path / "s0")

    ha = copy_store(tmp_path / "s0", tmp_path / "a")
    write_ndarrays_s(ha, "a", meta, offsets, steps, arrays)
    check_store_equals(ha, tmp_path / "a", meta, np.dtype(np.uint16), want)
    assert np.array_equal(whole_array(ha, meta), array_of(meta, want))
    files = chunk_files(tmp_path / "a")
    for c in set(chunks) - touched:
        k = os.path.relpath(ha.chunk_path("a", meta, list(c)), str(tmp_path / "a"))
        assert files[k] == before[k], c

    hc = copy_store(tmp_path / "s0", tmp_path / "c")
    write_ndarrays_s(hc, "a", meta, offsets, steps, arrays, slot_budget_bytes=2 * int(np.prod(CS)) * 2)
    assert chunk_files(tmp_path / "c") == files

    hd = copy_store(tmp_path / "s0", tmp_path / "d")
    dev = torch.device("cuda", 0)
    tensors = []
    for b, a in enumerate(arrays):
        wide = torch.zeros([2 * max(k, 1) for k in a.shape], dtype=torch.int16, device=dev)
        view = wide[tuple(slice(b % 2, b % 2 + 2 * k, 2) for k in a.shape)]  # every other element of a larger buffer
        view.copy_(torch.from_numpy(a.view(np.int16)).to(dev))
        tensors.append(view)
    write_ndarrays_s(hd, "a", meta, offsets, steps, tensors)
    assert chunk_files(tmp_path / "d") == files


def test_untouched_covered_and_absent_chunks(tmp_path):
    """One call on a gzip store.  Box 0 (2 x 2 x 2 samples at twice the chunk
    extent) touches 8 chunks of the 27 in its hull's range: the touched chunk
    [2, 2, 2] is absent and appears with fill around its sample; of the
    untouched ones [1, 0, 0] is absent and stays so, and [1, 1, 0] is corrupt
    and keeps its bytes.  Box 1 (4 x 6 x 8 samples at step 1, exactly chunk
    [3, 2, 1]) covers its chunk, whose corrupt old file is never read."""
    rng, h, meta, chunks = tiny_store(tmp_path, Gzip(6), absent_frac=0.0)
    for c in ((2, 2, 2), (1, 0, 0)):
        os.remove(h.chunk_path("a", meta, list(c)))
        del chunks[c]
    truncate(h.chunk_path("a", meta, [1, 1, 0]))
    truncate(h.chunk_path("a", meta, [3, 2, 1]))
    before = chunk_files(tmp_path)
    offsets = [[1, 2, 3], [12, 12, 8]]
    counts = [[2, 2, 2], [4, 6, 8]]
    steps = [[8, 12, 16], [1, 1, 1]]
    arrays = [rng.integers(0, 60000, cnt).astype(np.uint16) for cnt in counts]
    t0 = set(touched_chunks(meta, offsets[0], counts[0], steps[0]))
    assert t0 == set(itertools.product((0, 2), (0, 2), (0, 2)))
    assert (1, 1, 0) not in t0 and (1, 0, 0) not in t0
    want = {c: v.copy() for c, v in chunks.items()}
    for b in range(2):
        apply_box(meta, want, offsets[b], counts[b], steps[b], arrays[b])
    write_ndarrays_s(h, "a", meta, offsets, steps, arrays)
    files = chunk_files(tmp_path)
    rel = lambda c: os.path.relpath(h.chunk_path("a", meta, list(c)), str(tmp_path))  # noqa: E731
    assert rel((1, 0, 0)) not in files
    assert files[rel((1, 1, 0))] == before[rel((1, 1, 0))]  # corrupt, untouched, not rewritten
    assert sorted(want) == sorted(set(chunks) | {(2, 2, 2)}) and (want[(2, 2, 2)] == FILL).sum() == 4 * 6 * 8 - 1
    for c in set(chunks) - t0 - {(3, 2, 1)}:
        assert files[rel(c)] == before[rel(c)], c
    # the touched and the covered chunks decode to the model's
    keys = sorted(t0 | {(3, 2, 1)})
    got = h.read_chunks("a", meta, [list(c) for c in keys], np.uint16)
    for c, ch in zip(keys, got):
        assert ch is not None and np.array_equal(np.asarray(ch.get_data()), want[c]), c
    assert np.array_equal(want[(3, 2, 1)], arrays[1].reshape(-1))


def test_absent_touched_chunk_appears_with_fill_around_the_samples(tmp_path):
    rng, h, meta, chunks = tiny_store(tmp_path, Gzip(6), absent_frac=0.0)
    os.remove(h.chunk_path("a", meta, [2, 1, 2]))
    off, cnt, stp = [8, 7, 17], [2, 3, 3], [3, 2, 2]  # all inside chunk [2, 1, 2]
    assert touched_chunks(meta, off, cnt, stp) == [(2, 1, 2)]
    a = rng.integers(100, 60000, cnt).astype(np.uint16)
    write_ndarrays_s(h, "a", meta, [off], stp, [a])
    ch = np.asarray(h.read_chunk("a", meta, [2, 1, 2], np.uint16).get_data()).reshape(CS)
    assert np.array_equal(ch[0:4:3, 1:6:2, 1:6:2], a)
    assert (ch == FILL).sum() == ch.size - a.size


def test_corrupt_touched_chunk_that_is_not_covered_raises_and_writes_nothing(tmp_path):
    """Chunk [0, 2, 1] holds one sample of the box: it is read first, its
    decode status is returned, zcg_last_error names it and no file changes."""
    rng, h, meta, chunks = tiny_store(tmp_path, Gzip(6), absent_frac=0.0)
    truncate(h.chunk_path("a", meta, [0, 2, 1]))
    with pytest.raises(ZarrIOError) as single:  # the status the chunk has on its own
        h.read_chunk("a", meta, [0, 2, 1], np.uint16)
    before = snapshot(tmp_path)
    off, cnt, stp = [1, 2, 3], [2, 2, 2], [8, 12, 8]
    assert (0, 2, 1) in touched_chunks(meta, off, cnt, stp)
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays_s(h, "a", meta, [[0, 0, 0], off], [[1, 1, 1], stp],
                         [np.ones((2, 2, 2), np.uint16), np.ones(cnt, np.uint16)])
    assert ei.value.kind == single.value.kind and "chunk [0, 2, 1]" in str(ei.value)
    assert snapshot(tmp_path) == before


def test_a_later_box_wins_and_interleaved_boxes_both_land(tmp_path):
    """Even and odd planes of the whole array in one call land completely; a
    third box over the even planes' samples wins them."""
    rng, h, meta, chunks = tiny_store(tmp_path, Raw(), absent_frac=0.25)
    even = rng.integers(0, 60000, (9, 20, 24)).astype(np.uint16)
    odd = rng.integers(0, 60000, (9, 20, 24)).astype(np.uint16)
    write_ndarrays_s(h, "a", meta, [[0, 0, 0], [1, 0, 0]], [2, 1, 1], [even, odd])
    got = whole_array(h, meta)
    assert np.array_equal(got[0::2], even) and np.array_equal(got[1::2], odd)
    later = rng.integers(0, 60000, (9, 20, 24)).astype(np.uint16)
    part = rng.integers(0, 60000, (3, 5, 4)).astype(np.uint16)
    write_ndarrays_s(h, "a", meta, [[0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 1, 3]],
                     [[2, 1, 1], [2, 1, 1], [2, 1, 1], [4, 3, 5]], [even, odd, later, part])
    got = whole_array(h, meta)
    want = np.empty(SHAPE, np.uint16)
    want[0::2], want[1::2] = later, odd
    want[2:11:4, 1:14:3, 3:19:5] = part
    assert np.array_equal(got, want)


def test_a_small_slot_budget_splits_the_call_into_groups_that_share_chunks(tmp_path):
    """A budget of two chunks: 12 boxes along one row of chunks, each touching
    two neighbouring chunks, run in at least three groups, each chunk shared
    with the next group; the store equals the one a single group leaves, and
    the model."""
    rng, h0, meta, chunks = tiny_store(tmp_path / "s0", Gzip(6))
    offsets = [[3 * (b % 5), 4, 6] for b in range(12)]
    counts = [[3, 2, 2]] * 12
    steps = [[2, 3, 2]] * 12
    arrays = [rng.integers(0, 60000, (3, 2, 2)).astype(np.uint16) for _ in range(12)]
    per_box = [set(touched_chunks(meta, o, c, s)) for o, c, s in zip(offsets, counts, steps)]
    assert all(len(t) >= 2 for t in per_box) and len(set().union(*per_box)) >= 6
    # the planner's greedy grouping, restated: a box that would take the group's unique chunks above
    # the budget (two chunks) starts the next group; a box alone may exceed it
    groups, seen = [[]], set()
    for b, t in enumerate(per_box):
        if groups[-1] and len(seen | t) > 2:
            groups.append([])
            seen = set()
        groups[-1].append(b)
        seen |= t
    union = [set().union(*[per_box[b] for b in g]) for g in groups]
    assert len(groups) >= 3 and sum(1 for u, v in zip(union, union[1:]) if u & v) >= 2
    want = {c: v.copy() for c, v in chunks.items()}
    for b in range(12):
        apply_box(meta, want, offsets[b], counts[b], steps[b], arrays[b])
    ha = copy_store(tmp_path / "s0", tmp_path / "a")
    write_ndarrays_s(ha, "a", meta, offsets, steps, arrays)
    hb = copy_store(tmp_path / "s0", tmp_path / "b")
    write_ndarrays_s(hb, "a", meta, offsets, steps, arrays, slot_budget_bytes=2 * int(np.prod(CS)) * 2)
    assert chunk_files(tmp_path / "a") == chunk_files(tmp_path / "b")
    check_store_equals(hb, tmp_path / "b", meta, np.dtype(np.uint16), want)


def test_all_steps_one_equals_write_ndarrays_v(tmp_path):
    """Dense boxes through both calls leave byte-identical files (the strided
    call takes the _v plan and kernels)."""
    rng, h0, meta, chunks = tiny_store(tmp_path / "s0", Gzip(6))
    offsets = [[0, 0, 0], [3, 5, 7], [10, 2, 15], [16, 18, 20]]
    arrays = [rng.integers(0, 60000, s).astype(np.uint16) for s in ([4, 6, 8], [5, 7, 9], [6, 1, 3], [4, 4, 5])]
    ha = copy_store(tmp_path / "s0", tmp_path / "a")
    write_ndarrays_v(ha, "a", meta, offsets, arrays)
    hb = copy_store(tmp_path / "s0", tmp_path / "b")
    write_ndarrays_s(hb, "a", meta, offsets, [1, 1, 1], arrays)
    assert chunk_files(tmp_path / "a") == chunk_files(tmp_path / "b")
    assert chunk_files(tmp_path / "a") != chunk_files(tmp_path / "s0")


def test_argument_errors_with_a_context_touch_no_file(tmp_path):
    """A touched chunk outside the array's chunk grid is InvalidInput before
    any file is touched; an untouched chunk of the hull's range out there is
    no error."""
    rng, h, meta, chunks = tiny_store(tmp_path, Gzip(6))
    before = snapshot(tmp_path)
    one = np.ones((2, 1, 1), np.uint16)
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays_s(h, "a", meta, [[0, 0, 0], [21, 0, 0]], [[1, 1, 1], [3, 1, 1]], [one, one])  # chunks 0 .. 4
    assert ei.value.kind == "InvalidInput" and "chunk [5, 0, 0]" in str(ei.value)
    with pytest.raises(ZarrIOError) as ei:
        write_ndarrays_s(h, "a", meta, [[0, 0, 0]], [[0, 1, 1]], [one])
    assert ei.value.kind == "InvalidInput"
    assert snapshot(tmp_path) == before
    write_ndarrays_s(h, "a", meta, [[21, 0, 0]], [[3, 1, 1]], [np.ones((0, 1, 1), np.uint16)])  # no sample
    assert snapshot(tmp_path) == before


def test_plain_c_caller_writes_and_reads_back_two_strided_boxes(tmp_path):
    """tests/c_abi_sw/boxes_sw_c.c, built by its own Makefile, on a copy of the
    zarrita fixture: two boxes of 2x2x3 samples written with one
    zcg_store_write_boxes_s call and read back with zcg_store_read_boxes_s."""
    from golden_util import zarrita_chunks
    from zarr_amd.region import read_ndarrays_s
    c_abi = os.path.join(ROOT, "tests", "c_abi_sw")
    r = subprocess.run(["make", "-s", "-C", c_abi], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(c_abi, "boxes_sw_c")
    store = str(tmp_path / "zarrita")
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "zarrita"), store)
    outf = str(tmp_path / "boxes.bin")
    r = subprocess.run([exe, store, outf, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "boxes_sw_c: ok (2 boxes, 1 wave)" in r.stdout, (r.stdout, r.stderr)
    back = np.fromfile(outf, "<i2").reshape(2, 2, 2, 3)
    chunks = {g: v for g, _, v in zarrita_chunks()}
    full = region_ref.read_ndarray([4, 5, 6], [2, 3, 4], "C", [0, 0, 0], [4, 5, 6], chunks.get, np.int16, 0)
    want = full.copy()
    boxes = (([0, 1, 0], [2, 3, 2]), ([2, 0, 1], [1, 2, 2]))
    for b, (off, stp) in enumerate(boxes):
        vals = (-1000 * (b + 1) - np.arange(12)).astype(np.int16).reshape(2, 2, 3)
        assert np.array_equal(back[b], vals)
        want[tuple(slice(o, o + (c - 1) * s + 1, s) for o, c, s in zip(off, [2, 2, 3], stp))] = vals
    h = FilesystemHierarchy.open(store)
    meta = h.get_array_metadata("/seq/i2")
    got = read_ndarrays_s(h, "/seq/i2", meta, [BoundingBox([0, 0, 0], [4, 5, 6])], [1, 1, 1], np.int16)[0]
    assert np.array_equal(got, want) and not np.array_equal(want, full)
