#!/usr/bin/env python3
"""Many bounding boxes, write direction: one zcg_write_regions launch against
a loop of zcg_write_region calls, and one write_ndarrays call against a loop of
write_ndarray calls.  The sibling of tools/boxes_bench.py, with its shapes.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  small_boxes  4 096 u16 chunk slots of 64^3 (2 GiB, a 1024^3 array), B in
               {1, 16, 256, 4096} boxes of 64^3 at random unaligned offsets,
               each from its own dense input:
               (a) B zcg_write_region calls on pre-built per-box sub-tables,
               (b) one zcg_write_regions on the shared table.
  long_rows    bench.py's region leg array (f32, 256x256x4 chunks, F order,
               1 GiB): eight boxes of [2000, 2000, 4], same (a) and (b).
  store        a gzip-6 u16 array of 64^3 chunks in a temporary store, 256
               boxes of 32^3 at random offsets (smaller than a chunk, so the
               boxes share chunks): one write_ndarrays call against 256
               write_ndarray calls; wall time and chunk encodes on each side.
Boxes of one (b) call overlap, so which box's value an element keeps is not
defined; the timing does not care.  The check that (b) writes what (a) writes
is made once per leg with inputs that are windows of one array image, so that
overlapping boxes carry equal values.  The device legs time with HIP events on
the launch stream after a warm-up of every shape, `--repeats` times alternating
(a) and (b) in one process, and report the median and the min..max spread of
each.  Writes profiles/boxes_write_bench.json.

usage: tools/boxes_write_bench.py [--repeats R] [--out FILE] [--legs small_boxes,long_rows,store]
"""
import argparse
import ctypes
import itertools
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxes_bench import stats, verdict  # noqa: E402

LIMITS = {"small_boxes": 300, "long_rows": 240, "store": 420}  # child time limits, seconds


def device_compare(meta, es, bshape, offsets, slots, grid, repeats, check):
    """(a) a zcg_write_region per box on its own sub-table, (b) one
    zcg_write_regions on the table of the whole grid; dense inputs."""
    import numpy as np
    import torch
    from zarr_amd import _native
    from zarr_amd.region import BoundingBox, _region, _strides, region_grid
    dev = torch.device("cuda", 0)
    ctx = _native.context(0)
    lib = ctx.lib
    nd = len(bshape)
    N = meta.get_chunk_num_elements()
    B = len(offsets)
    order = "F" if meta.chunk_memory_layout == "F" else "C"
    strides = _strides(bshape, order)
    box_bytes = int(np.prod(bshape)) * es
    gstr = [int(np.prod(grid[d + 1:])) for d in range(nd)]
    slots_ptr = slots.data_ptr()
    ptr_of = lambda c: slots_ptr + sum(ci * s for ci, s in zip(c, gstr)) * N * es  # noqa: E731
    table = torch.tensor([ptr_of(c) for c in itertools.product(*[range(g) for g in grid])], dtype=torch.int64,
                         device=dev)
    subs, sub_at = [], []
    for off in offsets:
        lo, n = region_grid(meta, BoundingBox(off, bshape))
        sub_at.append(sum(len(s) for s in subs))
        subs.append([ptr_of(c) for c in itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])])
    subtab = torch.tensor(list(itertools.chain(*subs)), dtype=torch.int64, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*grid)
    stream = torch.cuda.current_stream(dev)
    h = stream.cuda_stream

    def runners(in_strides, in_ptrs):
        regions = [_region(meta, BoundingBox(off, bshape), es, False, 0, in_strides) for off in offsets]
        shared = _region(meta, BoundingBox([0] * nd, bshape), es, False, 0, in_strides)
        recs = (_native.Box * B)()
        for b, off in enumerate(offsets):
            for d in range(nd):
                recs[b].offset[d] = off[d]
            recs[b].out = in_ptrs[b]
        boxes = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).to(dev)
        calls = [(ctypes.byref(regions[b]), subtab.data_ptr() + 8 * sub_at[b], in_ptrs[b]) for b in range(B)]

        def run_a():
            for r, t, p in calls:
                assert lib.zcg_write_region(ctx.handle, r, t, p, h) == 0

        def run_b():
            assert lib.zcg_write_regions(ctx.handle, ctypes.byref(shared), ctypes.addressof(tlo),
                                         ctypes.addressof(tn), table.data_ptr(), boxes.data_ptr(), B,
                                         status.data_ptr(), h) == 0
        return run_a, run_b, (regions, shared, boxes)

    if check:
        # inputs that are windows of one image of the whole array: overlapping boxes agree
        ashape = [g * c for g, c in zip(grid, meta.chunk_shape)]
        astr = _strides(ashape, order)
        image = torch.randint(0, 127, (int(np.prod(ashape)) * es,), dtype=torch.int8, device=dev).view(torch.uint8)
        ptrs = [image.data_ptr() + sum(o * s for o, s in zip(off, astr)) * es for off in offsets]
        run_a, run_b, keep = runners(astr, ptrs)
        orig = slots.clone()
        run_a()
        torch.cuda.synchronize()
        after_a = slots.clone()
        slots.copy_(orig)
        run_b()
        torch.cuda.synchronize()
        assert bool((status == 0).all()) and torch.equal(slots, after_a), "zcg_write_regions differs"
        assert not torch.equal(slots, orig)
        del image, orig, after_a, keep
        torch.cuda.empty_cache()

    src = torch.empty(B * box_bytes, dtype=torch.uint8, device=dev)
    src.view(torch.int32).copy_(torch.arange(B * box_bytes // 4, dtype=torch.int32, device=dev) * 40503)
    run_a, run_b, keep = runners(strides, [src.data_ptr() + b * box_bytes for b in range(B)])
    for _ in range(2):  # warm-up of this shape
        run_a()
        run_b()
    torch.cuda.synchronize()
    assert bool((status == 0).all())
    ms = {"a": [], "b": []}
    for _ in range(repeats):  # alternating, so drift hits both alike
        for name, fn in (("a", run_a), ("b", run_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    a, b = stats(ms["a"]), stats(ms["b"])
    gibs = lambda s: round(B * box_bytes / (s["median_ms"] * 1e-3) / 2**30, 1)  # noqa: E731
    return {"boxes": B, "box_bytes": box_bytes, "a_loop_of_write_region": a, "b_one_write_regions": b,
            "a_gib_s_of_box": gibs(a), "b_gib_s_of_box": gibs(b),
            "speedup_of_medians": round(a["median_ms"] / b["median_ms"], 3), "b_against_a": verdict(a, b),
            "checked_against_a": bool(check)}


def leg_small_boxes(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata
    meta = ArrayMetadata.new([1024] * 3, [64] * 3, "<u2")
    meta.chunk_memory_layout = "C"
    dev = torch.device("cuda", 0)
    nbytes = 4096 * 64 ** 3 * 2
    slots = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    slots.view(torch.int32).copy_(torch.arange(nbytes // 4, dtype=torch.int32, device=dev) * 2654435)
    rng = np.random.default_rng(1)
    res = {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); boxes of 64^3 at random unaligned "
                       "offsets, dense inputs; GiB/s of box bytes (traffic is twice that)", "repeats": repeats,
           "by_boxes": {}}
    for B in (1, 16, 256, 4096):
        offsets = [[int(x) for x in rng.integers(1, 1024 - 64, 3)] for _ in range(B)]
        res["by_boxes"][str(B)] = device_compare(meta, 2, [64] * 3, offsets, slots, [16] * 3, repeats, B == 256)
        torch.cuda.empty_cache()
    return res


def leg_long_rows(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata
    meta = ArrayMetadata.new([256 * 32, 256 * 32, 4], [256, 256, 4], "<f4")  # bench.py's region leg (F order)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    slots = torch.randint(-2**31, 2**31 - 1, (1024 * 256 * 256 * 4,), dtype=torch.int32, device=dev,
                          generator=g).view(torch.uint8)
    rng = np.random.default_rng(2)
    offsets = [[int(rng.integers(1, 8192 - 2000)), int(rng.integers(1, 8192 - 2000)), 0] for _ in range(8)]
    r = device_compare(meta, 4, [2000, 2000, 4], offsets, slots, [32, 32, 1], repeats, True)
    r["workload"] = ("1024 f32 slots of 256x256x4 (1 GiB, F order: bench.py's region leg); eight boxes of "
                     "[2000, 2000, 4] at random unaligned offsets")
    r["repeats"] = repeats
    return r


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import BoundingBox, read_ndarrays, region_grid, write_ndarray, write_ndarrays
    meta = ArrayMetadata.new([256] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    offsets = [[int(v) for v in rng.integers(0, 256 - 32, 3)] for _ in range(256)]
    arrays = (full[:32, :32, :32][None] + np.arange(256, dtype=np.uint16)[:, None, None, None]).astype(np.uint16)
    want = full.copy()
    for off, a in zip(offsets, arrays):
        want[tuple(slice(o, o + 32) for o in off)] = a
    visited = [set(itertools.product(*[range(a, a + k) for a, k in zip(*region_grid(meta, BoundingBox(o, [32] * 3)))]))
               for o in offsets]
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(4), repeat=3)])

        def whole():
            return read_ndarrays(h, "a", meta, [[0, 0, 0]], [256] * 3, np.uint16)[0]

        # warm-up: both paths, and both must leave the array "later box wins" gives
        write_ndarrays(h, "a", meta, offsets, arrays)
        assert np.array_equal(whole(), want)
        for off, a in zip(offsets, arrays):
            write_ndarray(h, "a", meta, off, a)
        assert np.array_equal(whole(), want)
        wall = {"loop": [], "one": []}
        for _ in range(repeats):
            t0 = time.perf_counter()
            for off, a in zip(offsets, arrays):
                write_ndarray(h, "a", meta, off, a)
            wall["loop"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            write_ndarrays(h, "a", meta, offsets, arrays)
            wall["one"].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        assert np.array_equal(whole(), want)
    a, b = stats(wall["loop"]), stats(wall["one"])
    return {"workload": "gzip-6 u16 array 256^3 in 64 chunks of 64^3 (temporary store); 256 boxes of 32^3 at random "
                        "offsets, from host arrays", "repeats": repeats,
            "loop_of_256_write_ndarray": dict(a, chunk_encodes=sum(len(v) for v in visited)),
            "one_write_ndarrays": dict(b, chunk_encodes=len(set().union(*visited))),
            "speedup_of_medians": round(a["median_ms"] / b["median_ms"], 2)}


LEGS = {"small_boxes": leg_small_boxes, "long_rows": leg_long_rows, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_write_bench.json"))
    ap.add_argument("--legs", default="small_boxes,long_rows,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/boxes_write_bench.py", "legs": {}}
    for name in args.legs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats",
                                str(args.repeats)], capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result inside {LIMITS[name]} s; stopping", file=sys.stderr)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{name}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res["legs"][name] = json.loads(line[-1][7:])
        print(name, json.dumps(res["legs"][name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
