#!/usr/bin/env python3
"""Many bounding boxes: one zcg_read_regions launch against a loop of
zcg_read_region calls, and one read_ndarrays call against a loop of
read_ndarray calls.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  small_boxes  4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array),
               B in {1, 16, 256, 4096} boxes of 64^3 at random unaligned
               offsets, each into its own output (2 GiB of outputs at B = 4096):
               (a) B zcg_read_region calls on pre-built per-box sub-tables,
               (b) one zcg_read_regions on the shared table.
  long_rows    bench.py's region leg array (f32, 256x256x4 chunks, F order,
               1 GiB): eight boxes of [2000, 2000, 4], same (a) and (b).
  store        a gzip-6 u16 array of 64^3 chunks in a temporary store, 256
               overlapping 64^3 boxes: one read_ndarrays call against 256
               read_ndarray calls; wall time and chunk decodes on each side.
The device legs time with HIP events on the launch stream after a warm-up of
every shape, `--repeats` times alternating (a) and (b) in one process, and
report the median and the min..max spread of each; (b)'s boxes are checked
against (a)'s once.  Writes profiles/boxes_bench.json.

usage: tools/boxes_bench.py [--repeats R] [--out FILE] [--legs small_boxes,long_rows,store]
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
LIMITS = {"small_boxes": 300, "long_rows": 240, "store": 300}  # child time limits, seconds


def stats(ms):
    import numpy as np
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def verdict(a, b):
    """(b) against (a): faster beyond the spread, within it, or slower beyond it."""
    if b["max_ms"] < a["min_ms"]:
        return "faster"
    if b["min_ms"] > a["max_ms"]:
        return "slower"
    return "within spread"


def device_compare(meta, es, bshape, offsets, slots_ptr, grid, repeats):
    """(a) a zcg_read_region per box on its own sub-table, (b) one
    zcg_read_regions on the table of the whole grid; both fill, unit strides."""
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
    ptr_of = lambda c: slots_ptr + sum(ci * s for ci, s in zip(c, gstr)) * N * es  # noqa: E731
    table = torch.tensor([ptr_of(c) for c in itertools.product(*[range(g) for g in grid])], dtype=torch.int64,
                         device=dev)
    subs, regions, sub_at = [], [], []
    for off in offsets:
        bb = BoundingBox(off, bshape)
        lo, n = region_grid(meta, bb)
        sub_at.append(sum(len(s) for s in subs))
        subs.append([ptr_of(c) for c in itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])])
        regions.append(_region(meta, bb, es, True, 0, strides))
    subtab = torch.tensor(list(itertools.chain(*subs)), dtype=torch.int64, device=dev)
    out_a = torch.empty(B * box_bytes, dtype=torch.uint8, device=dev)
    out_b = torch.empty(B * box_bytes, dtype=torch.uint8, device=dev)
    recs = (_native.Box * B)()
    for b, off in enumerate(offsets):
        for d in range(nd):
            recs[b].offset[d] = off[d]
        recs[b].out = out_b.data_ptr() + b * box_bytes
    boxes = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).to(dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    shared = _region(meta, BoundingBox([0] * nd, bshape), es, True, 0, strides)
    tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*grid)
    stream = torch.cuda.current_stream(dev)
    h = stream.cuda_stream
    calls_a = [(ctypes.byref(regions[b]), subtab.data_ptr() + 8 * sub_at[b], out_a.data_ptr() + b * box_bytes)
               for b in range(B)]

    def run_a():
        for r, t, o in calls_a:
            assert lib.zcg_read_region(ctx.handle, r, t, o, h) == 0

    def run_b():
        assert lib.zcg_read_regions(ctx.handle, ctypes.byref(shared), ctypes.addressof(tlo), ctypes.addressof(tn),
                                    table.data_ptr(), boxes.data_ptr(), B, status.data_ptr(), h) == 0

    for _ in range(2):  # warm-up of this shape, and (b) must write what (a) writes
        run_a()
        run_b()
    torch.cuda.synchronize()
    assert bool((status == 0).all()) and torch.equal(out_a, out_b), "zcg_read_regions differs from zcg_read_region"
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
    gbs = lambda s: round(2 * B * box_bytes / (s["median_ms"] * 1e-3) / 1e9, 1)  # noqa: E731
    return {"boxes": B, "box_bytes": box_bytes, "a_loop_of_read_region": a, "b_one_read_regions": b,
            "a_gb_s_read_plus_written": gbs(a), "b_gb_s_read_plus_written": gbs(b),
            "speedup_of_medians": round(a["median_ms"] / b["median_ms"], 3), "b_against_a": verdict(a, b)}


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
                       "offsets, fill, dense outputs", "repeats": repeats, "by_boxes": {}}
    for B in (1, 16, 256, 4096):
        offsets = [[int(x) for x in rng.integers(1, 1024 - 64, 3)] for _ in range(B)]
        res["by_boxes"][str(B)] = device_compare(meta, 2, [64] * 3, offsets, slots.data_ptr(), [16] * 3, repeats)
        torch.cuda.empty_cache()
    return res


def leg_long_rows(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata
    meta = ArrayMetadata.new([256 * 32, 256 * 32, 4], [256, 256, 4], "<f4")  # bench.py's region leg (F order)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    slots = torch.randint(-2**31, 2**31 - 1, (1024 * 256 * 256 * 4,), dtype=torch.int32, device=dev, generator=g)
    rng = np.random.default_rng(2)
    offsets = [[int(rng.integers(1, 8192 - 2000)), int(rng.integers(1, 8192 - 2000)), 0] for _ in range(8)]
    r = device_compare(meta, 4, [2000, 2000, 4], offsets, slots.data_ptr(), [32, 32, 1], repeats)
    r["workload"] = ("1024 f32 slots of 256x256x4 (1 GiB, F order: bench.py's region leg); eight boxes of "
                     "[2000, 2000, 4] at random unaligned offsets")
    r["repeats"] = repeats
    return r


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import BoundingBox, read_ndarray, read_ndarrays, region_grid
    meta = ArrayMetadata.new([256] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    offsets = [[int(v) for v in rng.integers(0, 256 - 64, 3)] for _ in range(256)]
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(4), repeat=3)])
        visited = [set(itertools.product(*[range(a, a + k) for a, k in zip(*region_grid(meta, BoundingBox(o, [64] * 3)))]))
                   for o in offsets]
        want = np.stack([full[tuple(slice(o, o + 64) for o in off)] for off in offsets])
        # warm-up: both paths, and both must read the array's values
        assert np.array_equal(read_ndarrays(h, "a", meta, offsets, [64] * 3, np.uint16), want)
        assert np.array_equal(read_ndarray(h, "a", meta, BoundingBox(offsets[0], [64] * 3), np.uint16), want[0])
        wall = {"loop": [], "one": []}
        for _ in range(repeats):
            t0 = time.perf_counter()
            for off in offsets:
                read_ndarray(h, "a", meta, BoundingBox(off, [64] * 3), np.uint16)
            wall["loop"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            read_ndarrays(h, "a", meta, offsets, [64] * 3, np.uint16)
            wall["one"].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    a, b = stats(wall["loop"]), stats(wall["one"])
    return {"workload": "gzip-6 u16 array 256^3 in 64 chunks of 64^3 (temporary store); 256 overlapping boxes of "
                        "64^3 at random offsets, read to host arrays", "repeats": repeats,
            "loop_of_256_read_ndarray": dict(a, chunk_decodes=sum(len(v) for v in visited)),
            "one_read_ndarrays": dict(b, chunk_decodes=len(set().union(*visited))),
            "speedup_of_medians": round(a["median_ms"] / b["median_ms"], 2)}


LEGS = {"small_boxes": leg_small_boxes, "long_rows": leg_long_rows, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_bench.json"))
    ap.add_argument("--legs", default="small_boxes,long_rows,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/boxes_bench.py", "legs": {}}
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
