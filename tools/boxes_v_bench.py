#!/usr/bin/env python3
"""Many bounding boxes of differing shapes: one zcg_read_regions_v /
zcg_write_regions_v call against the loop of zcg_read_region / zcg_write_region
calls it replaces, and one read_ndarrays_v / write_ndarrays_v call against a
loop of read_ndarray / write_ndarray calls.  The method is tools/boxes_bench.py's.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  mixed    4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array), B in
           {16, 256, 4096} boxes with extents drawn from {8, 16, 32, 64, 96}^3 at
           random unaligned offsets, each dense into its own buffer: (a) B
           single-box calls on pre-built per-box sub-tables, (b) one _v call on
           the shared table; read and write direction.
  skew     one 256^3 box plus 4 095 boxes of 8^3: (a) and (b) as above, and the
           _v call on each of the two sub-lists alone.
  uniform  boxes of 64^3, B in {1, 16, 256, 4096}: zcg_read_regions (a) against
           zcg_read_regions_v (b); the ratio is the price of the plan launch and
           the unit search.
  store    a gzip-6 u16 array of 64^3 chunks in a temporary store, 256
           overlapping boxes of mixed shapes: one read_ndarrays_v against 256
           read_ndarray calls, one write_ndarrays_v against 256 write_ndarray
           calls; wall time and chunk decodes / encodes on each side.
The device legs time with HIP events on the launch stream after a warm-up,
`--repeats` times alternating the sides in one process, and report the median
and the min..max spread of each.  Writes profiles/boxes_v_bench.json.

The store leg runs 3 repeats at the most (its loop sides take 5 s per repeat)
unless --uncapped is given.

usage: tools/boxes_v_bench.py [--repeats R] [--out FILE] [--legs mixed,skew,uniform,store] [--uncapped]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from boxes_bench import stats, verdict  # noqa: E402

LIMITS = {"mixed": 420, "skew": 300, "uniform": 300, "store": 420}  # child time limits, seconds
GRID = [16] * 3


def alternate(sides, repeats, stream):
    """{name: fn} -> {name: stats}, HIP events, the sides alternating."""
    import torch
    ms = {k: [] for k in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ms.items()}


class Slots:
    """bench.py's small-box workload: 4 096 u16 slots of 64^3 over a 16^3 grid."""

    def __init__(self):
        import torch
        from zarr_amd import ArrayMetadata
        self.meta = ArrayMetadata.new([1024] * 3, [64] * 3, "<u2")
        self.meta.chunk_memory_layout = "C"
        self.dev = torch.device("cuda", 0)
        nbytes = 4096 * 64 ** 3 * 2
        self.slots = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.slots.view(torch.int32).copy_(torch.arange(nbytes // 4, dtype=torch.int32, device=self.dev) * 2654435)
        self.N = 64 ** 3
        self.gstr = [256, 16, 1]
        self.table = torch.tensor([self.ptr_of(c) for c in itertools.product(*[range(g) for g in GRID])],
                                  dtype=torch.int64, device=self.dev)

    def ptr_of(self, c):
        return self.slots.data_ptr() + sum(ci * s for ci, s in zip(c, self.gstr)) * self.N * 2


class Calls:
    """The two sides for one box list: single-box calls on per-box sub-tables
    and the _v call on the shared table, both directions."""

    def __init__(self, S, offsets, shapes):
        import numpy as np
        import torch
        from zarr_amd import _native
        from zarr_amd.region import BoundingBox, _region, _strides, region_grid, vboxes_tensor
        self.ctx = _native.context(0)
        self.lib = self.ctx.lib
        self.S, self.B = S, len(offsets)
        meta, dev = S.meta, S.dev
        at = [0]
        for shp in shapes:
            at.append(at[-1] + int(np.prod(shp)) * 2)
        self.bytes = at[-1]
        subs, self.regions, sub_at = [], [], []
        strides = [_strides(shp, "C") for shp in shapes]
        for off, shp, st in zip(offsets, shapes, strides):
            bb = BoundingBox(off, shp)
            lo, n = region_grid(meta, bb)
            sub_at.append(sum(len(s) for s in subs))
            subs.append([S.ptr_of(c) for c in itertools.product(*[range(a, a + k) for a, k in zip(lo, n)])])
            self.regions.append(_region(meta, bb, 2, True, 0, st))
        self.subtab = torch.tensor(list(itertools.chain(*subs)), dtype=torch.int64, device=dev)
        self.out_a = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        self.out_b = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        self.vb = vboxes_tensor(offsets, shapes, strides, [self.out_b.data_ptr() + a for a in at[:-1]])
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(self.lib.zcg_regions_v_scratch_bytes(self.B), dtype=torch.uint8, device=dev)
        bound = [max(s[d] for s in shapes) for d in range(3)]
        self.shared = _region(meta, BoundingBox([0] * 3, bound), 2, True, 0, [0] * 3)
        self.tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
        self.tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*GRID)
        self.stream = torch.cuda.current_stream(dev)
        self.h = self.stream.cuda_stream
        self.calls = [(ctypes.byref(self.regions[b]), self.subtab.data_ptr() + 8 * sub_at[b],
                       self.out_a.data_ptr() + at[b]) for b in range(self.B)]

    def loop(self, write=False):
        fn = self.lib.zcg_write_region if write else self.lib.zcg_read_region
        for r, t, o in self.calls:
            assert fn(self.ctx.handle, r, t, o, self.h) == 0

    def one(self, write=False):
        fn = self.lib.zcg_write_regions_v if write else self.lib.zcg_read_regions_v
        assert fn(self.ctx.handle, ctypes.byref(self.shared), ctypes.addressof(self.tlo), ctypes.addressof(self.tn),
                  self.S.table.data_ptr(), self.vb.data_ptr(), self.B, self.scratch.data_ptr(),
                  self.status.data_ptr(), self.h) == 0

    def check(self):
        """(b) must write what (a) writes (read direction)."""
        import torch
        self.loop()
        self.one()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all()) and torch.equal(self.out_a, self.out_b), \
            "zcg_read_regions_v differs from zcg_read_region"


def report(C, st, a="a", b="b"):
    gbs = lambda s: round(2 * C.bytes / (s["median_ms"] * 1e-3) / 1e9, 1)  # noqa: E731
    return {"boxes": C.B, "bytes_of_boxes": C.bytes, "a_loop_of_single_box_calls": st[a], "b_one_v_call": st[b],
            "a_gb_s_read_plus_written": gbs(st[a]), "b_gb_s_read_plus_written": gbs(st[b]),
            "speedup_of_medians": round(st[a]["median_ms"] / st[b]["median_ms"], 3),
            "b_against_a": verdict(st[a], st[b])}


def leg_mixed(repeats):
    import numpy as np
    import torch
    S = Slots()
    rng = np.random.default_rng(11)
    res = {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); boxes with extents drawn from "
                       "{8, 16, 32, 64, 96}^3 at random unaligned offsets, fill, dense buffers", "repeats": repeats,
           "read": {}, "write": {}}
    for B in (16, 256, 4096):
        shapes = [[int(x) for x in rng.choice([8, 16, 32, 64, 96], 3)] for _ in range(B)]
        offsets = [[int(rng.integers(1, 1024 - s)) for s in shp] for shp in shapes]
        C = Calls(S, offsets, shapes)
        C.check()
        C.check()
        st = alternate({"a": C.loop, "b": C.one}, repeats, C.stream)
        res["read"][str(B)] = report(C, st)
        C.loop(True)
        C.one(True)
        torch.cuda.synchronize()
        assert bool((C.status == 0).all())
        st = alternate({"a": lambda: C.loop(True), "b": lambda: C.one(True)}, repeats, C.stream)
        res["write"][str(B)] = report(C, st)
        del C
        torch.cuda.empty_cache()
    return res


def leg_skew(repeats):
    import numpy as np
    S = Slots()
    rng = np.random.default_rng(12)
    shapes = [[256] * 3] + [[8] * 3] * 4095
    offsets = [[int(rng.integers(1, 1024 - s)) for s in shp] for shp in shapes]
    C = Calls(S, offsets, shapes)
    big, small = Calls(S, offsets[:1], shapes[:1]), Calls(S, offsets[1:], shapes[1:])
    for c in (C, big, small):
        c.check()
        c.check()
    res = {"workload": "the mixed leg's slots; one 256^3 box plus 4095 boxes of 8^3, u16, random unaligned offsets",
           "repeats": repeats}
    for name, write in (("read", False), ("write", True)):
        st = alternate({"a": lambda: C.loop(write), "b": lambda: C.one(write), "big": lambda: big.one(write),
                        "small": lambda: small.one(write)}, repeats, C.stream)
        r = report(C, st)
        r["v_call_on_the_256_box_alone"] = st["big"]
        r["v_call_on_the_4095_small_boxes_alone"] = st["small"]
        r["b_over_sum_of_the_two_alone"] = round(st["b"]["median_ms"] / (st["big"]["median_ms"] +
                                                                          st["small"]["median_ms"]), 3)
        res[name] = r
    return res


def leg_uniform(repeats):
    import numpy as np
    import torch
    from zarr_amd import _native
    from zarr_amd.region import BoundingBox, _region, _strides
    S = Slots()
    rng = np.random.default_rng(1)
    res = {"workload": "the mixed leg's slots; boxes of 64^3 (tools/boxes_bench.py's small_boxes): a = "
                       "zcg_read_regions, b = zcg_read_regions_v", "repeats": repeats, "by_boxes": {}}
    for B in (1, 16, 256, 4096):
        offsets = [[int(x) for x in rng.integers(1, 1024 - 64, 3)] for _ in range(B)]
        C = Calls(S, offsets, [[64] * 3] * B)
        C.check()
        recs = (_native.Box * B)()
        box_bytes = 64 ** 3 * 2
        for b, off in enumerate(offsets):
            for d in range(3):
                recs[b].offset[d] = off[d]
            recs[b].out = C.out_a.data_ptr() + b * box_bytes
        boxes = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).to(S.dev)
        shared = _region(S.meta, BoundingBox([0] * 3, [64] * 3), 2, True, 0, _strides([64] * 3, "C"))
        status = torch.full((B,), -1, dtype=torch.int32, device=S.dev)

        def one_shape():
            assert C.lib.zcg_read_regions(C.ctx.handle, ctypes.byref(shared), ctypes.addressof(C.tlo),
                                          ctypes.addressof(C.tn), S.table.data_ptr(), boxes.data_ptr(), B,
                                          status.data_ptr(), C.h) == 0

        one_shape()
        C.one()
        torch.cuda.synchronize()
        assert torch.equal(C.out_a, C.out_b)
        st = alternate({"a": one_shape, "b": C.one}, repeats, C.stream)
        res["by_boxes"][str(B)] = {"a_read_regions": st["a"], "b_read_regions_v": st["b"],
                                   "b_over_a_of_medians": round(st["b"]["median_ms"] / st["a"]["median_ms"], 3),
                                   "b_against_a": verdict(st["a"], st["b"])}
        del C
        torch.cuda.empty_cache()
    return res


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import BoundingBox, read_ndarray, read_ndarrays_v, region_grid, write_ndarray, write_ndarrays_v
    repeats = repeats if UNCAPPED else min(repeats, 3)  # the loop sides take 5 s per repeat
    meta = ArrayMetadata.new([256] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    shapes = [[int(v) for v in rng.choice([8, 16, 32, 64, 96], 3)] for _ in range(256)]
    offsets = [[int(rng.integers(0, 256 - s + 1)) for s in shp] for shp in shapes]
    boxes = [BoundingBox(o, s) for o, s in zip(offsets, shapes)]
    arrays = [full[tuple(slice(o, o + s) for o, s in zip(bb.offset, bb.shape))] + 1 for bb in boxes]
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(4), repeat=3)])
        visited = [set(itertools.product(*[range(a, a + k) for a, k in zip(*region_grid(meta, bb))])) for bb in boxes]
        got = read_ndarrays_v(h, "a", meta, boxes, np.uint16)  # warm-up; both paths must read the array's values
        for g, a in zip(got, arrays):
            assert np.array_equal(g + 1, a)
        assert np.array_equal(read_ndarray(h, "a", meta, boxes[0], np.uint16) + 1, arrays[0])
        wall = {"read_loop": [], "read_one": [], "write_loop": [], "write_one": []}
        for _ in range(repeats):
            t0 = time.perf_counter()
            for bb in boxes:
                read_ndarray(h, "a", meta, bb, np.uint16)
            wall["read_loop"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            read_ndarrays_v(h, "a", meta, boxes, np.uint16)
            wall["read_one"].append((time.perf_counter() - t0) * 1e3)
        for _ in range(repeats):
            t0 = time.perf_counter()
            for bb, a in zip(boxes, arrays):
                write_ndarray(h, "a", meta, bb.offset, a)
            wall["write_loop"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            write_ndarrays_v(h, "a", meta, offsets, arrays)
            wall["write_one"].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    s = {k: stats(v) for k, v in wall.items()}
    per_box, union = sum(len(v) for v in visited), len(set().union(*visited))
    return {"workload": "gzip-6 u16 array 256^3 in 64 chunks of 64^3 (temporary store); 256 overlapping boxes with "
                        "extents drawn from {8, 16, 32, 64, 96}^3 at random offsets, host arrays", "repeats": repeats,
            "loop_of_256_read_ndarray": dict(s["read_loop"], chunk_decodes=per_box),
            "one_read_ndarrays_v": dict(s["read_one"], chunk_decodes=union),
            "read_speedup_of_medians": round(s["read_loop"]["median_ms"] / s["read_one"]["median_ms"], 2),
            "loop_of_256_write_ndarray": dict(s["write_loop"], chunk_encodes=per_box),
            "one_write_ndarrays_v": dict(s["write_one"], chunk_encodes=union),
            "write_speedup_of_medians": round(s["write_loop"]["median_ms"] / s["write_one"]["median_ms"], 2)}


UNCAPPED = False  # --uncapped: the store leg runs --repeats repeats, not 3 at the most

LEGS = {"mixed": leg_mixed, "skew": leg_skew, "uniform": leg_uniform, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_v_bench.json"))
    ap.add_argument("--legs", default="mixed,skew,uniform,store")
    ap.add_argument("--uncapped", action="store_true", help="store leg: do not cap the repeats at 3")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    global UNCAPPED
    UNCAPPED = args.uncapped
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/boxes_v_bench.py", "legs": {}}
    for name in args.legs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats",
                                str(args.repeats)] + (["--uncapped"] if args.uncapped else []),
                               capture_output=True, text=True, timeout=LIMITS[name])
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
