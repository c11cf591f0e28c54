#!/usr/bin/env python3
"""Lists of coordinates: one zcg_read_points / zcg_write_points / read_points
call against the only route there is without it, the _v box calls with P boxes
of shape (1, 1, 1).  The method is tools/boxes_s_bench.py's: both sides in one
process, alternating, after a warm-up; median and min..max spread of each.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  device   4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array,
           tools/boxes_v_bench.py's), P = 2^16 and 2^20 distinct random points.
           Gather: (a) zcg_read_regions_v with P boxes of shape 1, (b) one
           zcg_read_points in caller order, (c) the same on the points sorted
           by chunk and place in the chunk (values in sorted order).  The same
           three for the scatter.  HIP events on the launch stream.
  store    the gzip-6 u16 array 512^3 of 512 chunks of 64^3 of
           tools/boxes_s_bench.py in a temporary store, 4 096 points spread over
           the array and 4 096 points in 8 chunks: (a) read_ndarrays_v
           (as_tensor) with 1-element boxes, (b) read_points(as_tensor); wall
           time, and the chunks decoded on each side.
Writes profiles/points_bench.json; exits 1 if (b) is slower than (a) beyond the
spread.

usage: tools/points_bench.py [--repeats R] [--out FILE] [--legs device,store]
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
from boxes_v_bench import GRID, Slots, alternate  # noqa: E402

LIMITS = {"device": 420, "store": 420}  # child time limits, seconds


def vbox_records(pts, bases):
    """zcg_vbox records of 1-element boxes, built without a Python loop."""
    import numpy as np
    P = len(pts)
    rec = np.zeros((P, 25), np.uint64)  # offset[8], shape[8], strides[8], base
    rec[:, 0:3] = pts
    rec[:, 8:11] = 1
    rec[:, 16:19] = 1
    rec[:, 24] = bases
    return rec


class Sides:
    """P points on the synthetic slots: the 1-element-box route and the point calls."""

    def __init__(self, S, pts):
        import numpy as np
        import torch
        from zarr_amd import _native
        from zarr_amd.region import BoundingBox, _region
        self.ctx = _native.context(0)
        self.lib = self.ctx.lib
        self.S, self.P = S, len(pts)
        dev = S.dev
        P = self.P
        self.out = {k: torch.empty(P, dtype=torch.int16, device=dev) for k in "abc"}
        self.vals = torch.arange(P, dtype=torch.int16, device=dev)
        key = (pts // 64) @ np.array([256, 16, 1], np.uint64) * np.uint64(64 ** 3) + (pts % 64) @ np.array(
            [4096, 64, 1], np.uint64)
        self.perm = np.argsort(key, kind="stable")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
        self.coords = up(pts)
        self.sorted_coords = up(pts[self.perm])
        self.sorted_vals = self.vals[torch.from_numpy(self.perm).to(dev)].contiguous()
        at = np.uint64(2) * np.arange(P, dtype=np.uint64)
        self.vb_out = up(vbox_records(pts, np.uint64(self.out["a"].data_ptr()) + at))
        self.vb_in = up(vbox_records(pts, np.uint64(self.vals.data_ptr()) + at))
        self.status = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(self.lib.zcg_regions_v_scratch_bytes(P), dtype=torch.uint8, device=dev)
        self.first = torch.zeros(1, dtype=torch.int64, device=dev)
        self.r = _region(S.meta, BoundingBox([0] * 3, [1] * 3), 2, True, 0, [0] * 3)
        self.tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
        self.tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*GRID)
        self.stream = torch.cuda.current_stream(dev)
        self.h = self.stream.cuda_stream

    def _v(self, fn, boxes):
        assert fn(self.ctx.handle, ctypes.byref(self.r), ctypes.addressof(self.tlo), ctypes.addressof(self.tn),
                  self.S.table.data_ptr(), boxes.data_ptr(), self.P, self.scratch.data_ptr(), self.status.data_ptr(),
                  self.h) == 0

    def _p(self, fn, coords, vals):
        assert fn(self.ctx.handle, ctypes.byref(self.r), ctypes.addressof(self.tlo), ctypes.addressof(self.tn),
                  self.S.table.data_ptr(), coords.data_ptr(), self.P, vals.data_ptr(), self.first.data_ptr(),
                  self.h) == 0

    def read_a(self):
        self._v(self.lib.zcg_read_regions_v, self.vb_out)

    def read_b(self):
        self._p(self.lib.zcg_read_points, self.coords, self.out["b"])

    def read_c(self):
        self._p(self.lib.zcg_read_points, self.sorted_coords, self.out["c"])

    def write_a(self):
        self._v(self.lib.zcg_write_regions_v, self.vb_in)

    def write_b(self):
        self._p(self.lib.zcg_write_points, self.coords, self.vals)

    def write_c(self):
        self._p(self.lib.zcg_write_points, self.sorted_coords, self.sorted_vals)

    def check(self):
        """The three gathers agree; after each scatter a gather returns the values."""
        import torch
        perm = torch.from_numpy(self.perm).to(self.S.dev)
        for fn in (self.read_a, self.read_b, self.read_c):
            fn()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all()) and int(self.first.cpu().numpy().view("u8")[0]) == 2 ** 64 - 1
        assert torch.equal(self.out["a"], self.out["b"]) and torch.equal(self.out["a"][perm], self.out["c"]), \
            "zcg_read_points differs from zcg_read_regions_v with boxes of shape 1"
        keep = self.out["a"].clone()
        for fn in (self.write_a, self.write_b, self.write_c):
            self.vals.copy_(keep)  # put the old elements back first, then the new ones
            self.write_b()
            self.vals.copy_(torch.arange(self.P, dtype=torch.int16, device=self.S.dev))
            fn()
            self.read_b()
            torch.cuda.synchronize()
            assert torch.equal(self.out["b"], self.vals), "a scatter did not place the values"
        self.vals.copy_(keep)
        self.write_b()
        self.vals.copy_(torch.arange(self.P, dtype=torch.int16, device=self.S.dev))
        torch.cuda.synchronize()


def compare(st):
    a, b, c = st["a"], st["b"], st["c"]
    return {"a_one_element_boxes": a, "b_points_caller_order": b, "c_points_sorted": c,
            "a_over_b_of_medians": round(a["median_ms"] / b["median_ms"], 3),
            "b_over_c_of_medians": round(b["median_ms"] / c["median_ms"], 3), "b_against_a": verdict(a, b)}


def leg_device(repeats):
    import numpy as np
    import torch
    S = Slots()
    rng = np.random.default_rng(33)
    res = {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); P distinct uniformly random points, "
                       "fill; a = the _v call with P boxes of shape 1, b = one point call in caller order, c = one "
                       "point call on the points sorted by chunk and place", "repeats": repeats, "by_points": {}}
    for P in (1 << 16, 1 << 20):
        lin = rng.choice(1 << 30, size=P, replace=False).astype(np.uint64)
        pts = np.stack([lin >> np.uint64(20), (lin >> np.uint64(10)) & np.uint64(1023), lin & np.uint64(1023)], axis=1)
        C = Sides(S, pts)
        C.check()
        rd = alternate({"a": C.read_a, "b": C.read_b, "c": C.read_c}, repeats, C.stream)
        wr = alternate({"a": C.write_a, "b": C.write_b, "c": C.write_c}, repeats, C.stream)
        rate = lambda s: {"points_per_us": round(P / (s["median_ms"] * 1e3), 1),  # noqa: E731
                          "payload_gb_s": round(2 * P / (s["median_ms"] * 1e-3) / 1e9, 2),
                          "gb_s_at_one_64_byte_line_per_point": round(64 * P / (s["median_ms"] * 1e-3) / 1e9, 1)}
        res["by_points"][str(P)] = {"gather": dict(compare(rd), b_rate=rate(rd["b"]), c_rate=rate(rd["c"])),
                                    "scatter": dict(compare(wr), b_rate=rate(wr["b"]), c_rate=rate(wr["c"])),
                                    "bytes_per_point": {"a_record": 200, "b_coordinates": 24, "payload": 2}}
        del C
        torch.cuda.empty_cache()
    return res


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import BoundingBox, read_ndarrays_v, read_points
    meta = ArrayMetadata.new([512] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    full = np.tile(full, (2, 2, 2))  # 512^3: the 256^3 block in every octant
    res = {"workload": "gzip-6 u16 array 512^3 in 512 chunks of 64^3 (temporary store); 4096 points; a = "
                       "read_ndarrays_v(as_tensor=True) with 1-element boxes, b = read_points(as_tensor=True); "
                       "wall time", "repeats": repeats, "by_spread": {}}
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(8), repeat=3)])
        P = 4096
        for name, hi in (("whole_array", 512), ("eight_chunks", 128)):
            pts = rng.integers(0, hi, (P, 3)).astype(np.uint64)
            boxes = [BoundingBox([int(v) for v in c], [1, 1, 1]) for c in pts]
            want = full[tuple(pts[:, k].astype(np.int64) for k in range(3))]

            def box_route():
                t, _, _ = read_ndarrays_v(h, "a", meta, boxes, np.uint16, as_tensor=True)
                torch.cuda.synchronize()
                return t

            def point_route():
                t = read_points(h, "a", meta, pts, np.uint16, as_tensor=True)
                torch.cuda.synchronize()
                return t

            assert np.array_equal(box_route().cpu().numpy().view(np.uint16), want)
            assert np.array_equal(point_route().cpu().numpy().view(np.uint16), want)
            wall = {"a": [], "b": []}
            for _ in range(repeats):
                for side, fn in (("a", box_route), ("b", point_route)):
                    t0 = time.perf_counter()
                    fn()
                    wall[side].append((time.perf_counter() - t0) * 1e3)
            st = {k: stats(v) for k, v in wall.items()}
            chunks = len({tuple(int(v) // 64 for v in c) for c in pts})
            res["by_spread"][name] = {"a_one_element_boxes": st["a"], "b_read_points": st["b"],
                                      "a_over_b_of_medians": round(st["a"]["median_ms"] / st["b"]["median_ms"], 3),
                                      "b_against_a": verdict(st["a"], st["b"]), "points": P,
                                      "a_chunks_decoded": chunks, "b_chunks_decoded": chunks}
    return res


LEGS = {"device": leg_device, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"))
    ap.add_argument("--legs", default="device,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/points_bench.py", "legs": {}}
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
    slower = []
    for leg, r in res["legs"].items():
        for k, v in r.get("by_points", {}).items():
            slower += [f"{leg}/{k}/{dirn}" for dirn in ("gather", "scatter") if v[dirn]["b_against_a"] == "slower"]
        slower += [f"{leg}/{k}" for k, v in r.get("by_spread", {}).items() if v["b_against_a"] == "slower"]
    if slower:
        print("the point call is slower than the 1-element boxes beyond the spread: " + ", ".join(slower),
              file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
