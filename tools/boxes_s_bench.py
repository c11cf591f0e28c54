#!/usr/bin/env python3
"""Strided boxes: one zcg_read_regions_s / read_ndarrays_s call against the
only route there is without it — the dense read of every box's hull
(zcg_read_regions_v / read_ndarrays_v) followed by a device slice [::step] and
copy per box.  The method is tools/boxes_v_bench.py's: both sides in one
process, alternating, after a warm-up; median and min..max spread of each.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  device   4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array,
           tools/boxes_v_bench.py's): 32 boxes of 32 x 32 x 256 samples with
           steps 1, 2 and 4 in every dimension, and 8 boxes of 8 x 8 x 16
           samples with a step of the chunk extent, 64; random offsets, fill,
           dense views.  (a) zcg_read_regions_v of the hulls plus B sliced
           copies, (b) one zcg_read_regions_s.  Step 1 also records (b) against
           zcg_read_regions_v alone.  HIP events on the launch stream.
  store    a gzip-6 u16 array 512^3 of 512 chunks of 64^3 in a temporary store:
           16 boxes of 48^3 samples at steps 2 and 4, 4 boxes of 6^3 samples at
           the chunk extent 64 (every chunk of a hull's range holds one sample)
           and 4 boxes of 4^3 samples at twice the chunk extent (one chunk in
           eight holds a sample).  (a) read_ndarrays_v(as_tensor=True) of the
           hulls plus the sliced copies, (b) read_ndarrays_s(as_tensor=True);
           wall time, and the chunks decoded on each side.
Writes profiles/boxes_s_bench.json; exits 1 if (b) is slower than (a) beyond
the spread for a step above 1.

usage: tools/boxes_s_bench.py [--repeats R] [--out FILE] [--legs device,store]
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


def hull_of(counts, steps):
    return [(c - 1) * s + 1 if c else 0 for c, s in zip(counts, steps)]


class Sides:
    """One box list on the synthetic slots: the hull route and the strided call."""

    def __init__(self, S, offsets, counts, steps):
        import numpy as np
        import torch
        from zarr_amd import _native
        from zarr_amd.region import BoundingBox, _region, _strides, sboxes_tensor, vboxes_tensor
        self.ctx = _native.context(0)
        self.lib = self.ctx.lib
        self.S, self.B = S, len(offsets)
        dev = S.dev
        hulls = [hull_of(c, s) for c, s in zip(counts, steps)]
        at, hat = [0], [0]
        for c, h in zip(counts, hulls):
            at.append(at[-1] + int(np.prod(c)) * 2)
            hat.append(hat[-1] + int(np.prod(h)) * 2)
        self.bytes, self.hull_bytes = at[-1], hat[-1]
        self.out_a = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        self.out_b = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        self.hull = torch.empty(self.hull_bytes, dtype=torch.uint8, device=dev)
        self.vb = vboxes_tensor(offsets, hulls, [_strides(h, "C") for h in hulls],
                                [self.hull.data_ptr() + a for a in hat[:-1]])
        self.sb = sboxes_tensor(offsets, counts, steps, [_strides(c, "C") for c in counts],
                                [self.out_b.data_ptr() + a for a in at[:-1]])
        # the sliced copies of side (a): hull view [::step] -> the box, dense
        self.copies = []
        for b in range(self.B):
            src = self.hull[hat[b]:hat[b + 1]].view(torch.int16).view(*hulls[b])
            src = src[tuple(slice(None, None, s) for s in steps[b])]
            dst = self.out_a[at[b]:at[b + 1]].view(torch.int16).view(*counts[b])
            self.copies.append((dst, src))
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(self.lib.zcg_regions_s_scratch_bytes(self.B), dtype=torch.uint8, device=dev)
        bound = lambda xs: [max(x[d] for x in xs) for d in range(3)]  # noqa: E731
        self.r_hull = _region(S.meta, BoundingBox([0] * 3, bound(hulls)), 2, True, 0, [0] * 3)
        self.r_s = _region(S.meta, BoundingBox([0] * 3, bound(counts)), 2, True, 0, [0] * 3)
        self.tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
        self.tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*GRID)
        self.stream = torch.cuda.current_stream(dev)
        self.h = self.stream.cuda_stream

    def dense(self):
        assert self.lib.zcg_read_regions_v(self.ctx.handle, ctypes.byref(self.r_hull), ctypes.addressof(self.tlo),
                                           ctypes.addressof(self.tn), self.S.table.data_ptr(), self.vb.data_ptr(),
                                           self.B, self.scratch.data_ptr(), self.status.data_ptr(), self.h) == 0

    def hull_route(self):
        self.dense()
        for dst, src in self.copies:
            dst.copy_(src)

    def strided(self):
        assert self.lib.zcg_read_regions_s(self.ctx.handle, ctypes.byref(self.r_s), ctypes.addressof(self.tlo),
                                           ctypes.addressof(self.tn), self.S.table.data_ptr(), self.sb.data_ptr(),
                                           self.B, self.scratch.data_ptr(), self.status.data_ptr(), self.h) == 0

    def check(self):
        import torch
        self.hull_route()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all())
        self.strided()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all()) and torch.equal(self.out_a, self.out_b), \
            "zcg_read_regions_s differs from the sliced hull"


def compare(a, b):
    return {"a_hull_route": a, "b_one_s_call": b, "a_over_b_of_medians": round(a["median_ms"] / b["median_ms"], 3),
            "b_against_a": verdict(a, b)}


def leg_device(repeats):
    import numpy as np
    import torch
    S = Slots()
    rng = np.random.default_rng(21)
    res = {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); strided boxes at random offsets, "
                       "fill, dense views; a = zcg_read_regions_v of the hulls + a sliced device copy per box, "
                       "b = one zcg_read_regions_s", "repeats": repeats, "by_step": {}}
    for step, B, counts in ((1, 32, [32, 32, 256]), (2, 32, [32, 32, 256]), (4, 32, [32, 32, 256]),
                            (64, 8, [8, 8, 16])):
        hull = hull_of(counts, [step] * 3)
        offsets = [[int(rng.integers(0, 1024 - h + 1)) for h in hull] for _ in range(B)]
        C = Sides(S, offsets, [counts] * B, [[step] * 3] * B)
        C.check()
        C.check()
        sides = {"a": C.hull_route, "b": C.strided}
        if step == 1:
            sides["v"] = C.dense
        st = alternate(sides, repeats, C.stream)
        r = dict(compare(st["a"], st["b"]), boxes=B, samples_per_box=counts, bytes_of_boxes=C.bytes,
                 bytes_of_hulls=C.hull_bytes,
                 b_gb_s_of_boxes=round(C.bytes / (st["b"]["median_ms"] * 1e-3) / 1e9, 1))
        if step == 1:
            r["v_read_regions_v_alone"] = st["v"]
            r["b_over_v_of_medians"] = round(st["b"]["median_ms"] / st["v"]["median_ms"], 3)
            r["b_against_v"] = verdict(st["v"], st["b"])
        res["by_step"][str(step)] = r
        del C
        torch.cuda.empty_cache()
    return res


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import BoundingBox, read_ndarrays_s, read_ndarrays_v, region_grid, region_s_chunks
    meta = ArrayMetadata.new([512] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    full = np.tile(full, (2, 2, 2))  # 512^3: the 256^3 block in every octant
    res = {"workload": "gzip-6 u16 array 512^3 in 512 chunks of 64^3 (temporary store); a = "
                       "read_ndarrays_v(as_tensor=True) of the hulls + a sliced device copy per box, b = "
                       "read_ndarrays_s(as_tensor=True); wall time", "repeats": repeats, "by_step": {}}
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(8), repeat=3)])
        for step, B, n in ((2, 16, 48), (4, 16, 48), (64, 4, 6), (128, 4, 4)):
            counts, steps = [n] * 3, [step] * 3
            hull = hull_of(counts, steps)
            offsets = [[int(rng.integers(0, 512 - k + 1)) for k in hull] for _ in range(B)]
            boxes = [BoundingBox(o, counts) for o in offsets]
            hulls = [BoundingBox(o, hull) for o in offsets]
            sl = tuple(slice(None, None, step) for _ in range(3))
            out = torch.empty(B * n ** 3, dtype=torch.int16, device="cuda")

            def hull_route():
                t, at, _ = read_ndarrays_v(h, "a", meta, hulls, np.uint16, as_tensor=True)
                for b in range(B):
                    src = t[at[b]:at[b] + 2 * hull[0] * hull[1] * hull[2]].view(torch.int16).view(*hull)[sl]
                    out[b * n ** 3:(b + 1) * n ** 3].view(n, n, n).copy_(src)
                torch.cuda.synchronize()
                return out

            def strided():
                t, _, _ = read_ndarrays_s(h, "a", meta, boxes, steps, np.uint16, as_tensor=True)
                torch.cuda.synchronize()
                return t

            want = np.stack([full[tuple(slice(o, o + k, step) for o, k in zip(off, hull))] for off in offsets])
            assert np.array_equal(hull_route().cpu().numpy().view(np.uint16).reshape(want.shape), want)
            assert np.array_equal(strided().cpu().numpy().view(np.uint16).reshape(want.shape), want)
            wall = {"a": [], "b": []}
            for _ in range(repeats):
                for name, fn in (("a", hull_route), ("b", strided)):
                    t0 = time.perf_counter()
                    fn()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            st = {k: stats(v) for k, v in wall.items()}
            dense, touched = set(), set()
            for off in offsets:
                lo, k = region_grid(meta, BoundingBox(off, hull))
                dense |= set(itertools.product(*[range(a, a + m) for a, m in zip(lo, k)]))
                lo, k, t, cnt = region_s_chunks(meta, off, counts, steps)
                touched |= set(itertools.product(*[[lo[i] + j for j in range(k[i]) if t[i][j]] for i in range(3)]))
            res["by_step"][str(step)] = dict(compare(st["a"], st["b"]), boxes=B, samples_per_box=counts,
                                             a_chunks_decoded=len(dense), b_chunks_decoded=len(touched),
                                             share_of_chunks_decoded=round(len(touched) / len(dense), 3),
                                             b_over_a_of_medians=round(st["b"]["median_ms"] / st["a"]["median_ms"], 3))
    return res


LEGS = {"device": leg_device, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_s_bench.json"))
    ap.add_argument("--legs", default="device,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/boxes_s_bench.py", "legs": {}}
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
    slower = [f"{leg}/step {s}" for leg, r in res["legs"].items() for s, v in r["by_step"].items()
              if int(s) > 1 and v["b_against_a"] == "slower"]
    if slower:
        print("the strided call is slower than the hull route beyond the spread: " + ", ".join(slower),
              file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
