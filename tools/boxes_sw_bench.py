#!/usr/bin/env python3
"""Strided box writes: one zcg_write_regions_s / write_ndarrays_s call against
the only route there is without it — the dense read of every box's hull
(zcg_read_regions_v / read_ndarrays_v), an overlay hull[::step] = box per box,
and the dense write of the hulls (zcg_write_regions_v / write_ndarrays_v).  The
method is tools/boxes_s_bench.py's: both sides in one process, alternating,
after a warm-up; median and min..max spread of each.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  device   4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array,
           tools/boxes_v_bench.py's): 32 boxes of 32 x 32 x 256 samples with
           steps 1, 2 and 4 in every dimension, their hulls pairwise disjoint
           (one box per 128 x 128 column), and 8 boxes of 8 x 8 x 16 samples
           with a step of the chunk extent, 64, at random offsets; dense input
           views.  (a) zcg_read_regions_v of the hulls, B sliced device copies,
           zcg_write_regions_v of the hulls; (b) one zcg_write_regions_s.  Step
           1 also records (b) against zcg_write_regions_v alone.  HIP events on
           the launch stream.  Where the hulls are disjoint both sides must
           leave the same slots.
  store    a gzip-6 u16 array 512^3 of 512 chunks of 64^3 in two temporary
           stores with the same files: 16 boxes of 48^3 samples at steps 2 and
           4, and 4 boxes of 4^3 samples at twice the chunk extent.  (a)
           read_ndarrays_v of the hulls, the overlay in numpy, write_ndarrays_v
           of the hulls, in one call each, on one store; (b) write_ndarrays_s
           on the other; wall time and the chunks decoded and encoded on each
           side.  (b) must equal the boxes applied in order to the array; (a)
           in one call is that result only where no two hulls overlap (step 2:
           one box per 128^3 cell), and must equal (b) there.
Writes profiles/boxes_sw_bench.json; exits 1 if, for a step above 1, a run of
(b) is slower than the slowest run of (a).

usage: tools/boxes_sw_bench.py [--repeats R] [--out FILE] [--legs device,store]
"""
import argparse
import ctypes
import itertools
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from boxes_bench import stats, verdict  # noqa: E402
from boxes_s_bench import hull_of  # noqa: E402
from boxes_v_bench import GRID, Slots, alternate  # noqa: E402

LIMITS = {"device": 300, "store": 420}  # child time limits, seconds


class Sides:
    """One box list on the synthetic slots: the hull route and the strided call."""

    def __init__(self, S, offsets, counts, steps, rng):
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
        self.src = torch.from_numpy(rng.integers(0, 256, self.bytes, dtype=np.uint8)).to(dev)
        self.hull = torch.empty(self.hull_bytes, dtype=torch.uint8, device=dev)
        self.vb = vboxes_tensor(offsets, hulls, [_strides(h, "C") for h in hulls],
                                [self.hull.data_ptr() + a for a in hat[:-1]])
        self.sb = sboxes_tensor(offsets, counts, steps, [_strides(c, "C") for c in counts],
                                [self.src.data_ptr() + a for a in at[:-1]])
        # the overlays of side (a): the box, dense -> hull view [::step]
        self.copies = []
        for b in range(self.B):
            dst = self.hull[hat[b]:hat[b + 1]].view(torch.int16).view(*hulls[b])
            dst = dst[tuple(slice(None, None, s) for s in steps[b])]
            self.copies.append((dst, self.src[at[b]:at[b + 1]].view(torch.int16).view(*counts[b])))
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(self.lib.zcg_regions_s_scratch_bytes(self.B), dtype=torch.uint8, device=dev)
        bound = lambda xs: [max(x[d] for x in xs) for d in range(3)]  # noqa: E731
        self.r_hull = _region(S.meta, BoundingBox([0] * 3, bound(hulls)), 2, True, 0, [0] * 3)
        self.r_s = _region(S.meta, BoundingBox([0] * 3, bound(counts)), 2, False, 0, [0] * 3)
        self.tlo = (ctypes.c_uint64 * _native.MAX_DIMS)()
        self.tn = (ctypes.c_uint64 * _native.MAX_DIMS)(*GRID)
        self.stream = torch.cuda.current_stream(dev)
        self.h = self.stream.cuda_stream

    def _v(self, fn, r):
        assert fn(self.ctx.handle, ctypes.byref(r), ctypes.addressof(self.tlo), ctypes.addressof(self.tn),
                  self.S.table.data_ptr(), self.vb.data_ptr(), self.B, self.scratch.data_ptr(),
                  self.status.data_ptr(), self.h) == 0

    def dense_write(self):
        self._v(self.lib.zcg_write_regions_v, self.r_hull)

    def hull_route(self):
        self._v(self.lib.zcg_read_regions_v, self.r_hull)
        for dst, src in self.copies:
            dst.copy_(src)
        self.dense_write()

    def strided(self):
        assert self.lib.zcg_write_regions_s(self.ctx.handle, ctypes.byref(self.r_s), ctypes.addressof(self.tlo),
                                            ctypes.addressof(self.tn), self.S.table.data_ptr(), self.sb.data_ptr(),
                                            self.B, self.scratch.data_ptr(), self.status.data_ptr(), self.h) == 0

    def check(self, same):
        """Both sides from the same slots; `same`: the hulls are disjoint and the slots must agree."""
        import torch
        keep = self.S.slots.clone() if same else None
        self.hull_route()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all())
        if same:
            after_a = self.S.slots.clone()
            self.S.slots.copy_(keep)
            del keep
        self.strided()
        torch.cuda.synchronize()
        assert bool((self.status == 0).all())
        if same:
            assert torch.equal(after_a, self.S.slots), "zcg_write_regions_s differs from the hull route"


def compare(a, b):
    return {"a_hull_route": a, "b_one_s_call": b, "a_over_b_of_medians": round(a["median_ms"] / b["median_ms"], 3),
            "b_against_a": verdict(a, b), "every_b_run_within_slowest_a_run": b["max_ms"] <= a["max_ms"]}


def device_boxes(rng, step, B, counts):
    """B boxes; for the 32-box shapes one box per 128 x 128 column of the array, so the hulls are disjoint."""
    hull = hull_of(counts, [step] * 3)
    if B == 32:
        return [[128 * (b % 8) + int(rng.integers(0, 128 - hull[0] + 1)),
                 128 * (b // 8) + int(rng.integers(0, 128 - hull[1] + 1)),
                 int(rng.integers(0, 1024 - hull[2] + 1))] for b in range(B)], True
    return [[int(rng.integers(0, 1024 - h + 1)) for h in hull] for _ in range(B)], False


def leg_device(repeats):
    import numpy as np
    import torch
    S = Slots()
    rng = np.random.default_rng(21)
    res = {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); strided boxes, dense input views; "
                       "a = zcg_read_regions_v of the hulls + a sliced device copy per box + zcg_write_regions_v "
                       "of the hulls, b = one zcg_write_regions_s", "repeats": repeats, "by_step": {}}
    for step, B, counts in ((1, 32, [32, 32, 256]), (2, 32, [32, 32, 256]), (4, 32, [32, 32, 256]),
                            (64, 8, [8, 8, 16])):
        offsets, disjoint = device_boxes(rng, step, B, counts)
        C = Sides(S, offsets, [counts] * B, [[step] * 3] * B, rng)
        C.check(disjoint)
        C.check(False)
        sides = {"a": C.hull_route, "b": C.strided}
        if step == 1:
            sides["v"] = C.dense_write
        st = alternate(sides, repeats, C.stream)
        r = dict(compare(st["a"], st["b"]), boxes=B, samples_per_box=counts, bytes_of_boxes=C.bytes,
                 bytes_of_hulls=C.hull_bytes, slots_compared=disjoint,
                 b_gb_s_of_boxes=round(C.bytes / (st["b"]["median_ms"] * 1e-3) / 1e9, 1))
        if step == 1:
            r["v_write_regions_v_alone"] = st["v"]
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
    from zarr_amd.region import BoundingBox, read_ndarrays_v, region_grid, region_s_chunks, write_ndarrays_s, \
        write_ndarrays_v
    meta = ArrayMetadata.new([512] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    full = np.tile(full, (2, 2, 2))  # 512^3: the 256^3 block in every octant
    res = {"workload": "gzip-6 u16 array 512^3 in 512 chunks of 64^3 (two temporary stores with the same files); a = "
                       "read_ndarrays_v of the hulls + hull[::step] = box in numpy + write_ndarrays_v of the hulls, "
                       "b = write_ndarrays_s, host arrays on both sides; wall time", "repeats": repeats, "by_step": {}}
    with tempfile.TemporaryDirectory() as d:
        ha = FilesystemHierarchy.open_or_create(os.path.join(d, "a"))
        ha.create_array("a", meta)
        ha.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(8), repeat=3)])
        shutil.copytree(os.path.join(d, "a"), os.path.join(d, "b"))
        hb = FilesystemHierarchy.open(os.path.join(d, "b"))
        model = full.copy()
        for step, B, n in ((2, 16, 48), (4, 16, 48), (128, 4, 4)):
            counts, steps = [n] * 3, [step] * 3
            hull = hull_of(counts, steps)
            disjoint = step == 2  # one box per 128^3 cell; the larger hulls overlap at random offsets
            if disjoint:
                cells = rng.permutation(64)[:B]
                offsets = [[128 * int(c // 16 % 4) + int(rng.integers(0, 34)), 128 * int(c // 4 % 4) +
                            int(rng.integers(0, 34)), 128 * int(c % 4) + int(rng.integers(0, 34))] for c in cells]
            else:
                offsets = [[int(rng.integers(0, 512 - k + 1)) for k in hull] for _ in range(B)]
            hulls = [BoundingBox(o, hull) for o in offsets]
            sl = tuple(slice(None, None, step) for _ in range(3))
            arrays = [rng.integers(0, 60000, counts).astype(np.uint16) for _ in range(B)]

            def hull_route():
                hs = read_ndarrays_v(ha, "a", meta, hulls, np.uint16)
                for b in range(B):
                    hs[b][sl] = arrays[b]
                write_ndarrays_v(ha, "a", meta, offsets, hs)
                torch.cuda.synchronize()

            def strided():
                write_ndarrays_s(hb, "a", meta, offsets, steps, arrays)
                torch.cuda.synchronize()

            hull_route()
            strided()
            # (b) against the definition, box by box in order, on the array itself
            for b in range(B):
                model[tuple(slice(o, o + k, step) for o, k in zip(offsets[b], hull))] = arrays[b]
            rb = read_ndarrays_v(hb, "a", meta, hulls, np.uint16)
            for b in range(B):
                assert np.array_equal(rb[b], model[tuple(slice(o, o + k) for o, k in zip(offsets[b], hull))]), \
                    "write_ndarrays_s differs from the model"
            # one call of (a) is the sequential result only where no two hulls overlap
            ra = read_ndarrays_v(ha, "a", meta, hulls, np.uint16)
            same = all(np.array_equal(p, q) for p, q in zip(ra, rb))
            assert same or not disjoint, "the hull route differs from write_ndarrays_s"
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
                                             a_chunks_decoded=len(dense), a_chunks_encoded=len(dense),
                                             b_chunks_decoded=len(touched), b_chunks_encoded=len(touched),
                                             share_of_chunks=round(len(touched) / len(dense), 3),
                                             hulls_disjoint=bool(disjoint), a_equals_b_over_the_hulls=bool(same),
                                             b_over_a_of_medians=round(st["b"]["median_ms"] / st["a"]["median_ms"], 3))
    return res


LEGS = {"device": leg_device, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_sw_bench.json"))
    ap.add_argument("--legs", default="device,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/boxes_sw_bench.py", "legs": {}}
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    slower = [f"{leg}/step {s}" for leg, r in res["legs"].items() for s, v in r["by_step"].items()
              if int(s) > 1 and not v["every_b_run_within_slowest_a_run"]]
    if slower:
        print("a run of the strided call is slower than the slowest run of the hull route: " + ", ".join(slower),
              file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
