#!/usr/bin/env python3
"""Orthogonal selections: one zcg_read_ortho / read_ortho call against the two
routes there are without it, the point calls on the expanded product and the
dense hull plus an index-select per dimension.  The method is
tools/points_bench.py's: all sides in one process, alternating, after a
warm-up; median and min..max spread of each.

Legs (each in a child process of its own under a time limit; a child that
fails, faults or runs out of time ends the run there):
  device   4 096 synthetic u16 chunk slots of 64^3 (2 GiB, a 1024^3 array,
           tools/boxes_v_bench.py's), a 128 x 128 x 64 selection of random
           sorted indices (2^20 elements).  (o) one zcg_read_ortho, (p) one
           zcg_read_points on the product's coordinates, already on the device,
           (pb) the same plus building the coordinate tensor on the device,
           (h) zcg_read_regions_v of the hull and an index_select per
           dimension.  HIP events on the launch stream.
  store    the gzip-6 u16 array 512^3 of 512 chunks of 64^3 of
           tools/points_bench.py in a temporary store, 64 x 64 x 64 indices
           over the whole array and within eight chunks: (a) read_points
           (as_tensor) on the product, (b) read_ortho(as_tensor); wall time,
           and the chunks decoded on each side.
Writes profiles/ortho_bench.json.

usage: tools/ortho_bench.py [--repeats R] [--out FILE] [--legs device,store]
"""
import argparse
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


def leg_device(repeats):
    import numpy as np
    import torch
    from zarr_amd.region import (assemble_ortho, assemble_points, assemble_regions_v, ortho_scratch_bytes,
                                 regions_v_scratch_bytes, vboxes_tensor)
    S = Slots()
    dev, meta = S.dev, S.meta
    rng = np.random.default_rng(44)
    counts = [128, 128, 64]
    lists = [np.sort(rng.choice(1024, size=c, replace=False)).astype(np.int64) for c in counts]
    P = int(np.prod(counts))
    tens = [torch.from_numpy(a).to(dev) for a in lists]
    lo, n = [0] * 3, list(GRID)
    stream = torch.cuda.current_stream(dev)
    out = {k: torch.zeros(P, dtype=torch.int16, device=dev) for k in ("o", "p", "pb")}
    # (o)
    scratch = torch.empty(ortho_scratch_bytes(counts), dtype=torch.uint8, device=dev)
    outside = torch.zeros(3, dtype=torch.int64, device=dev)
    strides = [counts[1] * counts[2], counts[2], 1]

    def ortho():
        assemble_ortho(meta, 2, S.table, lo, n, tens, out["o"], strides, outside, True, 0, scratch=scratch)

    # (p), (pb)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    coords = torch.cartesian_prod(*tens).contiguous()

    def points():
        assemble_points(meta, 2, S.table, lo, n, coords, out["p"], first, True, 0)

    def points_build():
        c = torch.cartesian_prod(*tens).contiguous()
        assemble_points(meta, 2, S.table, lo, n, c, out["pb"], first, True, 0)

    # (h)
    off = [int(a[0]) for a in lists]
    hshape = [int(a[-1] - a[0] + 1) for a in lists]
    hull = torch.empty(hshape, dtype=torch.int16, device=dev)
    vb = vboxes_tensor([off], [hshape], [[hshape[1] * hshape[2], hshape[2], 1]], [hull.data_ptr()])
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    vscratch = torch.empty(regions_v_scratch_bytes(1), dtype=torch.uint8, device=dev)
    rel = [t - o for t, o in zip(tens, off)]
    res_h = {}

    def hull_select():
        assemble_regions_v(meta, hshape, 2, S.table, lo, n, vb, status, True, 0, scratch=vscratch)
        res_h["v"] = hull.index_select(0, rel[0]).index_select(1, rel[1]).index_select(2, rel[2])

    for fn in (ortho, points, points_build, hull_select):
        fn()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and [int(x) for x in outside.cpu().numpy().view("u8")] == [2 ** 64 - 1] * 3
    assert torch.equal(out["o"], out["p"]) and torch.equal(out["o"], out["pb"]), "zcg_read_ortho differs from the points"
    assert torch.equal(out["o"], res_h["v"].reshape(-1)), "zcg_read_ortho differs from the hull under index_select"
    st = alternate({"o": ortho, "p": points, "pb": points_build, "h": hull_select}, repeats, stream)
    rate = lambda s: {"elements_per_us": round(P / (s["median_ms"] * 1e3), 1),  # noqa: E731
                      "payload_gb_s": round(2 * P / (s["median_ms"] * 1e-3) / 1e9, 2)}
    return {"workload": "4096 u16 slots of 64^3 (2 GiB, array 1024^3, C order); a 128 x 128 x 64 selection of random "
                        "sorted distinct indices, fill, dense C-order output; o = one zcg_read_ortho, p = one "
                        "zcg_read_points on the product's coordinates (on the device already), pb = p plus "
                        "torch.cartesian_prod of the lists on the device, h = zcg_read_regions_v of the hull ("
                        + " x ".join(str(x) for x in hshape) + ") plus three index_select",
            "repeats": repeats, "elements": P, "o_ortho": st["o"], "p_points": st["p"],
            "pb_points_with_coordinate_build": st["pb"], "h_hull_index_select": st["h"],
            "p_over_o_of_medians": round(st["p"]["median_ms"] / st["o"]["median_ms"], 3),
            "pb_over_o_of_medians": round(st["pb"]["median_ms"] / st["o"]["median_ms"], 3),
            "h_over_o_of_medians": round(st["h"]["median_ms"] / st["o"]["median_ms"], 3),
            "o_against_p": verdict(st["p"], st["o"]), "o_against_h": verdict(st["h"], st["o"]),
            "o_rate": rate(st["o"]), "p_rate": rate(st["p"]),
            "bytes_per_element": {"p_coordinates": 24, "payload": 2, "o_records_in_all": 32 * sum(counts)}}


def leg_store(repeats):
    import numpy as np
    import torch
    from zarr_amd import ArrayMetadata, FilesystemHierarchy, Gzip, SliceDataChunk
    from zarr_amd.region import ortho_chunks, read_ortho, read_points
    meta = ArrayMetadata.new([512] * 3, [64] * 3, "<u2", Gzip(6))
    meta.chunk_memory_layout = "C"
    rng = np.random.default_rng(3)
    x = np.arange(256, dtype=np.float32)
    full = (1000 * np.sin(x / 17)[:, None, None] + 800 * np.cos(x / 29)[None, :, None] + 3 * x[None, None, :]
            + rng.integers(0, 4, (256, 256, 256)) + 3000).astype(np.uint16)
    full = np.tile(full, (2, 2, 2))  # 512^3: the 256^3 block in every octant
    res = {"workload": "gzip-6 u16 array 512^3 in 512 chunks of 64^3 (temporary store); 64 x 64 x 64 random sorted "
                       "distinct indices; a = read_points(as_tensor=True) on the product (the 6 MiB coordinate array "
                       "built before the clock starts), b = read_ortho(as_tensor=True); wall time",
           "repeats": repeats, "by_spread": {}}
    with tempfile.TemporaryDirectory() as d:
        h = FilesystemHierarchy.open_or_create(d)
        h.create_array("a", meta)
        h.write_chunks("a", meta, [SliceDataChunk(list(c), np.ascontiguousarray(
            full[tuple(slice(i * 64, i * 64 + 64) for i in c)]).reshape(-1))
            for c in itertools.product(range(8), repeat=3)])
        for name, hi in (("whole_array", 512), ("eight_chunks", 128)):
            lists = [np.sort(rng.choice(hi, size=64, replace=False)).astype(np.uint64) for _ in range(3)]
            t0 = time.perf_counter()
            pts = np.stack([g.reshape(-1) for g in np.meshgrid(*lists, indexing="ij")], axis=1)
            build_ms = (time.perf_counter() - t0) * 1e3
            want = full[np.ix_(*[a.astype(np.int64) for a in lists])]

            def point_route():
                t = read_points(h, "a", meta, pts, np.uint16, as_tensor=True)
                torch.cuda.synchronize()
                return t

            def ortho_route():
                t = read_ortho(h, "a", meta, lists, np.uint16, as_tensor=True)
                torch.cuda.synchronize()
                return t

            assert np.array_equal(point_route().cpu().numpy().view(np.uint16).reshape(want.shape), want)
            assert np.array_equal(ortho_route().cpu().numpy().view(np.uint16).reshape(want.shape), want)
            wall = {"a": [], "b": []}
            for _ in range(repeats):
                for side, fn in (("a", point_route), ("b", ortho_route)):
                    t0 = time.perf_counter()
                    fn()
                    wall[side].append((time.perf_counter() - t0) * 1e3)
            st = {k: stats(v) for k, v in wall.items()}
            chunks = len({tuple(int(v) // 64 for v in c) for c in itertools.product(*lists)})
            res["by_spread"][name] = {"a_read_points": st["a"], "b_read_ortho": st["b"],
                                      "a_over_b_of_medians": round(st["a"]["median_ms"] / st["b"]["median_ms"], 3),
                                      "b_against_a": verdict(st["a"], st["b"]), "elements": int(pts.shape[0]),
                                      "a_coordinate_build_ms_not_in_a": round(build_ms, 2),
                                      "a_coordinate_bytes": int(pts.nbytes), "b_index_bytes": 8 * 3 * 64,
                                      "a_chunks_decoded": chunks, "b_chunks_decoded": ortho_chunks(meta, lists)[3]}
    return res


LEGS = {"device": leg_device, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ortho_bench.json"))
    ap.add_argument("--legs", default="device,store")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child](args.repeats)))
        return 0
    res = {"source": "tools/ortho_bench.py", "legs": {}}
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
