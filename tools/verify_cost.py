#!/usr/bin/env python3
"""What the opt-in checksum verification costs (ZCG_FLAG_VERIFY_GZIP_TRAILER,
ZCG_FLAG_VERIFY_LZ4_CONTENT, ZCG_FLAG_VERIFY_ZLIB_TRAILER): device-resident batch decode with and without
the flag, alternating launch by launch, timed with HIP events on the launch
stream after a warm-up.  The data are bench.py's own (its generators and host
encoders are imported, bench.py is not changed).

Configurations: C2 (gzip level 6, f32, 4 096 x 1 MiB), LZ4 at 8 192 x 1 MiB
i16, and one lone 1 MiB chunk of each; and the zlib leg (c2_zlib_vs_gzip_4096):
C2's chunks as zlib streams (zlib.compress at level 6: the same deflate bodies)
beside the gzip members in ONE process, the four decodes (gzip, gzip + 0x1,
zlib, zlib + 0x8) alternating launch by launch, which gives the zlib decode
rate against gzip's and the Adler-32 pass against the CRC32 pass.  `--only`
runs a subset.  Each configuration runs in a child
process of its own under a time limit; a child that fails, faults or runs out
of time ends the run there.  Writes profiles/verify_cost.json: per
configuration the plain and the verifying decode in ms, the verify pass alone
(the difference of the two medians, the kernels are not launched apart) in ms
and GiB/s of the decoded bytes D, the decode-plus-verify to plain-decode
ratio, and for gzip the fraction of `--raw-gbs` (the raw codec's copy rate on
the same part, reading and writing D) the CRC pass reaches reading D once.

usage: tools/verify_cost.py [--steps K] [--warmup W] [--out FILE] [--raw-gbs R] [--only NAME,NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GIB = float(1 << 30)
CONFIGS = {  # name: (codec, batch, pool, child time limit in seconds)
    "c2_gzip_4096": ("gzip", 4096, 64, 420),
    "lz4_8192": ("lz4", 8192, 64, 420),
    "gzip_lone_chunk": ("gzip", 1, 1, 180),
    "lz4_lone_chunk": ("lz4", 1, 1, 180),
    "c2_zlib_vs_gzip_4096": ("zlib", 4096, 64, 420),
}


def pack(streams, n, pool, D, dev):
    """The pool's streams replicated into n device slots, n destinations of D
    bytes, and the descriptor / status arrays of a batch over them."""
    import numpy as np
    import torch
    order = np.arange(n, dtype=np.int64) % pool
    lens = np.array([len(s) for s in streams], np.int64)
    slot = int((lens.max() + 255) // 256 * 256)
    host_pool = np.zeros((pool, slot), np.uint8)
    for u, s in enumerate(streams):
        host_pool[u, :len(s)] = np.frombuffer(s, np.uint8)
    src = torch.from_numpy(host_pool).to(dev).index_select(0, torch.from_numpy(order).to(dev))
    dst = torch.empty(n * D, dtype=torch.uint8, device=dev)
    desc = np.stack([src.data_ptr() + np.arange(n, dtype=np.uint64) * slot, lens[order].astype(np.uint64),
                     dst.data_ptr() + np.arange(n, dtype=np.uint64) * D, np.full(n, D, np.uint64)], 1)

    class _P:
        pass
    packed = _P()
    packed.n = n
    packed.src, packed.dst, packed.order = src, dst, order
    packed.desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.int64)).to(dev)
    packed.status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    return packed


def child_zlib(name, steps, warmup):
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    import torch
    import bench
    from zarr_amd import ArrayMetadata, Zlib, _native
    from zarr_amd.batch import BatchCodec
    _, n, pool, _ = CONFIGS[name]
    dev = torch.device("cuda", 0)
    gmeta, gen, desc_txt = bench.workload("gzip")
    vals = [gen(i) for i in range(pool)]
    gz = bench.host_encode("gzip", vals, min(16, os.cpu_count() or 1))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        zs = list(ex.map(lambda v: zlib.compress(v.tobytes(), 6), vals))
    assert all(z[2:-4] == g[10:-8] for z, g in zip(zs, gz)), "the two containers hold the same deflate bodies"
    D = vals[0].nbytes
    zmeta = ArrayMetadata.new(gmeta.shape, gmeta.chunk_shape, gmeta.data_type, Zlib(6))
    gpack, zpack = pack(gz, n, pool, D, dev), pack(zs, n, pool, D, dev)
    legs = {"gzip": (gmeta, gpack, 0), "gzip_verify": (gmeta, gpack, _native.FLAG_VERIFY_GZIP_TRAILER),
            "zlib": (zmeta, zpack, 0), "zlib_verify": (zmeta, zpack, _native.FLAG_VERIFY_ZLIB_TRAILER)}
    bc = BatchCodec(0)
    stream = torch.cuda.current_stream(dev)
    ref = torch.from_numpy(np.stack([v.view(np.uint8) for v in vals])).to(dev)
    for leg, (meta, packed, f) in legs.items():  # warm-up, and every leg must decode every chunk to its input
        for _ in range(max(warmup, 1)):
            bc.decode(meta, packed, stream=stream, flags=f)
        torch.cuda.synchronize()
        assert (packed.status == 0).all().item(), (name, leg)
        out = packed.dst.view(n, D)
        for c0 in range(0, n, 256):
            want = ref[torch.from_numpy(packed.order[c0:c0 + 256]).to(dev)]
            assert bool((out[c0:c0 + 256] == want).all().item()), (name, leg)
    ms = {leg: [] for leg in legs}
    for _ in range(steps):  # alternating, so drift hits all four alike
        for leg, (meta, packed, f) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            bc.decode(meta, packed, stream=stream, flags=f)
            b.record(stream)
            torch.cuda.synchronize()
            ms[leg].append(a.elapsed_time(b))
    med = {leg: float(np.median(v)) for leg, v in ms.items()}
    crc, adler = med["gzip_verify"] - med["gzip"], med["zlib_verify"] - med["zlib"]
    gbs = lambda t: round(n * D / 1e9 / (max(t, 1e-6) * 1e-3), 1)  # noqa: E731
    print("RESULT " + json.dumps({
        "workload": desc_txt + "; the same chunks as zlib streams (zlib.compress level 6)", "chunks": n,
        "chunk_bytes": D, "steps": steps,
        "ms": {leg: round(v, 4) for leg, v in med.items()},
        "ms_min_max": {leg: [round(min(v), 4), round(max(v), 4)] for leg, v in ms.items()},
        "gib_s": {leg: round(n * D / GIB / (v * 1e-3), 2) for leg, v in med.items()},
        "zlib_to_gzip_decode_ratio": round(med["zlib"] / med["gzip"], 4),
        "crc32_pass_ms": round(crc, 4), "adler32_pass_ms": round(adler, 4),
        "crc32_pass_gbs": gbs(crc), "adler32_pass_gbs": gbs(adler),
        "adler32_to_crc32_pass_ratio": round(adler / max(crc, 1e-6), 4)}))


def child(name, steps, warmup):
    import numpy as np
    import torch
    import bench
    from zarr_amd import _native
    from zarr_amd.batch import BatchCodec
    codec, n, pool, _ = CONFIGS[name]
    dev = torch.device("cuda", 0)
    meta, gen, desc_txt = bench.workload(codec)
    vals = [gen(i) for i in range(pool)]
    streams = bench.host_encode(codec, vals, min(16, os.cpu_count() or 1))
    D = vals[0].nbytes
    packed = pack(streams, n, pool, D, dev)
    order, dst = packed.order, packed.dst
    bc = BatchCodec(0)
    stream = torch.cuda.current_stream(dev)
    flag = _native.FLAG_VERIFY_GZIP_TRAILER if codec == "gzip" else _native.FLAG_VERIFY_LZ4_CONTENT
    ref = torch.from_numpy(np.stack([v.view(np.uint8) for v in vals])).to(dev)
    for f in (0, flag):  # warm-up, and both must decode every chunk to its input
        for _ in range(max(warmup, 1)):
            bc.decode(meta, packed, stream=stream, flags=f)
        torch.cuda.synchronize()
        assert (packed.status == 0).all().item(), (name, f)
        out = dst.view(n, D)
        for c0 in range(0, n, 256):
            assert bool((out[c0:c0 + 256] == ref[torch.from_numpy(order[c0:c0 + 256]).to(dev)]).all().item()), (name, f)
    ms = {0: [], flag: []}
    for _ in range(steps):  # alternating, so drift hits both alike
        for f in (0, flag):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            bc.decode(meta, packed, stream=stream, flags=f)
            b.record(stream)
            torch.cuda.synchronize()
            ms[f].append(a.elapsed_time(b))
    assert (packed.status == 0).all().item()
    plain, ver = float(np.median(ms[0])), float(np.median(ms[flag]))
    extra = max(ver - plain, 1e-6)
    print("RESULT " + json.dumps({
        "workload": desc_txt, "chunks": n, "chunk_bytes": D, "steps": steps,
        "plain_ms": round(plain, 4), "verify_ms": round(ver, 4),
        "plain_ms_min_max": [round(min(ms[0]), 4), round(max(ms[0]), 4)],
        "verify_ms_min_max": [round(min(ms[flag]), 4), round(max(ms[flag]), 4)],
        "plain_gib_s": round(n * D / GIB / (plain * 1e-3), 2), "verify_gib_s": round(n * D / GIB / (ver * 1e-3), 2),
        "verify_pass_ms": round(ver - plain, 4), "verify_pass_gib_s_of_D": round(n * D / GIB / (extra * 1e-3), 2),
        "ratio_verify_to_plain": round(ver / plain, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cost.json"))
    ap.add_argument("--raw-gbs", type=float, default=2750.0,
                    help="the raw codec's rate on this part in GB/s (README: 2.7-2.8 TB/s)")
    ap.add_argument("--only", default=None, help="comma-separated configurations to run (default: all)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        (child_zlib if CONFIGS[args.child][0] == "zlib" else child)(args.child, args.steps, args.warmup)
        return 0
    res = {"source": "tools/verify_cost.py", "raw_codec_gbs": args.raw_gbs, "configs": {}}
    only = args.only.split(",") if args.only else list(CONFIGS)
    for name, (codec, _, _, limit) in CONFIGS.items():
        if name not in only:
            continue
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps),
                                "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result inside {limit} s; stopping", file=sys.stderr)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{name}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        r = json.loads(line[-1][7:])
        if codec == "gzip":  # the CRC pass reads D once; the raw codec reads and writes D
            r["crc_pass_gbs"] = round(r["chunks"] * r["chunk_bytes"] / 1e9 / (max(r["verify_pass_ms"], 1e-6) * 1e-3), 1)
            r["crc_pass_frac_of_raw_codec"] = round(r["crc_pass_gbs"] / args.raw_gbs, 4)
        res["configs"][name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
