#!/usr/bin/env python3
"""Token-level model of the wave inflate kernel's stage rule (zcg_inflate_wave.hip,
L phase) at one or more stage capacities, on one C2 chunk.  CPU only (zlib and
tools/deflate_tokens.py): it reprices the far / near shift of a larger or
smaller ring for other data without a GPU.

The rule: the chain's tokens are taken in groups of 128; a group that does not
fit whole into a stage that already has bytes is rejected and starts the next
stage (a stage that is empty takes the tokens that fit); a match's far part is
its first d - o bytes (o = its offset in the stage; sources before the stage,
copied from the committed output), the rest is its near part (resolved in
batches of 64 bytes per group, one batch run per group); far parts go out in
batches of 64 per group.  A stage also ends where an H round ends; the model
ends one at every block end (zlib closes a block after `--block-tokens` tokens,
16 383 at memLevel 8) and leaves further rounds inside a block out, so it
counts a stage or two per chunk fewer than the kernel (602 for 603.3 measured at
capacity 2 032).
  usage: stage_model.py [--chunk I] [--level L] [--block-tokens T] [capacity ...]   (default 2032 3056 4080)"""
import argparse
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import quant_chunk  # noqa: E402
from deflate_tokens import tokens  # noqa: E402


def model(tk, cap, block_tokens):
    r = dict(capacity=cap, stages=0, rejected_groups=0, groups=0, far_parts=0, far_bytes=0, near_bytes=0,
             near_batches=0, far_batches=0, literals=0)
    i, n = 0, len(tk)
    while i < n:
        blk_end = min(n, (i // block_tokens + 1) * block_tokens)
        r["stages"] += 1
        emitted = 0
        while i < blk_end:
            grp = tk[i:min(i + 128, blk_end)]
            e, take = emitted, 0
            for t in grp:
                ln = 1 if t[0] == 'L' else t[1]
                if e + ln > cap:
                    break
                e, take = e + ln, take + 1
            if take < len(grp) and emitted:
                r["rejected_groups"] += 1
                break
            r["groups"] += 1
            o, far, near = emitted, 0, 0
            for t in grp[:take]:
                if t[0] == 'L':
                    r["literals"] += 1
                    o += 1
                    continue
                ln, d = t[1], t[2]
                fl = min(ln, d - o) if o < d else 0
                if fl:
                    far += 1
                    r["far_bytes"] += fl
                near += ln - fl
                o += ln
            r["far_parts"] += far
            r["near_bytes"] += near
            r["far_batches"] += max(1, -(-far // 64))  # (the first batch runs even when it is empty)
            r["near_batches"] += -(-near // 64)
            emitted, i = e, i + take
            if take < len(grp):
                break
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--block-tokens", type=int, default=16383)
    ap.add_argument("capacity", type=int, nargs="*", default=[2032, 3056, 4080])
    a = ap.parse_args()
    v = quant_chunk(a.chunk).tobytes()
    c = zlib.compressobj(a.level, zlib.DEFLATED, -15)
    tk = tokens(c.compress(v) + c.flush())
    print(f"chunk {a.chunk}: {len(tk)} tokens, zlib {zlib.ZLIB_VERSION} level {a.level}")
    for cap in a.capacity:
        print(model(tk, cap, a.block_tokens))


if __name__ == "__main__":
    main()
