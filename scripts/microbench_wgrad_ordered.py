#!/usr/bin/env python3
"""Time the ordered split-K wgrad (partial kernel + fold) at the flagship
layer shapes, next to the default (atomics) and single-owner launches.

    python scripts/microbench_wgrad_ordered.py [--splits 0,8,16,32,64]
        [--iters 200] [--warmup 20]

One JSON line per (shape, path, split): µs per call by device events over
`iters` back-to-back calls, the effective split, the blocks of the
partial launch and the workspace bytes.  Per-kernel times come from a
`rocprofv3 --kernel-trace --stats` run of this script with small --iters.
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16384, 256, 784, True), (16384, 256, 256, False),
          (16384, 10, 256, False)]  # (Kb, Mo, N, masked): L1, hidden, head


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", default="0,8,16,32,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from shallowspeed_amd.ops import load_ext

    ext = load_ext(required=True)
    dev = torch.device("cuda", 0)
    empty = torch.Tensor()
    for Kb, Mo, N, masked in SHAPES:
        g = torch.Generator().manual_seed(Kb + Mo + N)
        dy = torch.randn(Kb, Mo, generator=g).to(dev, torch.bfloat16)
        x = torch.randn(Kb, N, generator=g).to(dev, torch.bfloat16)
        mask = torch.randn(Kb, Mo, generator=g).to(dev, torch.bfloat16) \
            if masked else empty
        gw = torch.zeros(Mo, N, device=dev)
        gb = torch.zeros(Mo, device=dev)
        row = dict(Kb=Kb, Mo=Mo, N=N, masked=masked)
        for path, split in (("atomic", 0), ("single", 1)):
            us = timed(lambda: ext.wgrad_tn(dy, x, gw, gb, mask, split),
                       args.iters if split != 1 else 20, args.warmup)
            print(json.dumps(dict(row, path=path, us=round(us, 2))))
        for split in (int(s) for s in args.splits.split(",")):
            eff, blocks, ws = ext.wgrad_ordered_plan(Kb, Mo, N, split)
            us = timed(lambda: ext.wgrad_tn_ordered(dy, x, gw, gb, mask,
                                                    split),
                       args.iters, args.warmup)
            print(json.dumps(dict(row, path="ordered", split=split, eff=eff,
                                  blocks=blocks, workspace=ws,
                                  us=round(us, 2))), flush=True)


if __name__ == "__main__":
    main()
