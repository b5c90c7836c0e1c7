#!/usr/bin/env python3
"""Time the ordered grouped wgrad (one partial launch + one tree fold per
planned launch) at the flagship layer shapes, next to the per-layer
ordered path (partial + serial fold per layer) and the default grouped
launch (atomics), with the fold's W arms side by side.

    python scripts/microbench_wgrad_group_ordered.py [--iters 200]
        [--warmup 20] [--splits 6,16,64] [--eager] [--only CASE]

One JSON line per (case, arm): µs per call by device events.  The calls
are captured into one graph of 20 and replayed, so the host's launch
rate is out of the number; --eager times back-to-back calls instead,
which is the form to put under `rocprofv3 --kernel-trace --stats` (with
a small --iters) for per-kernel times.

Cases: the head + two hidden layers (one planned launch), the first
layer (a run of one), all four (a step's weight gradients), and each
layer alone at the explicit --splits (the fold against the split).
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KB = 16384
HEAD, HIDDEN, FIRST = (KB, 10, 256), (KB, 256, 256), (KB, 256, 784)
PER_GRAPH = 20


def timed(fn, iters, warmup, eager):
    for _ in range(warmup):
        fn()
    run, n = fn, iters
    if not eager:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(PER_GRAPH):
                fn()
        run, n = graph.replay, max(1, iters // PER_GRAPH)
        run()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (n if eager else n * PER_GRAPH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--splits", default="6,16,64")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--only", default=None, help="run this case alone")
    args = ap.parse_args()
    from shallowspeed_amd.ops import load_ext

    ext = load_ext(required=True)
    dev = torch.device("cuda", 0)
    empty = torch.Tensor()

    def problem(shape, seed):
        Kb, Mo, N = shape
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(Kb, Mo, generator=g).to(dev, torch.bfloat16),
                torch.randn(Kb, N, generator=g).to(dev, torch.bfloat16),
                torch.zeros(Mo, N, device=dev), torch.zeros(Mo, device=dev))

    def report(case, arm, fn, **extra):
        us = timed(fn, args.iters, args.warmup, args.eager)
        print(json.dumps(dict(case=case, arm=arm, us=round(us, 2), **extra)),
              flush=True)

    def arms(case, probs, splits):
        if args.only not in (None, case):
            return
        shapes = [(p[0].shape[0], p[0].shape[1], p[1].shape[1]) for p in probs]
        launches, ws = ext.wgrad_group_ordered_plan(shapes, splits)
        plan = dict(splits=[list(la[1]) for la in launches],
                    blocks=[list(la[2]) for la in launches], workspace=ws)
        if splits is None:
            report(case, "atomics-grouped", lambda: ext.wgrad_tn_group(probs))
        per_layer = splits or [0] * len(probs)
        report(case, "ordered-per-layer", lambda: [
            ext.wgrad_tn_ordered(dy, x, gw, gb, empty, s)
            for (dy, x, gw, gb), s in zip(probs, per_layer)])
        for waves in (4, 8, 16):
            report(case, f"grouped-ordered-W{waves}",
                   lambda: ext.wgrad_tn_group_ordered(probs, splits, waves),
                   **plan)

    head, h1, h2, first = (problem(s, k) for k, s in
                           enumerate((HEAD, HIDDEN, HIDDEN, FIRST)))
    arms("head+hidden+hidden", [head, h1, h2], None)
    arms("first", [first], None)
    arms("step", [head, h1, h2, first], None)
    for split in (int(s) for s in args.splits.split(",")):
        for name, p in (("head", head), ("hidden", h1), ("first", first)):
            arms(f"{name}@{split}", [p], [split])


if __name__ == "__main__":
    main()
