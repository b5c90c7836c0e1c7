"""Microbench the unmasked wgrad of the flagship's layer shapes on MI355X:
one LDS staging set against two (wgrad_tn's `stages` argument), over the
split sweep of profiles/r03_wgrad_onchip_reduce.md §2.

    python scripts/microbench_wgrad_group.py [--rounds 5] [--iters 200]
        [--only all|stages|group] [--cells "6,16;7,8"]

Each (shape, split) cell times both depths alternately, `rounds` times
each, and prints the min / median / max of the per-call time in µs, so a
difference can be read against the cell's own spread.  The next block
times the four launches of one flagship step back to back.

The last block (alone with --only group) is the grouped launch
(wgrad_tn_group): the head and the two hidden layers of a step, each
with operands and gradients of its own, in ONE launch, over hidden split
x head split x head first / last in the grid, each cell against the
three launches back to back at the launcher's splits.
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.ops import load_ext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--only", choices=["all", "stages", "group"], default="all")
ap.add_argument("--cells", default="",
                help="grouped launch: 'hidden,head;...' split pairs to time "
                     "instead of the full sweep")
args = ap.parse_args()

e = load_ext(required=True)
dev = torch.device("cuda", 0)
empty = torch.Tensor()


def timed(fn):
    """µs per call over args.iters calls, device events."""
    for _ in range(10):
        fn()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / args.iters


def cell(fns):
    """Alternate the arms, args.rounds each: {arm: (min, median, max)}."""
    got = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn))
    return {k: (min(v), statistics.median(v), max(v)) for k, v in got.items()}


def fmt(t):
    return f"{t[0]:6.1f} / {t[1]:6.1f} / {t[2]:6.1f}"


Kb = args.batch
# (Mo, N): first layer, hidden, head
layers = [(256, 784), (256, 256), (10, 256)]
ops = []
for Mo, N in layers:
    g = torch.Generator().manual_seed(Mo * 1000 + N)
    dy = torch.randn(Kb, Mo, generator=g).to(dev).bfloat16()
    x = torch.randn(Kb, N, generator=g).to(dev).bfloat16()
    gw = torch.zeros(Mo, N, device=dev)
    gb = torch.zeros(Mo, device=dev)
    ops.append((dy, x, gw, gb))

print(f"wgrad_tn unmasked, Kb = {Kb}; µs per call as min / median / max "
      f"of {args.rounds} rounds x {args.iters} calls")
if args.only != "group":
    print("| Mo x N | split | stages 1 | stages 2 |")
    print("|---|---:|---|---|")
for (Mo, N), (dy, x, gw, gb) in zip(layers if args.only != "group" else [],
                                    ops):
    for sk in (0, 8, 16, 32, 64):
        r = cell({
            s: (lambda s=s: e.wgrad_tn(dy, x, gw, gb, empty, sk, s))
            for s in (1, 2)
        })
        print(f"| {Mo} x {N} | {sk} | {fmt(r[1])} | {fmt(r[2])} |")


def step(stages):
    # backward order: head, third, second, first layer
    for i in (2, 1, 1, 0):
        dy, x, gw, gb = ops[i]
        e.wgrad_tn(dy, x, gw, gb, empty, 0, stages)


if args.only != "group":
    print("\nthe four wgrads of one step, auto split, back to back")
    print("| arm | µs per step (min / median / max) |")
    print("|---|---|")
    arms = {
        "stages 1 everywhere": lambda: step(1),
        "stages 2 everywhere": lambda: step(2),
        "launcher's choice": lambda: step(0),
    }
    for k, v in cell(arms).items():
        print(f"| {k} | {fmt(v)} |")

if args.only == "stages":
    sys.exit(0)


# ---- grouped launch: head + two hidden layers, separate buffers each
def problem(Mo, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Kb, Mo, generator=g).to(dev).bfloat16(),
            torch.randn(Kb, N, generator=g).to(dev).bfloat16(),
            torch.zeros(Mo, N, device=dev), torch.zeros(Mo, device=dev))


head, hid3, hid2 = problem(10, 256, 1), problem(256, 256, 2), \
    problem(256, 256, 3)


def three_launches():
    for dy, x, gw, gb in (head, hid3, hid2):
        e.wgrad_tn(dy, x, gw, gb, empty, 0, 0)


shapes = [(Kb, 10, 256), (Kb, 256, 256), (Kb, 256, 256)]
rule = e.wgrad_group_plan(shapes, None)
print(f"\nhead + 2 hidden wgrads, own buffers each; the group rule plans "
      f"{rule}")
print("| hidden split | head split | head | blocks | three launches | "
      "one grouped launch |")
print("|---:|---:|---|---:|---|---|")
sweep = [(hs, ks) for hs in (0, 4, 6, 8, 12, 16)
         for ks in ((0,) if hs == 0 else (8, 16, 32, 64))]
if args.cells:
    sweep = [tuple(int(v) for v in c.split(",")) for c in args.cells.split(";")]
for hs, ks in sweep:  # 0, 0 = the launcher's rule
    for first in (True, False):
        probs = [head, hid3, hid2] if first else [hid3, hid2, head]
        splits = [ks, hs, hs] if first else [hs, hs, ks]
        sh = shapes if first else shapes[1:] + shapes[:1]
        blocks = sum(e.wgrad_group_plan(sh, splits)[0][2])
        r = cell({
            "three": three_launches,
            "group": lambda: e.wgrad_tn_group(probs, splits),
        })
        print(f"| {hs} | {ks} | {'first' if first else 'last'} | "
              f"{blocks} | {fmt(r['three'])} | {fmt(r['group'])} |")
