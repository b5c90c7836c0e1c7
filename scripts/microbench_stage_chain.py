"""Microbench the stage arms of the chain kernels (csrc/fwd_chain.hip,
csrc/bwd_chain.hip) on pipeline stages that have no loss head.  Needs a
GPU; one process, one GPU.

  stage step   forward + backward + wgrads of a stage model on a seeded
               dout, chains on against off (F.set_fwd_chain /
               F.set_bwd_chain; off is the per-layer path), for
                 pp2 stage 0 of 784,256,256,256,256,10 (784 -> 3 x 256)
                 pp3 stage 1 of an all-256 model         (256 -> 3 x 256)
               at M = 16384 and M = 4096
  bwd arms     F.bwd_chain_stage alone on the stage's stashed h, every
               (rows, waves) arm, against the masked linear_dgrad per
               layer (relu_bwd where the input gradient is skipped)

Times are device-event time over back-to-back calls (launch gaps
included), per call in µs; the arms alternate inside every round and the
table gives the best, the median and the slowest round, so they compare
with one another, not with profiler kernel times.  Run it twice to see
the spread between runs."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.models import MLP  # noqa: E402
from shallowspeed_amd.ops import functional as F  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = 5
H = 256


def bench(arms, iters):
    """arms: {name: fn}; every round times each arm once, in turn."""
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(30):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / iters * 1e3)
    for name, ts in times.items():
        print(f"  {name:40s}: best {min(ts):7.1f}  median "
              f"{statistics.median(ts):7.1f}  max {max(ts):7.1f} us",
              flush=True)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


STAGES = {
    "pp2 stage 0 (784 -> 3 x 256)": ([784, 256, 256, 256, 256, 10], 0, 2),
    "pp3 stage 1 (256 -> 3 x 256)": ([256] * 8 + [10], 1, 3)}

for name, (sizes, stage, pp) in STAGES.items():
    for M in (16384, 4096):
        model = MLP(sizes, stage, pp, M).materialize_device(dev)
        model.zero_grad()
        x = rnd(M, model.in_dim, seed=1)
        dout = rnd(M, H, seed=2, scale=1 / 64)

        def step(on):
            F.set_fwd_chain(on)
            F.set_bwd_chain(on)
            model.forward(x, 0)
            model.backward(dout, 0)

        print(f"{name}, M={M}: forward + backward + wgrads", flush=True)
        bench({"chains off (per layer)": lambda: step(False),
               "chains on (stage arms)": lambda: step(True)}, 6000)

        F.set_fwd_chain(True)
        model.forward(x, 0)
        layers = model.layers[::-1]
        hs = [l._cache[("y", 0)] for l in layers]
        dgrads = [l for l in layers
                  if not (l is model.layers[0] and model._skip_input_grad)]
        w_ts = [l.weight.compute_t() for l in dgrads]

        def per_layer():
            d = dout
            for l, h in zip(layers, hs):
                if l in dgrads:
                    d = F.linear_dgrad(d, l.weight.compute(),
                                       l.weight.compute_t(), h)
                else:
                    d = F.relu_bwd(d, h)

        print(f"{name}, M={M}: backward data path alone", flush=True)
        arms = {"masked linear_dgrad per layer": per_layer}
        for arm in ((32, 4), (32, 8), (64, 4), (64, 8)):
            arms["bwd_chain_stage rows=%d waves=%d" % arm] = (
                lambda a=arm: F.bwd_chain_stage(dout, hs, w_ts, *a))
        bench(arms, 20000)
        for l in model.layers:
            l._cache.clear()
