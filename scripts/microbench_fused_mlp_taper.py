"""Microbench the mixed-width fused serving forward
(csrc/fused_mlp_taper.hip) on 784,512,256,128,10 and 784,1024,256,10 at
M = 1024 and 16384, every built (rows, waves) arm the widths can take,
against the per-layer serving path such a model took before:

  per layer   one gemm_nt (bias, ReLU) per hidden layer + the head's
              gemm_nt + row_argmax

Times are device-event time over back-to-back launches (launch gaps
included), per call in µs; the arms alternate inside every round and the
table gives the best, the median and the slowest round.  The last line of
a shape compares the best arm's median with the per-layer median and with
five times the larger of the two (max - best) spreads, the bar for
shipping the shape class switched on.  Needs a GPU."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.ops import functional as F  # noqa: E402

dev = torch.device("cuda", 0)
ITERS, ROUNDS = 200, 7
g = torch.Generator().manual_seed(0)


def bench(arms):
    """arms: {name: fn}; every round times each arm once, in turn."""
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / ITERS * 1e3)
    for name, ts in times.items():
        print(f"{name:36s}: best {min(ts):6.1f}  median "
              f"{statistics.median(ts):6.1f}  max {max(ts):6.1f} us")
    return times


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


for sizes in ([784, 512, 256, 128, 10], [784, 1024, 256, 10]):
    widths = sizes[1:-1]
    ws = [rnd(o, i, scale=i ** -0.5) for i, o in zip(sizes, sizes[1:])]
    bs = [rnd(o, scale=0.5) for o in sizes[1:]]
    for M in (1024, 16384):
        x = rnd(M, sizes[0])

        def per_layer():
            h = x
            for w, b in zip(ws[:-1], bs[:-1]):
                h = F.linear_fwd(h, w, b, relu=True)
            return F.row_argmax(F.linear_fwd(h, ws[-1], bs[-1]))

        print("model", ",".join(map(str, sizes)), "M =", M)
        arms = {"per layer": per_layer}
        for arm in F.FUSED_MLP_TAPER_ARMS[max(widths)]:
            if min(widths) // arm[1] >= 16:
                arms["fused_mlp_taper rows=%d waves=%d" % arm] = (
                    lambda a=arm: F.fused_mlp_forward(x, ws, bs, rows=a[0],
                                                      waves=a[1]))
        same = (per_layer() == F.fused_mlp_forward(x, ws, bs)).sum().item()
        print(f"argmax equal to the per-layer path's in {same} of {M} rows")
        times = bench(arms)
        base = times.pop("per layer")
        best = min(times, key=lambda k: statistics.median(times[k]))
        spread = max(max(t) - min(t) for t in (base, times[best]))
        gain = statistics.median(base) - statistics.median(times[best])
        print(f"  best: {best}; gain {gain:.1f} us over per layer, 5 x spread "
              f"{5 * spread:.1f} us -> {'on' if gain > 5 * spread else 'off'}")
