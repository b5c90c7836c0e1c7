"""Microbench the wide chain kernels (csrc/fwd_chain_wide.hip,
csrc/bwd_chain_wide.hip) at H = 128 and 512, M = 1024 and 16384, in_dims
784, three ReLU layers, 10 classes, every built (rows, waves) arm,
against the per-layer launches they replace:

  forward   3 x gemm_nt + head_fwd_fused
  backward  head_bwd_fused + 3 x relu_bwd + 2 x gemm_nt (the first
            layer's dgrad is not in the chain)

Times are device-event time over back-to-back launches (launch gaps
included), per call in µs; the arms alternate inside every round and the
table gives the best, the median and the slowest round.  Needs a GPU."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.ops import functional as F  # noqa: E402
from shallowspeed_amd.ops import load_ext  # noqa: E402

e = load_ext(required=True)
dev = torch.device("cuda", 0)
empty = torch.Tensor()
ITERS, ROUNDS = 100, 5
C, IN0, N, GB = 10, 784, 3, 16384
g = torch.Generator().manual_seed(0)


def bench(arms):
    """arms: {name: fn}; every round times each arm once, in turn."""
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(10):
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


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


for H in F.CHAIN_WIDE_WIDTHS:
    for M in (1024, 16384):
        x = rnd(M, IN0)
        dims = [IN0] + [H] * N
        ws = [rnd(H, dims[l], scale=dims[l] ** -0.5) for l in range(N)]
        bs = [rnd(H, scale=0.1) for _ in range(N)]
        w_head, b_head = rnd(C, H, scale=H ** -0.5), rnd(C, scale=0.1)
        w_head_t = w_head.t().contiguous()
        w_ts = [w.t().contiguous() for w in ws[:0:-1]]  # top first
        target = torch.zeros(M, C)
        target[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
        target = target.to(dev).bfloat16()
        hs, probs = F.fwd_chain_wide(x, ws, bs, w_head, b_head)
        hs_top = hs[::-1]

        def fwd_layers():
            h = x
            for w, b in zip(ws, bs):
                h = e.gemm_nt(h, w, b, empty, True)
            return e.head_fwd_fused(h, w_head, b_head)

        def bwd_layers():
            _, dh = e.head_bwd_fused(probs, target, hs_top[0], w_head_t,
                                     float(GB), empty, empty)
            for l in range(N):
                dz = e.relu_bwd(dh, hs_top[l])
                if l < len(w_ts):
                    dh = e.gemm_nt(dz, w_ts[l], empty, empty, False)

        print(f"H={H} M={M} in={IN0} layers={N} C={C}")
        arms = {"forward per layer": fwd_layers,
                "backward per layer": bwd_layers}
        for arm in F.CHAIN_WIDE_ARMS[H]:
            arms["fwd_chain_wide rows=%d waves=%d" % arm] = (
                lambda a=arm: F.fwd_chain_wide(x, ws, bs, w_head, b_head, *a))
            arms["bwd_chain_wide rows=%d waves=%d" % arm] = (
                lambda a=arm: F.bwd_chain_wide(probs, target, w_head_t, GB,
                                               hs_top, w_ts, *a))
        bench(arms)
