"""Microbench dropout at the flagship shapes.  Needs a GPU.

  hidden forward  16384 x 256 x 256, bias + ReLU:
                  plain gemm_nt
                  dropout in the epilogue (one Philox call per
                    fragment, shared inside the lane quads)
                  plain gemm_nt + standalone dropout_fwd pass
  backward chain  16384 x 256, C = 10: unscaled against scaled dz

Times are device-event time over back-to-back launches (launch gaps
included), per call in µs; the arms alternate inside every round and
the table gives the best and the median round, so they compare with one
another, not with profiler kernel times."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.ops import functional as F  # noqa: E402
from shallowspeed_amd.ops import load_ext  # noqa: E402

e = load_ext(required=True)
dev = torch.device("cuda", 0)
empty = torch.Tensor()
ITERS, ROUNDS = 200, 7


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
        print(f"{name:44s}: best {min(ts):6.1f}  median "
              f"{statistics.median(ts):6.1f} us")


M, H, C = 16384, 256, 10
g = torch.Generator().manual_seed(0)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


x = rnd(M, H)
w = rnd(H, H, scale=H ** -0.5)
b = rnd(H, scale=0.1)
P = 0.1
key = (0x5EED, 3, 1, 0, 1, P)  # seed, step, layer, row_first, stride, p

print(f"hidden forward {M} x {H} x {H}, bias + ReLU, p = {P}")
bench({
    "gemm_nt plain": lambda: e.gemm_nt(x, w, b, empty, True),
    "epilogue, Philox per fragment (quad-shared)":
        lambda: F.linear_fwd_dropout(x, w, b, *key),
    "gemm_nt + standalone dropout_fwd": lambda: F.linear_fwd_dropout(
        x, w, b, *key, fused=False),
})

probs = torch.softmax(torch.randn(M, C, generator=g), 1).to(dev).bfloat16()
t = torch.zeros(M, C)
t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
t = t.to(dev).bfloat16()
w_head_t = rnd(C, H, scale=H ** -0.5).t().contiguous()
hs = [torch.relu(rnd(M, H)) for _ in range(3)]
w_ts = [rnd(H, H, scale=H ** -0.5).t().contiguous() for _ in range(2)]
scale = F.dropout_params(P)[1]

print(f"backward chain, M={M} H={H} C={C}, three layers, dz_1 emitted")
bench({
    "chain unscaled": lambda: F.bwd_chain(probs, t, w_head_t, M, hs, w_ts),
    "chain scaled": lambda: F.bwd_chain(probs, t, w_head_t, M, hs, w_ts,
                                        dz_scale=scale),
})
