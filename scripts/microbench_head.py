"""Microbench the fused classifier head (csrc/head.hip) against the
unfused chain at the flagship head shape (16384 x 256 -> 10), and the
rows-per-block arms of both kernels.  Needs a GPU.

Times are host wall time over back-to-back launches ending in a device
synchronise (best of 3 x 300 calls), so they include the launch floor
and are comparable among the arms, not with profiler kernel times."""
import sys
import time

import torch

sys.path.insert(0, ".")
from shallowspeed_amd.ops import load_ext  # noqa: E402

e = load_ext(required=True)
dev = torch.device("cuda", 0)
empty = torch.Tensor()


def bench(fn, iters=300, reps=3):
    best = float("inf")
    for _ in range(reps):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters * 1e6)
    return best  # us


M, K, C = 16384, 256, 10
g = torch.Generator().manual_seed(0)
x = torch.randn(M, K, generator=g).to(dev).bfloat16()
w = (torch.randn(C, K, generator=g) * K ** -0.5).to(dev).bfloat16()
b = torch.zeros(C, device=dev).bfloat16()
w_t = w.t().contiguous()
t = torch.zeros(M, C)
t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
t = t.to(dev).bfloat16()
gw = torch.zeros(C, K, device=dev)
gb = torch.zeros(C, device=dev)

probs = e.softmax_fwd(e.gemm_nt(x, w, b, empty, False))
dz = e.head_xent_bwd(probs, t, float(M))

print(f"head shape M={M} K={K} C={C}")
us = bench(lambda: e.softmax_fwd(e.gemm_nt(x, w, b, empty, False)))
print(f"fwd unfused gemm_nt + softmax_fwd        : {us:6.1f} us")
for rb in (32, 64, 128):
    us = bench(lambda: e.head_fwd_fused(x, w, b, rb))
    print(f"fwd fused, {rb:3d} rows/block              : {us:6.1f} us")


def unfused_bwd():
    d = e.head_xent_bwd(probs, t, float(M))
    e.gemm_nt(d, w_t, empty, empty, False)
    e.wgrad_tn(d, x, gw, gb, empty, 0)


us = bench(unfused_bwd)
print(f"bwd unfused xent_bwd + dgrad + wgrad_tn  : {us:6.1f} us")
us = bench(lambda: e.wgrad_tn(dz, x, gw, gb, empty, 0))
print(f"    wgrad_tn alone                       : {us:6.1f} us")
for rb in (32, 64, 128):
    us = bench(lambda: e.head_bwd_fused(probs, t, x, w_t, float(M), gw, gb,
                                        rb))
    print(f"bwd fused with wgrad, {rb:3d} rows/block   : {us:6.1f} us")
for rb in (32, 64, 128):
    us = bench(lambda: e.head_bwd_fused(probs, t, x, w_t, float(M), empty,
                                        empty, rb))
    print(f"bwd fused, no wgrad, {rb:3d} rows/block    : {us:6.1f} us")


def split_bwd():
    d, _ = e.head_bwd_fused(probs, t, x, w_t, float(M), empty, empty, 64)
    e.wgrad_tn(d, x, gw, gb, empty, 0)


us = bench(split_bwd)
print(f"bwd fused(no wgrad, 64) + wgrad_tn       : {us:6.1f} us")

# training metrics: the accumulator's slot count S (a block adds into
# slot blockIdx % S), in the fused backward and as the standalone launch
acc = torch.zeros(256, 4, dtype=torch.int32, device=dev)
for rb in (32, 64):
    us = bench(lambda: e.head_bwd_fused(probs, t, x, w_t, float(M), empty,
                                        empty, rb))
    print(f"bwd fused, no wgrad, {rb:3d} rows, no metrics : {us:6.1f} us")
    for S in (1, 16, 256):
        us = bench(lambda: e.head_bwd_fused(probs, t, x, w_t, float(M),
                                            empty, empty, rb, acc, S))
        print(f"bwd fused, no wgrad, {rb:3d} rows, S = {S:3d}    : "
              f"{us:6.1f} us")
for S in (1, 16, 256):
    a = acc[:S]
    us = bench(lambda: e.head_metrics(probs, t, a, "xent"))
    print(f"head_metrics standalone, xent, S = {S:3d}    : {us:6.1f} us")
us = bench(lambda: e.head_metrics(probs, t, acc[:16], "mse"))
print(f"head_metrics standalone, mse,  S =  16    : {us:6.1f} us")


def bwd_then_metrics():
    e.head_bwd_fused(probs, t, x, w_t, float(M), empty, empty, 32)
    e.head_metrics(probs, t, acc[:16], "xent")


us = bench(bwd_then_metrics)
print(f"bwd fused(32, no metrics) + head_metrics : {us:6.1f} us")
