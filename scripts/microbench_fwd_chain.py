"""Microbench the forward chain kernel (csrc/fwd_chain.hip) at the
flagship shape (16384 rows, 256 wide, 10 classes) against the launches
it replaces.  Needs a GPU.

  from h1     two 256-wide layers + head from the stored h1, every
              (rows, waves) arm, against 2 x gemm_nt + head_fwd_fused
  from x      the 784-wide layer streamed + two layers + head, every
              arm, against 3 x gemm_nt + head_fwd_fused, and against
              gemm_nt for the first layer + the shipped chain from h1

Times are device-event time over back-to-back launches (launch gaps
included), per call in µs; the arms alternate inside every round and
the table gives the best and the median round, so they compare with one
another, not with profiler kernel times.

  starts      the shipped eight-wave arms from x, the K loops side by
              side (kloop 1 = B one step ahead, 2 = three steps ahead),
              at M = 16384, 32768 (two rounds of 64-row tiles) and 4096
              (32 rows), with and without the gradient buffer's zeros
              riding in the launch (against the memset launch)"""
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
              f"{statistics.median(ts):6.1f}  max {max(ts):6.1f} us")


M, H, C, IN0 = 16384, 256, 10, 784
g = torch.Generator().manual_seed(0)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


x = rnd(M, IN0)
w1, b1 = rnd(H, IN0, scale=IN0 ** -0.5), rnd(H, scale=0.1)
ws = [rnd(H, H, scale=H ** -0.5) for _ in range(2)]
bs = [rnd(H, scale=0.1) for _ in range(2)]
w_head, b_head = rnd(C, H, scale=H ** -0.5), rnd(C, scale=0.1)
h1 = e.gemm_nt(x, w1, b1, empty, True)
ARMS = ((32, 4), (32, 8), (64, 4), (64, 8))


def replaced_from_h1():
    h = e.gemm_nt(h1, ws[0], bs[0], empty, True)
    h = e.gemm_nt(h, ws[1], bs[1], empty, True)
    return e.head_fwd_fused(h, w_head, b_head)


def replaced_from_x():
    h = e.gemm_nt(x, w1, b1, empty, True)
    h = e.gemm_nt(h, ws[0], bs[0], empty, True)
    h = e.gemm_nt(h, ws[1], bs[1], empty, True)
    return e.head_fwd_fused(h, w_head, b_head)


def gemm_then_chain():
    h = e.gemm_nt(x, w1, b1, empty, True)
    return F.fwd_chain(h, ws, bs, w_head, b_head, 64, 8, l1=1)


print(f"forward from h1, M={M} H={H} C={C}")
arms = {"2 x gemm_nt + head_fwd_fused": replaced_from_h1}
for arm in ARMS:
    arms["chain from h1 rows=%d waves=%d" % arm] = (
        lambda a=arm: F.fwd_chain(h1, ws, bs, w_head, b_head, *a, l1=1))
bench(arms)

print(f"forward from x, M={M} in={IN0} H={H} C={C}")
arms = {"3 x gemm_nt + head_fwd_fused": replaced_from_x,
        "gemm_nt + chain from h1 rows=64 waves=8": gemm_then_chain}
for arm in ARMS:
    arms["chain from x rows=%d waves=%d" % arm] = (
        lambda a=arm: F.fwd_chain(x, [w1] + ws, [b1] + bs, w_head, b_head,
                                  *a, l1=2))
bench(arms)

# the flagship's flat gradient buffer: 335114 floats
grads = torch.empty(784 * 256 + 2 * 256 * 256 + 2560 + 3 * 256 + 10,
                    device=dev)
for m, rows in ((16384, 64), (32768, 64), (4096, 32)):
    xm = rnd(m, IN0)
    print(f"starts from x, M={m} rows={rows} waves=8")
    arms = {}
    for kloop in (1, 2):
        arms[f"l1=2 kloop={kloop}"] = (
            lambda k=kloop: F.fwd_chain(xm, [w1] + ws, [b1] + bs, w_head,
                                        b_head, rows, 8, l1=2, kloop=k))
    arms["grads.zero_() + l1=2 kloop=2"] = (
        lambda: (grads.zero_(),
                 F.fwd_chain(xm, [w1] + ws, [b1] + bs, w_head, b_head, rows,
                             8, l1=2, kloop=2)))
    arms["l1=2 kloop=2 zero=grads"] = (
        lambda: F.fwd_chain(xm, [w1] + ws, [b1] + bs, w_head, b_head, rows,
                            8, l1=2, kloop=2, zero=grads))
    bench(arms)
