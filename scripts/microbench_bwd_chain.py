"""Microbench the backward chain kernel (csrc/bwd_chain.hip) at the
flagship shape (16384 rows, 256 wide, 10 classes) against the launches
it replaces, and the masked against the unmasked weight gradient that
follows it.  Needs a GPU.

  chain arms      (rows, waves, W^T from L2 or through LDS)
                  x {dz_1 emitted, chain stops at dh_1}
  replaced chain  head_bwd_fused + 2 x gemm_nt with the fused ReLU mask
  wgrad_tn        masked (dh, h) against unmasked (dz) at
                  16384 x 256 x 256 and 16384 x 256 x 784

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


M, H, C, IN0 = 16384, 256, 10, 784
g = torch.Generator().manual_seed(0)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev).bfloat16()


probs = torch.softmax(torch.randn(M, C, generator=g), 1).to(dev).bfloat16()
t = torch.zeros(M, C)
t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
t = t.to(dev).bfloat16()
w_head_t = rnd(C, H, scale=H ** -0.5).t().contiguous()
hs = [torch.relu(rnd(M, H)) for _ in range(3)]  # h3, h2, h1
w_ts = [rnd(H, H, scale=H ** -0.5).t().contiguous() for _ in range(2)]
x_head = hs[0]


def replaced():
    _, dh = e.head_bwd_fused(probs, t, x_head, w_head_t, float(M), empty,
                             empty)
    dh = e.gemm_nt(dh, w_ts[0], empty, hs[0], False)
    return e.gemm_nt(dh, w_ts[1], empty, hs[1], False)


print(f"backward data path, M={M} H={H} C={C}")
arms = {"head_bwd_fused + 2 x masked gemm_nt": replaced}
for arm in ((32, 4, 0), (32, 8, 0), (64, 4, 0), (64, 8, 0), (64, 8, 1)):
    name = "chain rows=%d waves=%d%s" % (arm[0], arm[1],
                                         " W via LDS" if arm[2] else "")
    arms[name + ", dz_1 emitted"] = (
        lambda a=arm: F.bwd_chain(probs, t, w_head_t, M, hs, w_ts, *a))
    arms[name + ", stops at dh_1"] = (
        lambda a=arm: F.bwd_chain(probs, t, w_head_t, M, hs[:2], w_ts, *a))
bench(arms)

# the weight gradients that follow: masked on dh (today) against
# unmasked on dz (after the chain); same values, so dz = dh * mask
dh = rnd(M, H, scale=1e-3)
dz = e.relu_bwd(dh, hs[2])
for n_in in (H, IN0):
    x = rnd(M, n_in)
    gw = torch.zeros(H, n_in, device=dev)
    gb = torch.zeros(H, device=dev)
    print(f"wgrad_tn {M} x {H} x {n_in}")
    bench({
        "wgrad_tn masked (dh, h)": lambda: e.wgrad_tn(dh, x, gw, gb, hs[2], 0),
        "wgrad_tn unmasked (dz)": lambda: e.wgrad_tn(dz, x, gw, gb, empty, 0),
    })
