"""Microbench the wide chain kernels (csrc/fwd_chain_wide.hip,
csrc/bwd_chain_wide.hip) at H = 128 and 512, M = 1024 and 16384, in_dims
784, three ReLU layers, 10 classes, every built (rows, waves) arm,
against the per-layer launches they replace:

  forward   3 x gemm_nt + head_fwd_fused
  backward  head_bwd_fused + 3 x relu_bwd + 2 x gemm_nt (the first
            layer's dgrad is not in the chain)

Times are device-event time over back-to-back launches (launch gaps
included), per call in µs; the arms alternate inside every round and the
table gives the best, the median and the slowest round.  Needs a GPU.

  python scripts/microbench_chain_wide.py dropout
              the same shapes with p = 0.2 on every ReLU layer: the
              per-layer path against fwd_chain_wide_dropout and
              bwd_chain_wide(dz_scale), both kernels and the training
              step (profiles/r24_chain_wide_dropout.md)
  python scripts/microbench_chain_wide.py stage [H M]
              the stage arms, for a pipeline stage with no head: every
              arm and both starts against the per-layer launches, p = 0
              and 0.2, and the stage step with the wide chains off and on
              (profiles/r25_chain_wide_stage.md); H M: that shape only"""
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


def dropout_section():
    """`dropout`: p = 0.2 on every ReLU layer, per width and batch, the
    shipped arm.  Forward: 3 x gemm_nt_dropout + head_fwd_fused against
    fwd_chain_wide_dropout, and fwd_chain_wide to price the mask.
    Backward: head_bwd_fused + 3 x relu_bwd(scale) + 2 x gemm_nt against
    bwd_chain_wide(dz_scale), and the unscaled launch.  Step: zero_grad,
    forward, backward, SGD of one model, F.set_chain_wide_dropout off
    against on (the wide chains themselves switched on for both)."""
    from shallowspeed_amd.models import MLP, SGD

    p, seed, layers = 0.2, 0x1234567887654321, (0, 1, 2)
    thr, scale = F.dropout_params(p)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    F.set_chain_wide(True)
    for H in F.CHAIN_WIDE_WIDTHS:
        for M in (1024, 16384):
            x = rnd(M, IN0)
            dims = [IN0] + [H] * N
            ws = [rnd(H, dims[l], scale=dims[l] ** -0.5) for l in range(N)]
            bs = [rnd(H, scale=0.1) for _ in range(N)]
            w_head, b_head = rnd(C, H, scale=H ** -0.5), rnd(C, scale=0.1)
            w_head_t = w_head.t().contiguous()
            w_ts = [w.t().contiguous() for w in ws[:0:-1]]  # top first
            target = torch.eye(C)[torch.arange(M) % C].to(dev).bfloat16()
            key = (seed, 7, layers, (p,) * N, 0, 1)
            hs, probs = F.fwd_chain_wide_dropout(x, ws, bs, w_head, b_head,
                                                 *key)
            hs_top = hs[::-1]

            def fwd_layers():
                h = x
                for l, w, b in zip(layers, ws, bs):
                    h = e.gemm_nt_dropout(h, w, b, k0, k1, 7, l, 0, 1, thr,
                                          scale, True)
                return e.head_fwd_fused(h, w_head, b_head)

            def bwd_layers():
                _, dh = e.head_bwd_fused(probs, target, hs_top[0], w_head_t,
                                         float(GB), empty, empty)
                for l in range(N):
                    dz = F.relu_bwd(dh, hs_top[l], scale=scale)
                    if l < len(w_ts):
                        dh = e.gemm_nt(dz, w_ts[l], empty, empty, False)

            print(f"dropout p={p} H={H} M={M} in={IN0} layers={N} C={C}")
            bench({
                "forward per layer (dropout)": fwd_layers,
                "fwd_chain_wide_dropout": lambda: F.fwd_chain_wide_dropout(
                    x, ws, bs, w_head, b_head, *key),
                "fwd_chain_wide (no mask)": lambda: F.fwd_chain_wide(
                    x, ws, bs, w_head, b_head),
                "backward per layer (scaled)": bwd_layers,
                "bwd_chain_wide dz_scale": lambda: F.bwd_chain_wide(
                    probs, target, w_head_t, GB, hs_top, w_ts,
                    dz_scale=scale),
                "bwd_chain_wide (no scale)": lambda: F.bwd_chain_wide(
                    probs, target, w_head_t, GB, hs_top, w_ts),
            })
            model = MLP([IN0] + [H] * N + [C], 0, 1, M, dropout=p,
                        dropout_seed=seed).materialize_device(dev)
            opt = SGD(model.parameters(), lr=0.01)

            def step(on):
                F.set_chain_wide_dropout(on)
                model.zero_grad()
                model.forward(x, 0)
                model.backward(target, 0)
                opt.step()
                model.dropout_step += 1

            bench({"step, SS_CHAIN_WIDE_DROPOUT off": lambda: step(False),
                   "step, SS_CHAIN_WIDE_DROPOUT on": lambda: step(True)})
    F.set_chain_wide_dropout(False)


def stage_section(only=None):
    """`stage [H M]`: the stage arms (csrc/fwd_chain_wide_stage.hip,
    fwd_chain_wide_stage_drop.hip, bwd_chain_wide_stage.hip) per width and
    batch, three ReLU layers, no head.  Forward: 3 x gemm_nt against every
    arm, for a stage 0 (in_dims 784, streamed) and for a middle stage
    (in_dims H) under both starts.  Backward from dout: 3 x relu_bwd +
    gemm_nt against every arm, for a middle stage (three dgrads, dx out)
    and a stage 0 (two).  The same under p = 0.2 on the shipped arm.  Then
    the stage step (zero_grad, forward, backward with its wgrads) of a
    stage-0 and a middle-stage model, F.set_chain_wide off against on."""
    from shallowspeed_amd.models import MLP

    p, seed, layers = 0.2, 0x1234567887654321, (0, 1, 2)
    thr, scale = F.dropout_params(p)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    key = (seed, 7, layers, (p,) * N, 0, 1)
    for H in F.CHAIN_WIDE_WIDTHS:
        for M in (1024, 16384):
            if only and (H, M) != only:
                continue
            xs = {IN0: rnd(M, IN0), H: rnd(M, H)}
            ws = {k: [rnd(H, d, scale=d ** -0.5) for d in [k] + [H] * (N - 1)]
                  for k in xs}
            bs = [rnd(H, scale=0.1) for _ in range(N)]
            dout = rnd(M, H, scale=1 / 64)
            hs_top = F.fwd_chain_wide_stage(xs[H], ws[H], bs)[::-1]
            hd_top = F.fwd_chain_wide_stage_dropout(xs[H], ws[H], bs,
                                                    *key)[::-1]
            w_ts = [w.t().contiguous() for w in ws[H][::-1]]  # top first

            def fwd_layers(k, drop=False):
                h = xs[k]
                for l, w, b in zip(layers, ws[k], bs):
                    h = e.gemm_nt_dropout(h, w, b, k0, k1, 7, l, 0, 1, thr,
                                          scale, True) if drop \
                        else e.gemm_nt(h, w, b, empty, True)

            def bwd_layers(nw, s=1.0):
                dh = dout
                for l in range(N):
                    dz = F.relu_bwd(dh, (hd_top if s != 1.0 else hs_top)[l],
                                    scale=s)
                    if l < nw:
                        dh = e.gemm_nt(dz, w_ts[l], empty, empty, False)

            print(f"stage H={H} M={M} layers={N}")
            arms = {"fwd per layer in=784": lambda: fwd_layers(IN0),
                    "fwd per layer in=H": lambda: fwd_layers(H),
                    "bwd per layer 3 dgrads": lambda: bwd_layers(3),
                    "bwd per layer 2 dgrads": lambda: bwd_layers(2)}
            for arm in F.CHAIN_WIDE_ARMS[H]:
                tag = " rows=%d waves=%d" % arm
                arms["fwd stage in=784" + tag] = (
                    lambda a=arm: F.fwd_chain_wide_stage(xs[IN0], ws[IN0], bs,
                                                         *a))
                for start, name in ((1, "streamed"), (2, "tile")):
                    arms[f"fwd stage in=H {name}" + tag] = (
                        lambda a=arm, s=start: F.fwd_chain_wide_stage(
                            xs[H], ws[H], bs, *a, s))
                for nw in (3, 2):
                    arms[f"bwd stage {nw} dgrads" + tag] = (
                        lambda a=arm, n=nw: F.bwd_chain_wide_stage(
                            dout, hs_top, w_ts[:n], *a))
            bench(arms)
            print(f"stage dropout p={p} H={H} M={M} layers={N}")
            bench({
                "fwd per layer drop in=784": lambda: fwd_layers(IN0, True),
                "fwd per layer drop in=H": lambda: fwd_layers(H, True),
                "fwd stage drop in=784": lambda: F.fwd_chain_wide_stage_dropout(
                    xs[IN0], ws[IN0], bs, *key),
                "fwd stage drop in=H streamed": lambda:
                    F.fwd_chain_wide_stage_dropout(xs[H], ws[H], bs, *key,
                                                   0, 0, 1),
                "fwd stage drop in=H tile": lambda:
                    F.fwd_chain_wide_stage_dropout(xs[H], ws[H], bs, *key,
                                                   0, 0, 2),
                "bwd per layer scaled 3 dgrads": lambda: bwd_layers(3, scale),
                "bwd stage dz_scale 3 dgrads": lambda: F.bwd_chain_wide_stage(
                    dout, hd_top, w_ts, dz_scale=scale),
            })
            models = {"stage 0": MLP([IN0] + [H] * 4 + [C], 0, 2, M),
                      "middle": MLP([H] * 8 + [C], 1, 3, M)}
            steps = {}
            for name, model in models.items():
                model.materialize_device(dev)

                def step(on, model=model, k=model.layers[0].in_dims):
                    F.set_chain_wide(on)
                    model.zero_grad()
                    model.forward(xs[k], 0)
                    model.backward(dout, 0)

                steps[f"step {name}, SS_CHAIN_WIDE=0"] = lambda s=step: s(False)
                steps[f"step {name}, SS_CHAIN_WIDE=1"] = lambda s=step: s(True)
            bench(steps)


if sys.argv[1:] == ["dropout"]:
    dropout_section()
    sys.exit(0)
if sys.argv[1:2] == ["stage"]:
    stage_section(tuple(int(a) for a in sys.argv[2:4]) or None)
    sys.exit(0)

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
