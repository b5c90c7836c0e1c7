"""Benchmark harness (driver contract).

`python bench.py --gpus N --steps K --warmup W` runs the flagship
training step — 4-layer MLP, MNIST shape (784→256→256→256→10), bf16,
synthetic data, fused softmax-cross-entropy head — on N GPUs of one
node as DP over RCCL/xGMI (weak scaling: fixed per-GPU batch).

For N>1 the driver launches this via torch.distributed.run with one
rank per GPU; RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* come from the env.

Rank 0 prints ONE JSON line with the whole-job samples/sec.  (Under
the production nccl/RCCL backend stdout carries only that line; the
gloo TEST backend prints its own "[Gloo] Rank..." connectivity banners
to stdout — pipe through `grep '^{'` when parsing gloo runs.)

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the line.  `--dump-outputs DIR` additionally
writes what the last timed step left behind (the updated f32 master
parameters and the f32 gradients that produced them) as DIR/<name>.npy.
The step runs whatever path the arguments select (split-K atomic wgrad
unless `--deterministic` is given).  Data and initial weights are
seeded, and a dump run starts its last timed step from the initial
weights again, so that step's inputs are identical from run to run and
two builds can be compared output for output: what remains between runs
is the f32 summation order of one step's atomics (none at all under
`--deterministic`).  `--full` is where any measurement beyond the
headline figure belongs (there is none today).
"""

import argparse
import json
import os
import time

import torch

# --dump-outputs cap: 64 MB of float32 in all
_DUMP_BUDGET_ELEMS = (64 << 20) // 4


def sample_slice(size, keep, seed):
    """A fixed sample of `keep` of `size` flat indices: every stride-th
    element from a seeded offset.  A slice, so taking it costs neither
    an index array nor a pass over the elements left out."""
    import numpy as np

    stride = max(1, size // keep)
    first = int(np.random.default_rng(seed).integers(stride))
    return slice(first, first + stride * keep, stride)


def dump_outputs(out_dir, model, rank=0, world=1,
                 budget_elems=_DUMP_BUDGET_ELEMS):
    """Write the state the timed path hands back — per parameter, the
    f32 master after the last step and the f32 gradient of that step —
    as float32 .npy files.  Arrays are written whole while they fit the
    64 MB budget; beyond it each array contributes a fixed, seeded
    sample of its elements proportional to its size."""
    import numpy as np

    arrays = []
    for i, p in enumerate(model.parameters()):
        arrays.append((f"param_{i:02d}", p.data))
        if p.grad is not None:
            arrays.append((f"grad_{i:02d}", p.grad))
    total = sum(t.numel() for _, t in arrays)
    os.makedirs(out_dir, exist_ok=True)
    prefix = f"rank{rank}_" if world > 1 else ""
    for k, (name, t) in enumerate(arrays):
        t = t.detach()
        if total > budget_elems:
            keep = max(1, t.numel() * budget_elems // total)
            t = t.reshape(-1)[sample_slice(t.numel(), keep, 1000 + k)]
        a = t.to(torch.float32).cpu().contiguous().numpy()
        np.save(os.path.join(out_dir, prefix + name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-batch", type=int, default=16384)
    ap.add_argument("--mubatches", type=int, default=1)
    ap.add_argument("--pp", type=int, default=1)
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor parallelism (composes with --dp; "
                         "pp must be 1)")
    ap.add_argument("--schedule", default="naive",
                    choices=["naive", "gpipe", "pipedream"])
    ap.add_argument("--layer-sizes", default="784,256,256,256,10")
    ap.add_argument("--loss", default="xent", choices=["xent", "mse"])
    ap.add_argument("--backend", default=None,
                    help="torch.distributed backend override "
                         "(default: nccl on GPU, gloo on CPU)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--graph", action="store_true",
                    help="capture steps in a hipGraph and replay "
                         "(single-GPU; replay floor ~10µs makes eager "
                         "faster at the flagship step size — measured)")
    ap.add_argument("--no-graph", action="store_true",
                    help="(compat) force eager; eager is the default")
    ap.add_argument("--deterministic", action="store_true",
                    help="bitwise-reproducible mode (split_k=1 wgrad)")
    ap.add_argument("--fp8-fwd", action="store_true",
                    help="MX-fp8 training forward on qualifying layers")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the last step's "
                         "parameters and gradients as DIR/<name>.npy "
                         "(float32, at most 64 MB in all); that step "
                         "starts from the seeded initial weights so its "
                         "inputs are the same in every run")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline "
                         "figure (none exist today; a plain run is "
                         "already the whole benchmark)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import SCHEDULES, Worker, init_topology

    if args.deterministic:
        from shallowspeed_amd.ops import functional as _F

        _F.set_deterministic(True)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus or args.gpus == 1 or world == 1, \
        f"--gpus {args.gpus} vs WORLD_SIZE {world}"
    n = max(world, 1)
    pp = args.pp
    tp = args.tp
    if tp > 1:
        assert pp == 1, "tp composes with dp only"
        dp = n // tp
        assert dp * tp == n, f"dp({dp})*tp({tp}) != {n}"
    else:
        dp = n // pp
        assert dp * pp == n, f"dp({dp})*pp({pp}) != {n}"

    device = torch.device(args.device) if args.device else None
    topo = init_topology(dp, pp, backend=args.backend, device=device,
                         tp=tp)
    device = topo.device
    is_gpu = device.type == "cuda"

    sizes = [int(s) for s in args.layer_sizes.split(",")]
    assert args.local_batch % args.mubatches == 0
    # PP needs len(sizes) % pp == 0 (stage slicing, layers.py:242):
    # pad the default config with extra hidden layers if needed
    while len(sizes) % pp != 0:
        sizes.insert(1, sizes[1])
    assert len(sizes) % pp == 0
    global_batch = args.local_batch * dp
    mubatch = args.local_batch // args.mubatches

    if tp > 1:
        from shallowspeed_amd.parallel import TPMLP

        model = TPMLP(sizes, topo.tp_group, topo.tp_rank, tp, global_batch,
                      loss=args.loss)
    else:
        model = MLP(sizes, topo.stage_id, pp, global_batch, loss=args.loss)
    model.materialize_device(device)
    if args.fp8_fwd:
        model.set_fp8_fwd(True)
    opt = SGD(model.parameters(), lr=0.001)
    # synthetic data of the benchmark shape, random-init weights (no
    # network for datasets/checkpoints in this environment)
    n_samples = max(args.local_batch * dp * 2, 2 * global_batch)
    ds = Dataset(global_batch, mubatch, n_samples=n_samples,
                 in_dim=sizes[0], n_classes=sizes[-1], device=device)
    ds.load(topo.dp_rank, dp)
    worker = Worker(topo, model, ds, opt)
    sched_cls = SCHEDULES[args.schedule]
    sched = sched_cls(ds.num_mubatches(), pp, topo.stage_id)
    nb = ds.num_batches()

    use_graph = args.graph and not args.no_graph and is_gpu \
        and topo.world == 1

    def one_step(i):
        if use_graph:
            worker.execute_graphed(sched, i % nb)
        else:
            worker.execute(sched, i % nb)

    import torch.distributed as dist

    def barrier_sync():
        if is_gpu:
            torch.cuda.synchronize(device)
        if topo.is_distributed:
            if is_gpu and dist.get_backend() == "nccl":
                dist.barrier(device_ids=[device.index])
            else:
                dist.barrier()
        if is_gpu:
            torch.cuda.synchronize(device)

    # --dump-outputs: the dumped step must be a function of the
    # arguments.  Data and initial weights are seeded, but the default
    # wgrad kernels combine split-K partial sums with f32 atomics, so
    # every step's gradients carry arrival-order noise in their low
    # bits, and bf16 training amplifies it step after step until two
    # runs no longer agree to rounding.  So a dump run puts the seeded
    # initial weights back just before its LAST timed step (clock
    # stopped meanwhile): that step runs the very path the arguments
    # select, on inputs that are identical from run to run, and what it
    # leaves differs between runs only by one step's f32 summation order.
    init_weights = None
    if args.dump_outputs:
        init_weights = [p.data.clone() for p in model.parameters()]

    def restore_init_weights():
        for p, w0 in zip(model.parameters(), init_weights):
            p.data.copy_(w0)
            p.sync_lp()
        if hasattr(model, "invalidate_fp8"):
            model.invalidate_fp8()

    for i in range(args.warmup):
        one_step(i)
    barrier_sync()
    paused = 0.0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if init_weights is not None and i == args.steps - 1:
            barrier_sync()
            t_pause = time.perf_counter()
            restore_init_weights()
            barrier_sync()
            paused = time.perf_counter() - t_pause
        one_step(i)
    barrier_sync()
    elapsed = time.perf_counter() - t0 - paused

    # MAX elapsed over ranks
    if topo.is_distributed:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if is_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    samples = global_batch * args.steps
    value = samples / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, model, topo.rank, topo.world)

    if topo.rank == 0:
        print(json.dumps({
            "metric": "samples/sec (whole node), 4-layer MLP MNIST-shape, "
                      "DP×PP at 1/2/4/8 GPUs",
            "value": value,
            "unit": "samples/sec",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if is_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": ("mlp4_mnist_784x256x256x256x10"
                          if sizes == [784, 256, 256, 256, 10] else
                          "mlp%d_%s" % (len(sizes) - 1,
                                        "x".join(map(str, sizes[:3]))
                                        + ("..." if len(sizes) > 4 else ""))),
                "global_batch": global_batch,
                "seq_len": None,
                "parallelism": f"dp{dp}"
                + (f"xpp{pp}" if pp > 1 else "")
                + (f"xtp{tp}" if tp > 1 else ""),
                "schedule": args.schedule,
                "loss": args.loss,
                "mubatches": args.mubatches,
                "hipgraph": use_graph,
                "fp8_fwd": args.fp8_fwd,
                "deterministic": args.deterministic,
                "peak_mem_gb": (round(torch.cuda.max_memory_allocated()
                                      / 2**30, 2) if is_gpu else None),
            },
        }), flush=True)

    if topo.is_distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
