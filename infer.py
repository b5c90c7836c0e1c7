"""Batched inference driver (serving path).

Loads a stage-sharded checkpoint (or fresh shape-seeded weights) and
runs the forward-only pipeline over a dataset, reporting predictions
and throughput.  Uses the same Worker + InferenceSchedule machinery as
training eval (reference: compute_accuracy, train.py:21-47, fwd-only
schedule pipe.py:275-294) — so it works single-GPU or as a PP pipeline
under torchrun.

    python infer.py --batch 16384 --samples 65536          # 1 GPU
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 4 \
        infer.py --pp 4 --checkpoint ckpt/                 # pipeline
"""

import argparse
import json
import time

import torch

from shallowspeed_amd.data import Dataset
from shallowspeed_amd.models import MLP
from shallowspeed_amd.parallel import InferenceSchedule, Worker, init_topology


def build_fp8_plan(model, batch):
    """Pre-quantize qualifying Linear weights to MX-fp8 (e4m3 + E8M0
    block scales, ops.functional.fp8_quantize); layers whose shapes
    fall outside the fp8 tier (O%256, I%256, batch%256) stay bf16.
    Weight quantization happens ONCE — the serving analogue of
    weight-only deployment quantization (beyond the reference's
    scope)."""
    from shallowspeed_amd.models import Linear
    from shallowspeed_amd.ops.functional import fp8_quantize

    plan = []
    for layer in model.layers:
        if not isinstance(layer, Linear):
            continue  # loss head: inference takes argmax of logits
        w = layer.weight.compute().to(torch.bfloat16)
        bias = layer.bias.compute().to(torch.bfloat16)
        O, I = w.shape
        ok = (O % 256 == 0 and I % 256 == 0 and batch % 256 == 0
              and I >= 256 and w.is_cuda)
        if ok:
            wq, wsc = fp8_quantize(w)
            plan.append(("fp8", wq, wsc, bias,
                         layer.activation == "relu"))
        else:
            plan.append(("bf16", w, None, bias,
                         layer.activation == "relu"))
    return plan


def build_fused_plan(model, batch):
    """Qualify the model for the persistent fused-MLP forward kernel
    (csrc/fused_mlp.hip): 256-wide ReLU hidden chain (1..8 layers),
    head ≤16 classes, batch % 64 == 0.  Activations stay LDS-resident
    across the whole chain; the head emits per-row argmax directly."""
    import torch

    from shallowspeed_amd.models import Linear

    ls = [l for l in model.layers if isinstance(l, Linear)]
    if len(ls) < 2:
        return None
    hidden, head = ls[:-1], ls[-1]
    ok = (batch % 64 == 0 and 1 <= len(hidden) <= 8
          and all(l.out_dims == 256 and l.activation == "relu"
                  for l in hidden)
          and head.in_dims == 256 and head.out_dims <= 16
          and head.activation is None
          and model.device.type == "cuda")
    if not ok:
        return None
    ptrs = []
    for l in ls:
        ptrs += [l.weight.compute().data_ptr(),
                 l.bias.compute().data_ptr()]
    desc = torch.tensor(ptrs, dtype=torch.int64).to(model.device)
    return (desc, ls[0].in_dims, len(hidden), head.out_dims)


def fused_forward_fn(model, batch, scores=False):
    """How --fused runs a batch of `batch` rows of this model: a callable
    x -> argmax (x -> (argmax, f32 logits) with scores=True), or None
    when no fused kernel serves the model.

    The 256-wide flagship at batch % 64 == 0 keeps csrc/fused_mlp.hip
    (build_fused_plan); every other ReLU chain of one hidden width in
    {128, 256, 512, 1024} with a head of up to 16 classes, at any batch,
    and any request for scores, goes to csrc/fused_mlp_wide.hip through
    F.fused_mlp_forward.  A ReLU chain whose hidden widths differ, each
    one of those four (784,512,256,128,10), goes the same way to
    csrc/fused_mlp_taper.hip."""
    from shallowspeed_amd.models import Linear
    from shallowspeed_amd.ops import functional as F
    from shallowspeed_amd.ops import load_ext

    if model.device.type != "cuda":
        return None
    plan = None if scores else build_fused_plan(model, batch)
    if plan is not None:
        ext = load_ext(required=True)
        desc, ind, nh, co = plan
        return lambda x: ext.fused_mlp_argmax(x, desc, ind, nh, co)
    ls = [l for l in model.layers if isinstance(l, Linear)]
    if len(ls) < 2 or ls[-1].activation is not None or any(
            l.activation != "relu" for l in ls[:-1]):
        return None
    ws = [l.weight.compute() for l in ls]
    bs = [l.bias.compute() for l in ls]
    probe = torch.zeros(1, ls[0].in_dims, dtype=torch.bfloat16,
                        device=model.device)
    if not F.fused_mlp_ok(probe, ws, bs):
        return None
    return lambda x: F.fused_mlp_forward(x, ws, bs, logits=scores)


def fp8_forward(plan, x):
    """fp8-RESIDENT chain: a layer whose successor is also fp8 emits
    its output pre-quantized from the GEMM epilogue (gemm_nt_f8_q) —
    activations never round-trip through bf16 between fp8 layers."""
    from shallowspeed_amd.ops import load_ext
    from shallowspeed_amd.ops.functional import (fp8_quantize, linear_fwd,
                                                 linear_fwd_fp8)

    e = load_ext(required=True)
    h = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
    hq = hs = None  # fp8-resident activation, when set
    for li, (kind, w, wsc, bias, relu) in enumerate(plan):
        nxt_fp8 = li + 1 < len(plan) and plan[li + 1][0] == "fp8"
        if kind == "fp8":
            if hq is None:
                hq, hs = fp8_quantize(h)
            if nxt_fp8:
                hq, hs = e.gemm_nt_f8_q(hq, hs, w, wsc, bias, relu)
            else:
                h = linear_fwd_fp8(hq, hs, w, wsc, bias, relu)
                hq = hs = None
        else:
            assert hq is None  # nxt_fp8 guarantees bf16 h here
            h = linear_fwd(h, w, bias, relu)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pp", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--layer-sizes", default="784,256,256,256,10")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--data-dir", default=None)
    ap.add_argument("--out", default=None, help="write predictions (.pt)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--backend", default=None)
    ap.add_argument("--fp8", action="store_true",
                    help="MX-fp8 serving path for qualifying wide layers "
                         "(weights pre-quantized; activations per batch)")
    ap.add_argument("--fused", action="store_true",
                    help="persistent fused-MLP forward kernel (whole "
                         "layer chain in ONE launch, LDS-resident "
                         "activations, in-kernel argmax; ReLU chains "
                         "of one hidden width in 128/256/512/1024, "
                         "up to 8 hidden layers and 16 classes, any "
                         "batch)")
    ap.add_argument("--scores", default=None, metavar="PATH",
                    help="with --fused: also save the f32 logits the "
                         "argmax was taken over (.pt)")
    ap.add_argument("--graph", action="store_true",
                    help="capture the forward-only batch in a hipGraph "
                         "and replay it per batch (single GPU; collapses "
                         "the per-kernel launch gaps that dominate the "
                         "forward-only serving loop)")
    args = ap.parse_args()

    sizes = [int(s) for s in args.layer_sizes.split(",")]
    while len(sizes) % args.pp != 0:
        sizes.insert(1, sizes[1])

    device = torch.device(args.device) if args.device else None
    topo = init_topology(1, args.pp, backend=args.backend, device=device)
    device = topo.device

    model = MLP(sizes, topo.stage_id, args.pp, args.batch)
    model.materialize_device(device)
    if args.checkpoint:
        from shallowspeed_amd.checkpoint import load_checkpoint

        load_checkpoint(args.checkpoint, model, topo)
    model.eval()

    ds = Dataset(args.batch, args.batch, save_dir=args.data_dir,
                 n_samples=args.samples, in_dim=sizes[0],
                 n_classes=sizes[-1], device=device).load(0, 1)
    worker = Worker(topo, model, ds, None, use_dp=False)
    sched = InferenceSchedule(1, args.pp, topo.stage_id)

    fp8_plan = None
    if args.fp8:
        assert args.pp == 1, "--fp8 serving path is single-stage"
        fp8_plan = build_fp8_plan(model, args.batch)

    fused_fn = None
    if args.fused and topo.world == 1 and not fp8_plan:
        fused_fn = fused_forward_fn(model, args.batch,
                                    scores=bool(args.scores))
        if fused_fn is None:
            print("# --fused: model/batch outside the fused tier, "
                  "falling back", flush=True)
    if args.scores and fused_fn is None:
        print("# --scores needs the --fused path: not written", flush=True)

    graphed = None
    if args.graph and device.type == "cuda" and topo.world == 1 \
            and not fp8_plan and fused_fn is None:
        # Serving graph: one persistent input slot + captured forward
        # + argmax; per batch = one D2D copy + one graph replay.  The
        # forward-only loop is launch-gap-bound (kernel sum ~59 µs vs
        # ~91 µs wall at the flagship shape), so replay reclaims the
        # gaps in a way the GPU-bound training step cannot.
        from shallowspeed_amd.ops.functional import row_argmax as _ram

        model.eval()
        gx = torch.empty_like(ds.x_compute[:args.batch])
        gx.copy_(ds.x_compute[:args.batch])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            gout = _ram(model.forward(gx))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout = _ram(model.forward(gx))
        graphed = (g, gx, gout)

    preds = []
    # warmup
    if fp8_plan:
        fp8_forward(fp8_plan, ds.x[:args.batch])
    worker.execute(sched, 0)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    from shallowspeed_amd.ops.functional import row_argmax

    scores = []
    for b in range(ds.num_batches()):
        if fused_fn is not None:
            out = fused_fn(ds.x_compute[b * args.batch:(b + 1) * args.batch])
            if args.scores:
                scores.append(out[1])
                out = out[0]
            preds.append(out)
            continue
        if graphed is not None:
            g, gx, gout = graphed
            gx.copy_(ds.x_compute[b * args.batch:(b + 1) * args.batch],
                     non_blocking=True)
            g.replay()
            preds.append(gout.clone())
            continue
        if fp8_plan:
            logits = fp8_forward(fp8_plan,
                                 ds.x[b * args.batch:(b + 1) * args.batch])
            preds.append(row_argmax(logits))
            continue
        worker.execute(sched, b)
        if topo.stage_id == args.pp - 1:
            # HIP row-argmax, on device; one transfer at the end
            # (torch's ROCm argmax on skinny bf16 is ~1.3 ms/batch)
            preds.append(row_argmax(worker._out_bufs[0]))
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    preds = [p.cpu() for p in preds]

    if topo.stage_id == args.pp - 1:
        n = ds.num_batches() * args.batch
        print(json.dumps({
            "inference_samples_per_sec": n / dt,
            "ms_per_batch": dt / ds.num_batches() * 1e3,
            "batch": args.batch,
            "n": n,
        }))
        if args.out:
            torch.save(torch.cat(preds), args.out)
            print(f"predictions -> {args.out}")
        if scores:
            torch.save(torch.cat([s.cpu() for s in scores]), args.scores)
            print(f"scores -> {args.scores}")


if __name__ == "__main__":
    main()
