"""HIP kernel numerics vs plain PyTorch fp32 references (the GPU
analog of the reference's finite-difference checks,
tests/test_functional.py).  All tests need a real MI355X."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def rand_bf16(*shape, device, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return t.to(device=device, dtype=BF)


def tol(ref, atol=1e-2, rtol=2e-2):
    return dict(atol=atol + 1e-3 * ref.abs().max().item(), rtol=rtol)


# ------------------------------------------------------------- MFMA layout

def test_mfma_layout(gpu_device):
    """A=I with ASYMMETRIC B catches transposed C-writes
    (cdna_hip_programming.md §3: always asymmetric-B check)."""
    e = ext()
    M = N = K = 64
    a = torch.eye(M, K, device=gpu_device, dtype=BF)
    b = torch.arange(N * K, device=gpu_device, dtype=torch.float32)
    b = ((b % 37) / 37.0 + (b // K) * 0.01).reshape(N, K).to(BF)
    empty = torch.Tensor()
    c = e.gemm_nt(a, b, empty, empty, False)
    torch.testing.assert_close(c.float(), b.t().float().contiguous(),
                               atol=1e-2, rtol=1e-2)


# ------------------------------------------------------------- gemm_nt

@pytest.mark.parametrize("shape", [
    (32, 10, 784), (64, 64, 64), (128, 128, 784), (100, 127, 123),
    (8192, 128, 784), (33, 17, 9), (256, 10, 123),
])
def test_gemm_nt_vs_torch(gpu_device, shape):
    M, N, K = shape
    e = ext()
    a = rand_bf16(M, K, device=gpu_device, seed=1)
    b = rand_bf16(N, K, device=gpu_device, seed=2)
    empty = torch.Tensor()
    c = e.gemm_nt(a, b, empty, empty, False)
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(c.float(), ref, **tol(ref))


def test_gemm_nt_bias_relu(gpu_device):
    e = ext()
    M, N, K = 128, 96, 200
    a = rand_bf16(M, K, device=gpu_device, seed=3)
    b = rand_bf16(N, K, device=gpu_device, seed=4)
    bias = rand_bf16(N, device=gpu_device, seed=5)
    empty = torch.Tensor()
    c = e.gemm_nt(a, b, bias, empty, True)
    ref = torch.clamp(a.float() @ b.float().t() + bias.float(), min=0)
    torch.testing.assert_close(c.float(), ref, **tol(ref))
    assert (c.float() >= 0).all()


def test_gemm_nt_mask(gpu_device):
    """dgrad with fused ReLU mask: (a ⊙ 1[mask>0]) @ b^T."""
    e = ext()
    M, N, K = 96, 64, 128
    a = rand_bf16(M, K, device=gpu_device, seed=6)
    mask = rand_bf16(M, K, device=gpu_device, seed=7)
    b = rand_bf16(N, K, device=gpu_device, seed=8)
    empty = torch.Tensor()
    c = e.gemm_nt(a, b, empty, mask, False)
    am = a.float() * (mask.float() > 0)
    ref = am @ b.float().t()
    torch.testing.assert_close(c.float(), ref, **tol(ref))


# ------------------------------------------------------------- wgrad

@pytest.mark.parametrize("shape", [
    (256, 64, 64), (8192, 128, 784), (100, 127, 123), (32, 10, 123),
])
def test_wgrad_accumulate_and_bias(gpu_device, shape):
    Kb, Mo, N = shape
    e = ext()
    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=9)
    x = rand_bf16(Kb, N, device=gpu_device, seed=10)
    gw = torch.ones(Mo, N, device=gpu_device, dtype=torch.float32)
    gb = torch.ones(Mo, device=gpu_device, dtype=torch.float32)
    empty = torch.Tensor()
    e.wgrad_tn(dy, x, gw, gb, empty, 0)
    ref_w = 1.0 + dy.float().t() @ x.float()
    ref_b = 1.0 + dy.float().sum(0)
    torch.testing.assert_close(gw, ref_w, **tol(ref_w))
    torch.testing.assert_close(gb, ref_b, **tol(ref_b))


def test_wgrad_mask_and_splitk_determinism_modes(gpu_device):
    e = ext()
    Kb, Mo, N = 4096, 64, 96
    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=11)
    mask = rand_bf16(Kb, Mo, device=gpu_device, seed=12)
    x = rand_bf16(Kb, N, device=gpu_device, seed=13)
    dym = dy.float() * (mask.float() > 0)
    ref_w = dym.t() @ x.float()
    ref_b = dym.sum(0)
    for split_k in (0, 1, 4):
        gw = torch.zeros(Mo, N, device=gpu_device, dtype=torch.float32)
        gb = torch.zeros(Mo, device=gpu_device, dtype=torch.float32)
        e.wgrad_tn(dy, x, gw, gb, mask, split_k)
        torch.testing.assert_close(gw, ref_w, **tol(ref_w))
        torch.testing.assert_close(gb, ref_b, **tol(ref_b))


# ------------------------------------------------------------- elementwise

def test_relu_fwd_bwd(gpu_device):
    e = ext()
    x = rand_bf16(1000, 37, device=gpu_device, seed=14)
    y = e.relu_fwd(x)
    torch.testing.assert_close(y.float(), torch.clamp(x.float(), min=0))
    dy = rand_bf16(1000, 37, device=gpu_device, seed=15)
    dx = e.relu_bwd(dy, y)
    torch.testing.assert_close(dx.float(), dy.float() * (y.float() > 0))


@pytest.mark.parametrize("C", [10, 64, 100, 1000])
def test_softmax_fwd_bwd(gpu_device, C):
    e = ext()
    x = rand_bf16(257, C, device=gpu_device, scale=3.0, seed=16)
    s = e.softmax_fwd(x)
    ref = torch.softmax(x.float(), dim=-1)
    torch.testing.assert_close(s.float(), ref, atol=8e-3, rtol=2e-2)
    dy = rand_bf16(257, C, device=gpu_device, seed=17)
    dx = e.softmax_bwd(dy, s)
    sf = s.float()
    dot = (sf * dy.float()).sum(-1, keepdim=True)
    torch.testing.assert_close(dx.float(), sf * (dy.float() - dot),
                               atol=8e-3, rtol=2e-2)


def test_head_bwd_kernels(gpu_device):
    e = ext()
    B, C, GB = 128, 10, 512
    z = rand_bf16(B, C, device=gpu_device, scale=2.0, seed=18)
    s = e.softmax_fwd(z)
    t = torch.zeros(B, C)
    t[torch.arange(B), torch.randint(0, C, (B,))] = 1
    t = t.to(device=gpu_device, dtype=BF)
    # mse head
    sf = s.float()
    g = -2.0 * (t.float() - sf) / GB
    ref = sf * (g - (sf * g).sum(-1, keepdim=True))
    dz = e.head_mse_bwd(s, t, GB)
    torch.testing.assert_close(dz.float(), ref, atol=1e-4, rtol=2e-2)
    # xent head
    dz2 = e.head_xent_bwd(s, t, GB)
    torch.testing.assert_close(dz2.float(), (sf - t.float()) / GB,
                               atol=1e-4, rtol=2e-2)


# ------------------------------------------------------------- SGD

def test_sgd_multi(gpu_device):
    from shallowspeed_amd.models import Linear, Sequential, SGD

    model = Sequential([
        Linear(123, 65, activation="relu"),
        Linear(65, 10),
    ]).materialize_device(gpu_device)
    opt = SGD(model.parameters(), lr=0.1)
    for p in model.parameters():
        p.grad.normal_(generator=None)
    before = [p.data.clone() for p in model.parameters()]
    grads = [p.grad.clone() for p in model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    for b, g, p in zip(before, grads, model.parameters()):
        torch.testing.assert_close(p.data, b - 0.1 * g)
        # bf16 copies refreshed in-kernel
        torch.testing.assert_close(p.lp.float(), p.data.to(BF).float())
        if p.lp_t is not None:
            torch.testing.assert_close(p.lp_t.float(),
                                       p.data.to(BF).t().float().contiguous())


# ----------------------------------------------------- end-to-end on GPU

def test_gpu_training_learns(gpu_device):
    """Whole engine on HIP kernels: loss head + GEMMs + SGD learn the
    synthetic teacher task (reference gate: accuracy climbs)."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import (
        GPipeSchedule, NaiveParallelSchedule, PipeDreamFlushSchedule,
        Topology, Worker)

    model = MLP([784, 256, 128, 10], 0, 1, 512, loss="xent")
    model.materialize_device(gpu_device)
    opt = SGD(model.parameters(), lr=0.05)
    ds = Dataset(512, 128, n_samples=2048, in_dim=784, n_classes=10,
                 device=gpu_device).load(0, 1)
    w = Worker(Topology(device=gpu_device), model, ds, opt)

    def acc():
        model.eval()
        p = model.forward(ds.x.to(BF), 0)
        model.train()
        return (p.float().argmax(-1).cpu() ==
                ds.y.float().argmax(-1).cpu()).float().mean().item()

    a0 = acc()
    for sched in (NaiveParallelSchedule, GPipeSchedule,
                  PipeDreamFlushSchedule):
        for b in range(ds.num_batches()):
            w.execute(sched(ds.num_mubatches(), 1, 0), b)
    for _ in range(10):
        for b in range(ds.num_batches()):
            w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), b)
    a1 = acc()
    assert a1 > a0 + 0.15, (a0, a1)


def test_gpu_matches_cpu_reference_one_step(gpu_device):
    """One full training step GPU(bf16 HIP kernels) vs CPU(f32 torch):
    weights agree to bf16 tolerance."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import NaiveParallelSchedule, Topology, Worker

    def run(device):
        model = MLP([48, 32, 16, 10], 0, 1, 64, loss="xent")
        model.materialize_device(device)
        opt = SGD(model.parameters(), lr=0.05)
        ds = Dataset(64, 16, n_samples=64, in_dim=48, n_classes=10,
                     device=device).load(0, 1)
        w = Worker(Topology(device=torch.device(device)), model, ds, opt)
        w.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), 0)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        return [p.data.float().cpu() for p in model.parameters()]

    got = run(gpu_device)
    want = run("cpu")
    for g, w_ in zip(got, want):
        torch.testing.assert_close(g, w_, atol=3e-2, rtol=3e-2)


def test_gpu_graph_matches_eager(gpu_device):
    """hipGraph-captured steps train the same as eager steps."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    def run(graphed):
        model = MLP([96, 64, 32, 10], 0, 1, 256, loss="xent")
        model.materialize_device(gpu_device)
        opt = SGD(model.parameters(), lr=0.05)
        ds = Dataset(256, 64, n_samples=512, in_dim=96, n_classes=10,
                     device=gpu_device).load(0, 1)
        w = Worker(Topology(device=gpu_device), model, ds, opt)
        sched = GPipeSchedule(ds.num_mubatches(), 1, 0)
        for step in range(6):
            b = step % ds.num_batches()
            if graphed:
                w.execute_graphed(sched, b)
            else:
                w.execute(sched, b)
        torch.cuda.synchronize()
        return [p.data.float().cpu() for p in model.parameters()]

    eager = run(False)
    graphed = run(True)
    # split-K wgrad uses f32 atomicAdd, so summation ORDER differs run
    # to run — eager-vs-eager shows the same ~1e-3 jitter after 6 SGD
    # steps; the graph must agree within that envelope.
    for a, b in zip(eager, graphed):
        torch.testing.assert_close(a, b, atol=1e-2, rtol=5e-2)


def test_gpu_checkpoint_roundtrip(tmp_path, gpu_device):
    from shallowspeed_amd.checkpoint import load_checkpoint, save_checkpoint
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.parallel import Topology

    model = MLP([48, 32, 10], 0, 1, 16).materialize_device(gpu_device)
    for p in model.parameters():
        p.data.add_(torch.randn_like(p.data) * 0.1)
        p.sync_lp()
    save_checkpoint(tmp_path, model, Topology(device=gpu_device), step=1)
    fresh = MLP([48, 32, 10], 0, 1, 16).materialize_device(gpu_device)
    load_checkpoint(tmp_path, fresh, Topology(device=gpu_device))
    for a, b in zip(model.parameters(), fresh.parameters()):
        torch.testing.assert_close(a.data, b.data)
        torch.testing.assert_close(a.lp.float(), b.lp.float())
        if a.lp_t is not None:
            torch.testing.assert_close(a.lp_t.float(), b.lp_t.float())


# --------------------------------------------------- layernorm / gelu

@pytest.mark.parametrize("C", [32, 256, 777])
def test_gpu_layernorm_vs_torch(gpu_device, C):
    e = ext()
    B = 513
    x = rand_bf16(B, C, device=gpu_device, seed=21)
    gamma = rand_bf16(C, device=gpu_device, seed=22)
    beta = rand_bf16(C, device=gpu_device, seed=23)
    y, mean, rstd = e.ln_fwd(x, gamma, beta, 1e-5)
    ref = torch.nn.functional.layer_norm(
        x.float(), (C,), gamma.float(), beta.float(), 1e-5)
    torch.testing.assert_close(y.float(), ref, atol=3e-2, rtol=3e-2)

    dy = rand_bf16(B, C, device=gpu_device, seed=24)
    dx = e.ln_bwd_dx(dy, x, gamma, mean, rstd)
    dgamma = torch.zeros(C, device=gpu_device, dtype=torch.float32)
    dbeta = torch.zeros(C, device=gpu_device, dtype=torch.float32)
    e.ln_bwd_dparam(dy, x, mean, rstd, dgamma, dbeta)

    xr = x.float().requires_grad_(True)
    gr = gamma.float().requires_grad_(True)
    br = beta.float().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    yr.backward(dy.float())
    torch.testing.assert_close(dx.float(), xr.grad, atol=3e-2, rtol=5e-2)
    torch.testing.assert_close(dgamma, gr.grad, atol=0.3, rtol=3e-2)
    torch.testing.assert_close(dbeta, br.grad, atol=0.3, rtol=3e-2)


def test_gpu_gelu_vs_torch(gpu_device):
    e = ext()
    z = rand_bf16(1000, 53, device=gpu_device, scale=2.0, seed=25)
    y = e.gelu_fwd(z)
    ref = torch.nn.functional.gelu(z.float(), approximate="tanh")
    torch.testing.assert_close(y.float(), ref, atol=1e-2, rtol=2e-2)
    dy = rand_bf16(1000, 53, device=gpu_device, seed=26)
    zf = z.float().requires_grad_(True)
    torch.nn.functional.gelu(zf, approximate="tanh").backward(dy.float())
    dz = e.gelu_bwd(dy, z)
    torch.testing.assert_close(dz.float(), zf.grad, atol=1e-2, rtol=2e-2)


def test_gpu_ln_gelu_stack_trains(gpu_device):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import (LayerNorm, Linear, SGD, Sequential,
                                         SoftmaxXent)
    from shallowspeed_amd.parallel import NaiveParallelSchedule, Topology, Worker

    gbs = 256
    model = Sequential([
        Linear(64, 128, activation="gelu"),
        LayerNorm(128),
        Linear(128, 10),
        SoftmaxXent(gbs),
    ])
    model.in_dim, model.out_dim = 64, 10
    model.materialize_device(gpu_device)
    opt = SGD(model.parameters(), lr=0.1)
    ds = Dataset(gbs, 64, n_samples=1024, in_dim=64, n_classes=10,
                 device=gpu_device).load(0, 1)
    w = Worker(Topology(device=gpu_device), model, ds, opt)

    def acc():
        model.eval()
        p = model.forward(ds.x.to(BF), 0)
        model.train()
        return (p.float().argmax(-1) == ds.y.float().argmax(-1)).float() \
            .mean().item()

    a0 = acc()
    for _ in range(20):
        for b in range(ds.num_batches()):
            w.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), b)
    torch.cuda.synchronize()
    assert acc() > a0 + 0.15


def test_gpu_reference_default_config_trains(gpu_device):
    """End-to-end with the reference's exact (odd-sized) layer config
    [784,128,127,126,125,124,123,10] (reference train.py:98) — edge
    cases: non-multiple-of-64 dims through every kernel."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    sizes = [784, 128, 127, 126, 125, 124, 123, 10]
    model = MLP(sizes, 0, 1, 128, loss="mse")  # reference loss head
    model.materialize_device(gpu_device)
    opt = SGD(model.parameters(), lr=0.05)
    ds = Dataset(128, 32, n_samples=512, in_dim=784, n_classes=10,
                 device=gpu_device).load(0, 1)
    w = Worker(Topology(device=gpu_device), model, ds, opt)
    h0 = [p.data.float().abs().sum().item() for p in model.parameters()]
    for _ in range(3):
        for b in range(ds.num_batches()):
            w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), b)
    torch.cuda.synchronize()
    for p in model.parameters():
        v = p.data.float()
        assert torch.isfinite(v).all()
    # weights moved
    h1 = [p.data.float().abs().sum().item() for p in model.parameters()]
    assert any(abs(a - b) > 1e-6 for a, b in zip(h0, h1))


def test_gpu_sgd_momentum_weight_decay(gpu_device):
    from shallowspeed_amd.models import Linear, SGD, Sequential

    model = Sequential([Linear(65, 33), Linear(33, 10)])
    model.materialize_device(gpu_device)
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=0.01)
    tw = [p.data.clone().requires_grad_(True) for p in model.parameters()]
    topt = torch.optim.SGD(tw, lr=0.1, momentum=0.9, weight_decay=0.01)
    for step in range(3):
        for p, t in zip(model.parameters(), tw):
            g = torch.randn_like(p.data)
            p.grad.copy_(g)
            t.grad = g.clone()
        opt.step()
        topt.step()
    torch.cuda.synchronize()
    for p, t in zip(model.parameters(), tw):
        torch.testing.assert_close(p.data, t.detach(), atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(p.lp.float(), p.data.to(BF).float())


def test_gpu_deferred_wgrad_matches_eager(gpu_device):
    """Pipeline schedules defer per-µbatch wgrads into chunked
    kernels; grads must match the eager per-µbatch path."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    def run(defer):
        model = MLP([96, 64, 48, 10], 0, 1, 512, loss="xent")
        model.materialize_device(gpu_device)
        if not defer:
            model.set_defer_wgrad = lambda *a, **k: None  # force eager
        opt = SGD(model.parameters(), lr=0.0)  # keep weights fixed
        ds = Dataset(512, 128, n_samples=512, in_dim=96, n_classes=10,
                     device=gpu_device).load(0, 1)
        w = Worker(Topology(device=gpu_device), model, ds, opt)
        w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), 0)
        torch.cuda.synchronize()
        if defer:
            assert w._defer_active, "deferred mode should engage"
        return [p.grad.clone().cpu() for p in model.parameters()]

    got = run(True)
    want = run(False)
    for g, r in zip(got, want):
        torch.testing.assert_close(g, r, atol=2e-3, rtol=2e-2)


def test_gpu_row_argmax(gpu_device):
    from shallowspeed_amd.ops.functional import row_argmax

    x = rand_bf16(4097, 10, device=gpu_device, scale=3.0, seed=30)
    got = row_argmax(x)
    want = x.float().argmax(-1)
    torch.testing.assert_close(got.cpu(), want.cpu())
    x2 = rand_bf16(33, 1000, device=gpu_device, seed=31)
    torch.testing.assert_close(row_argmax(x2).cpu(),
                               x2.float().argmax(-1).cpu())


@pytest.mark.parametrize("shape", [
    (4096, 2048, 2048), (8192, 128, 256), (256, 128, 8192),
])
def test_gemm_nt_glds_tier(gpu_device, shape):
    """Aligned unmasked shapes dispatch to the global_load_lds-staged
    kernel; numerics vs f32 torch (+ bias/relu epilogues)."""
    M, N, K = shape
    e = ext()
    a = rand_bf16(M, K, device=gpu_device, seed=40)
    b = rand_bf16(N, K, device=gpu_device, seed=41)
    bias = rand_bf16(N, device=gpu_device, seed=42)
    empty = torch.Tensor()
    c = e.gemm_nt(a, b, empty, empty, False)
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(c.float(), ref, **tol(ref, atol=0.05))
    c2 = e.gemm_nt(a, b, bias, empty, True)
    ref2 = torch.clamp(ref + bias.float(), min=0)
    torch.testing.assert_close(c2.float(), ref2, **tol(ref2, atol=0.05))


def test_gemm_shape_fuzz(gpu_device):
    """Odd-shape sweep through every GEMM dispatch tier (deterministic
    pseudo-random shapes; catches bounds/edge regressions)."""
    import random as _r

    e = ext()
    rng = _r.Random(12345)
    empty = torch.Tensor()
    for trial in range(24):
        M = rng.randint(1, 400)
        N = rng.randint(1, 300)
        K = rng.randint(1, 300)
        a = rand_bf16(M, K, device=gpu_device, seed=trial)
        b = rand_bf16(N, K, device=gpu_device, seed=trial + 1000)
        c = e.gemm_nt(a, b, empty, empty, False)
        ref = a.float() @ b.float().t()
        torch.testing.assert_close(c.float(), ref, **tol(ref)), (M, N, K)
        # wgrad same shapes (Kb=M)
        gw = torch.zeros(N, K, device=gpu_device, dtype=torch.float32)
        gb = torch.zeros(N, device=gpu_device, dtype=torch.float32)
        dy = rand_bf16(M, N, device=gpu_device, seed=trial + 2000)
        x = rand_bf16(M, K, device=gpu_device, seed=trial + 3000)
        e.wgrad_tn(dy, x, gw, gb, empty, 0)
        rw = dy.float().t() @ x.float()
        torch.testing.assert_close(gw, rw, **tol(rw)), (M, N, K)
        torch.testing.assert_close(gb, dy.float().sum(0), **tol(rw))


@pytest.mark.parametrize("shape,bias_on,relu", [
    ((256, 512, 128), False, False),
    ((512, 512, 384), True, True),
    ((1024, 768, 512), True, False),
    ((768, 1024, 2048), False, True),
])
def test_gemm_nt_256_tier(gpu_device, shape, bias_on, relu):
    """Direct numerics of the 256-tile 8-phase kernel (gemm256.hip)
    vs f32 torch, including the bias/ReLU epilogues."""
    M, N, K = shape
    e = ext()
    a = rand_bf16(M, K, device=gpu_device, seed=50)
    b = rand_bf16(N, K, device=gpu_device, seed=51)
    bias = (rand_bf16(N, device=gpu_device, seed=52) if bias_on
            else torch.Tensor())
    c = e.gemm_nt_256(a, b, bias, relu)
    ref = a.float() @ b.float().t()
    if bias_on:
        ref = ref + bias.float()
    if relu:
        ref = torch.clamp(ref, min=0)
    torch.testing.assert_close(c.float(), ref, **tol(ref, atol=0.05))


def test_gemm_nt_256_dispatch_consistency(gpu_device):
    """A qualifying wide shape through the production gemm_nt dispatch
    (which routes to the 256 tier) must match f32 torch AND be
    bit-stable across runs (race screen of the integrated path)."""
    e = ext()
    M, N, K = 4096, 2048, 1024  # 16x8 = 128 blocks >= gate
    a = rand_bf16(M, K, device=gpu_device, seed=60)
    b = rand_bf16(N, K, device=gpu_device, seed=61)
    empty = torch.Tensor()
    first = e.gemm_nt(a, b, empty, empty, False)
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(first.float(), ref, **tol(ref, atol=0.05))
    for _ in range(4):
        again = e.gemm_nt(a, b, empty, empty, False)
        assert torch.equal(again, first)


@pytest.mark.parametrize("shape", [
    (128, 256, 256), (384, 512, 256), (2048, 1024, 1024),
])
def test_wgrad_tn_256_tier(gpu_device, shape):
    """256-tile 8-phase wgrad (wgrad256.hip): accumulation semantics
    (gw +=) vs f32 torch."""
    Kb, Mo, N = shape
    e = ext()
    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=70)
    x = rand_bf16(Kb, N, device=gpu_device, seed=71)
    gw = torch.randn(Mo, N, device=gpu_device)  # pre-seeded: += check
    want = gw + dy.float().t() @ x.float()
    e.wgrad_tn_256(dy, x, gw)
    torch.testing.assert_close(gw, want, **tol(want, atol=0.05))


def test_wgrad_tn_256_dispatch_with_bias(gpu_device):
    """The production wgrad_tn dispatch at a qualifying wide shape
    (256-tier + separate colsum for gb) matches f32 torch."""
    e = ext()
    Kb, Mo, N = 512, 2048, 2048  # 64 output tiles >= gate
    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=72)
    x = rand_bf16(Kb, N, device=gpu_device, seed=73)
    gw = torch.zeros(Mo, N, device=gpu_device)
    gb = torch.zeros(Mo, device=gpu_device)
    e.wgrad_tn(dy, x, gw, gb, torch.Tensor(), 0)
    rw = dy.float().t() @ x.float()
    torch.testing.assert_close(gw, rw, **tol(rw, atol=0.05))
    torch.testing.assert_close(gb, dy.float().sum(0), **tol(rw, atol=0.05))


def test_fp8_quantize_and_gemm(gpu_device):
    """MX-fp8 tier (csrc/fp8.hip): quantizer + scaled-MFMA GEMM vs the
    dequantized-operand f32 oracle (kernel-exact up to bf16 output
    rounding; quantization noise is excluded by construction)."""
    e = ext()

    def dequant(q, s):
        R, K = q.shape
        qf = q.to(torch.int32)
        sgn = torch.where(qf >= 128, -1.0, 1.0)
        qa = qf & 0x7F
        ee = qa >> 3
        m = (qa & 7).float()
        mag = torch.where(ee == 0, (m / 8.0) * 2.0 ** -6,
                          (1 + m / 8.0) * torch.pow(2.0, ee.float() - 7))
        k = torch.arange(K, device=q.device)
        g = ((k >> 6) & 1) + 2 * ((k >> 4) & 1)
        w = k >> 7
        sc = s.to(torch.int32)[w, :, g].t().float()
        return sgn * mag * torch.pow(2.0, sc - 127)

    for (M, N, K, bias_on, relu) in [(256, 256, 256, False, False),
                                     (512, 512, 512, True, True)]:
        a = rand_bf16(M, K, device=gpu_device, seed=80)
        b = rand_bf16(N, K, device=gpu_device, seed=81)
        bias = (rand_bf16(N, device=gpu_device, seed=82) if bias_on
                else torch.Tensor())
        qa, sa = e.fp8_quantize(a)
        qb, sb = e.fp8_quantize(b)
        c = e.gemm_nt_f8(qa, sa, qb, sb, bias, relu)
        want = dequant(qa, sa) @ dequant(qb, sb).t()
        if bias_on:
            want = want + bias.float()
        if relu:
            want = torch.clamp(want, min=0)
        torch.testing.assert_close(c.float(), want, **tol(want, atol=0.05))
        # quantization quality: e2e error vs bf16 math bounded
        full = a.float() @ b.float().t()
        if bias_on:
            full += bias.float()
        if relu:
            full = torch.clamp(full, min=0)
        denom = full.abs().mean().clamp_min(1.0)
        assert ((c.float() - full).abs() / denom).mean().item() < 0.05


def test_fp8_serving_cli(gpu_device, tmp_path):
    """infer.py --fp8 end-to-end: runs, and predictions agree with the
    bf16 path on the overwhelming majority of samples (fp8
    quantization may flip a few near-ties)."""
    import json
    import subprocess
    import sys as _sys

    outs = {}
    for flag in ([], ["--fp8"]):
        res = subprocess.run(
            [_sys.executable, "infer.py", "--batch", "256", "--samples",
             "512", "--layer-sizes", "256,512,512,256",
             "--out", str(tmp_path / f"p{len(flag)}.pt")] + flag,
            capture_output=True, text=True, timeout=300, check=True)
        j = json.loads([l for l in res.stdout.splitlines()
                        if l.startswith("{")][0])
        assert j["inference_samples_per_sec"] > 0
        outs[len(flag)] = torch.load(tmp_path / f"p{len(flag)}.pt",
                                     weights_only=False)
    agree = (outs[0] == outs[1]).float().mean().item()
    # random-init logits over 256 classes are near-ties, so fp8 noise
    # legitimately flips ~10% of argmaxes (measured 0.91); a BROKEN
    # fp8 path agrees at chance (1/256).  Trained-model margins give
    # far higher agreement (infer --fp8 A/B in profiles/).
    assert agree > 0.75, f"fp8 predictions diverge: agree={agree}"


def test_fp8_fused_quant_output(gpu_device):
    """gemm_nt_f8_q (EMIT_Q epilogue): dequantized fused output equals
    the bf16-out path within one e4m3 ulp."""
    e = ext()
    M = N = K = 256
    a = rand_bf16(M, K, device=gpu_device, seed=90)
    b = rand_bf16(N, K, device=gpu_device, seed=91)
    qa, sa = e.fp8_quantize(a)
    qb, sb = e.fp8_quantize(b)
    c16 = e.gemm_nt_f8(qa, sa, qb, sb, torch.Tensor(), False).float()
    cq, cs = e.gemm_nt_f8_q(qa, sa, qb, sb, torch.Tensor(), False)
    # dequant (same as test_fp8_quantize_and_gemm)
    qf = cq.to(torch.int32)
    sgn = torch.where(qf >= 128, -1.0, 1.0)
    qq = qf & 0x7F
    ee = qq >> 3
    m = (qq & 7).float()
    mag = torch.where(ee == 0, (m / 8.0) * 2.0 ** -6,
                      (1 + m / 8.0) * torch.pow(2.0, ee.float() - 7))
    k = torch.arange(N, device=gpu_device)
    g = ((k >> 6) & 1) + 2 * ((k >> 4) & 1)
    w = k >> 7
    sc = cs.to(torch.int32)[w, :, g].t().float()
    cd = sgn * mag * torch.pow(2.0, sc - 127)
    rel = ((cd - c16).abs() / c16.abs().clamp_min(4.0)).max().item()
    assert rel < 0.07, rel


def test_fused_mlp_fwd_matches_eager(gpu_device):
    """Persistent fused-MLP forward (csrc/fused_mlp.hip): same bf16
    rounding points and k-accumulation order as the eager layer chain,
    so per-row argmax must match exactly."""
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.ops import load_ext
    from shallowspeed_amd.ops.functional import row_argmax

    e = load_ext(required=True)
    for sizes, rows in (([784, 256, 256, 256, 10], 1024),
                        ([784, 256, 256, 256, 256, 256, 256, 10], 448),
                        ([100, 256, 10], 64)):
        model = MLP(sizes, 0, 1, rows, loss="xent").materialize_device(
            gpu_device)
        model.eval()
        g = torch.Generator().manual_seed(len(sizes))
        x = torch.randn(rows, sizes[0], generator=g).bfloat16().to(gpu_device)
        probs = model.forward(x)
        want = row_argmax(probs)
        import infer as infer_mod

        plan = infer_mod.build_fused_plan(model, rows)
        assert plan is not None, sizes
        desc, ind, nh, co = plan
        got = e.fused_mlp_argmax(x, desc, ind, nh, co)
        torch.cuda.synchronize()
        # The fused head argmaxes UNROUNDED f32 logits; the eager path
        # argmaxes bf16-rounded probs.  On a random-init model the
        # near-uniform probs produce exact bf16 ties, where the two may
        # legally pick different (equal-prob) classes — every
        # disagreement must be such a tie; anything else is a bug.
        gl = got.long()
        wl = want.long()
        mm = (gl != wl).nonzero().flatten()
        rows_idx = torch.arange(probs.shape[0], device=probs.device)
        p_got = probs[rows_idx, gl]
        p_want = probs[rows_idx, wl]
        if mm.numel():
            assert torch.equal(p_got[mm], p_want[mm]), (
                sizes, mm[:5].tolist())
        assert mm.numel() <= max(1, probs.shape[0] // 50), (
            sizes, mm.numel())  # ties must stay rare


# ------------------------------------- launch ladders, one case per rung

FLAG_COMBOS = [(False, False), (True, False), (False, True), (True, True)]


def _mx_dequant(q, s):
    """e4m3 bytes [R,K] + e8m0 scales [K/128,R,4] -> f32 (the oracle of
    test_fp8_quantize_and_gemm)."""
    K = q.shape[1]
    qf = q.to(torch.int32)
    sgn = torch.where(qf >= 128, -1.0, 1.0)
    qa = qf & 0x7F
    ee = qa >> 3
    m = (qa & 7).float()
    mag = torch.where(ee == 0, (m / 8.0) * 2.0 ** -6,
                      (1 + m / 8.0) * torch.pow(2.0, ee.float() - 7))
    k = torch.arange(K, device=q.device)
    g = ((k >> 6) & 1) + 2 * ((k >> 4) & 1)
    sc = s.to(torch.int32)[k >> 7, :, g].t().float()
    return sgn * mag * torch.pow(2.0, sc - 127)


def _epilogue(ref, bias, bias_on, relu):
    if bias_on:
        ref = ref + bias.float()
    return torch.clamp(ref, min=0) if relu else ref


@pytest.mark.parametrize("shape", [
    (32, 64, 32), (1024, 768, 32), (8200, 1024, 32), (8192, 1024, 32),
], ids=["rows32", "rows64", "reg128", "glds"])
def test_gemm_nt_epilogue_ladder(gpu_device, shape):
    """Every (bias, relu) combination plus mask-alone through each
    gemm_nt tier, so a ladder with swapped or dropped flags fails.  The
    gates of ss_gemm_nt send the shapes to their tiers:
      32x64x32      M < 48 -> 32-row configuration
      1024x768x32   16x12 = 192 blocks of 64^2 (not < 192) and 8x6 = 48
                    blocks of 128^2 (< 512) -> 64-row configuration
      8200x1024x32  65x8 = 520 blocks of 128^2 (>= 512); M % 128 != 0
                    keeps it off the glds tier, M % 256 != 0 makes the
                    256 tier decline -> 128^2 register-staged kernel
      8192x1024x32  64x8 = 512 aligned blocks of 128^2; K % 128 != 0
                    makes the 256 tier decline -> gemm_nt_glds_kernel
    A mask keeps every shape off the 256 and glds tiers, so mask-alone
    at the last shape runs the masked 128^2 register-staged kernel."""
    M, N, K = shape
    e = ext()
    a = rand_bf16(M, K, device=gpu_device, seed=100)
    b = rand_bf16(N, K, device=gpu_device, seed=101)
    bias = rand_bf16(N, device=gpu_device, seed=102)
    mask = rand_bf16(M, K, device=gpu_device, seed=103)
    empty = torch.Tensor()
    base = a.float() @ b.float().t()
    for bias_on, relu in FLAG_COMBOS:
        c = e.gemm_nt(a, b, bias if bias_on else empty, empty, relu)
        ref = _epilogue(base, bias, bias_on, relu)
        torch.testing.assert_close(c.float(), ref, **tol(ref),
                                   msg=lambda m: f"{bias_on=} {relu=}: {m}")
    c = e.gemm_nt(a, b, empty, mask, False)
    ref = (a.float() * (mask.float() > 0)) @ b.float().t()
    torch.testing.assert_close(c.float(), ref, **tol(ref))


def test_gemm_nt_f8_epilogue_ladder(gpu_device):
    """All four (bias, relu) combinations of gemm_nt_f8 against the
    dequantised-operand oracle, and of gemm_nt_f8_q against the
    bf16-output call (within one e4m3 ulp, as
    test_fp8_fused_quant_output), at 256x256x256 (one 256-tile)."""
    e = ext()
    M = N = K = 256
    a = rand_bf16(M, K, device=gpu_device, seed=110)
    b = rand_bf16(N, K, device=gpu_device, seed=111)
    bias = rand_bf16(N, device=gpu_device, seed=112)
    qa, sa = e.fp8_quantize(a)
    qb, sb = e.fp8_quantize(b)
    base = _mx_dequant(qa, sa) @ _mx_dequant(qb, sb).t()
    for bias_on, relu in FLAG_COMBOS:
        bt = bias if bias_on else torch.Tensor()
        c16 = e.gemm_nt_f8(qa, sa, qb, sb, bt, relu).float()
        want = _epilogue(base, bias, bias_on, relu)
        torch.testing.assert_close(c16, want, **tol(want, atol=0.05),
                                   msg=lambda m: f"{bias_on=} {relu=}: {m}")
        cq, cs = e.gemm_nt_f8_q(qa, sa, qb, sb, bt, relu)
        cd = _mx_dequant(cq, cs)
        rel = ((cd - c16).abs() / c16.abs().clamp_min(4.0)).max().item()
        assert rel < 0.07, (bias_on, relu, rel)


@pytest.mark.parametrize("bias_on,relu", FLAG_COMBOS)
def test_gemm_nt_256w_epilogue_ladder(gpu_device, bias_on, relu):
    """The 4-wave 256-tile variant (gemm256w.hip) with each (bias, relu)
    combination at 256x256x128 (one tile, one K-step pair) vs f32 torch."""
    e = ext()
    M, N, K = 256, 256, 128
    a = rand_bf16(M, K, device=gpu_device, seed=120)
    b = rand_bf16(N, K, device=gpu_device, seed=121)
    bias = rand_bf16(N, device=gpu_device, seed=122)
    c = e.gemm_nt_256w(a, b, bias if bias_on else torch.Tensor(), relu)
    ref = _epilogue(a.float() @ b.float().t(), bias, bias_on, relu)
    torch.testing.assert_close(c.float(), ref, **tol(ref, atol=0.05))


@pytest.mark.parametrize("N", [2048, 40])
@pytest.mark.parametrize("masked", [False, True])
def test_colsum_mask_ladder(gpu_device, N, masked):
    """Standalone colsum with and without mask: N = 2048 takes the
    8-wide kernel (N % 8 == 0 and N >= 2048), N = 40 the scalar one."""
    e = ext()
    M = 64
    dy = rand_bf16(M, N, device=gpu_device, seed=130)
    mask = rand_bf16(M, N, device=gpu_device, seed=131)
    gb = e.colsum(dy, mask if masked else torch.Tensor())
    ref = dy.float()
    if masked:
        ref = ref * (mask.float() > 0)
    ref = ref.sum(0)
    torch.testing.assert_close(gb, ref, **tol(ref))
