"""Fused classifier head (csrc/head.hip) against the unfused extension
ops it replaces.

probs, dz and dx must be BIT-identical to gemm_nt -> softmax_fwd,
head_xent_bwd and gemm_nt(dz, Wt).  The in-kernel weight/bias gradient
differs only in f32 summation order, so it is held to the worst-case
bound of an f32 sum of M exact products taken in any order,

    |g - ref| <= (M + 8) * 2^-24 * (|dz|^T |x| + |g0|),

with ref = g0 + dz^T x in f64 from the bf16 dz.  The bound does not
depend on the code under test; the existing single-owner wgrad kernel is
checked against it at the same shapes.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def rand_bf16(*shape, device, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return t.to(device=device, dtype=BF)


def tol(ref, atol=1e-2, rtol=2e-2):
    return dict(atol=atol + 1e-3 * ref.abs().max().item(), rtol=rtol)


def one_hot(M, C, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.zeros(M, C)
    t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
    return t.to(device=device, dtype=BF)


def grad_ref_and_bound(dz, x, g0w, g0b, M):
    """f64 reference and elementwise bound for (gW, gb), on the CPU."""
    dzd, xd = dz.double().cpu(), x.double().cpu()
    eps = (M + 8) * 2.0 ** -24
    ref_w = g0w.double().cpu() + dzd.t() @ xd
    ref_b = g0b.double().cpu() + dzd.sum(0)
    bnd_w = eps * (dzd.abs().t() @ xd.abs() + g0w.double().cpu().abs())
    bnd_b = eps * (dzd.abs().sum(0) + g0b.double().cpu().abs())
    return ref_w, ref_b, bnd_w, bnd_b


def assert_within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"max bound {bound.max().item():.3e}, margin {-worst:.3e}")
    assert (err <= bound).all(), (what, err.max().item(), worst)


@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    F.set_deterministic(False)


# ------------------------------------------------------------ kernel level

_INPUTS = {}


def head_case(M, K, C, device):
    """Seeded inputs and the unfused chain's outputs, computed once per
    shape and shared (never modified) by the tests below."""
    key = (M, K, C)
    if key not in _INPUTS:
        e = ext()
        x = rand_bf16(M, K, device=device, seed=100 + M)
        w = rand_bf16(C, K, device=device, scale=K ** -0.5, seed=200 + K)
        b = rand_bf16(C, device=device, scale=0.5, seed=300 + C)
        w_t = w.t().contiguous()
        t = one_hot(M, C, device, seed=400 + M)
        logits = e.gemm_nt(x, w, b, EMPTY, False)
        probs = e.softmax_fwd(logits)
        dz = e.head_xent_bwd(probs, t, float(M))
        dx = e.gemm_nt(dz, w_t, EMPTY, EMPTY, False)
        _INPUTS[key] = dict(x=x, w=w, b=b, w_t=w_t, t=t, probs=probs, dz=dz,
                            dx=dx)
    return _INPUTS[key]


MS = [1, 15, 64, 65, 200, 1027]
KCS = [(32, 10), (256, 10), (256, 16), (96, 3)]


@pytest.mark.parametrize("KC", KCS, ids=lambda kc: f"K{kc[0]}C{kc[1]}")
@pytest.mark.parametrize("M", MS)
def test_fused_outputs_bit_identical(gpu_device, M, KC):
    K, C = KC
    e = ext()
    c = head_case(M, K, C, gpu_device)
    probs = e.head_fwd_fused(c["x"], c["w"], c["b"])
    assert probs.shape == (M, C) and probs.dtype == BF
    assert torch.equal(probs, c["probs"])
    gw = torch.zeros(C, K, device=gpu_device)
    gb = torch.zeros(C, device=gpu_device)
    dz, dx = e.head_bwd_fused(probs, c["t"], c["x"], c["w_t"], float(M), gw,
                              gb)
    assert torch.equal(dz, c["dz"])
    assert torch.equal(dx, c["dx"])
    # without the in-kernel wgrad the same dz / dx come out
    dz2, dx2 = e.head_bwd_fused(probs, c["t"], c["x"], c["w_t"], float(M),
                                EMPTY, EMPTY)
    assert torch.equal(dz2, c["dz"])
    assert torch.equal(dx2, c["dx"])


@pytest.mark.parametrize("start", ["zeros", "seeded"])
@pytest.mark.parametrize("KC", KCS, ids=lambda kc: f"K{kc[0]}C{kc[1]}")
@pytest.mark.parametrize("M", MS)
def test_fused_wgrad_within_f32_bound(gpu_device, M, KC, start):
    K, C = KC
    e = ext()
    c = head_case(M, K, C, gpu_device)
    if start == "zeros":
        g0w = torch.zeros(C, K, device=gpu_device)
        g0b = torch.zeros(C, device=gpu_device)
    else:
        g0w = rand_bf16(C, K, device=gpu_device, seed=7).float() * 1.37
        g0b = rand_bf16(C, device=gpu_device, seed=8).float() * 0.73
    ref_w, ref_b, bnd_w, bnd_b = grad_ref_and_bound(c["dz"], c["x"], g0w, g0b,
                                                    M)
    # the existing single-owner kernel defines what the bound must admit
    ow, ob = g0w.clone(), g0b.clone()
    e.wgrad_tn(c["dz"], c["x"], ow, ob, EMPTY, 1)
    assert_within(ow, ref_w, bnd_w, "wgrad_tn split_k=1 gW")
    assert_within(ob, ref_b, bnd_b, "wgrad_tn split_k=1 gb")

    gw, gb = g0w.clone(), g0b.clone()
    e.head_bwd_fused(c["probs"], c["t"], c["x"], c["w_t"], float(M), gw, gb)
    assert_within(gw, ref_w, bnd_w, "fused gW")
    assert_within(gb, ref_b, bnd_b, "fused gb")

    # the kernel ACCUMULATES: a second call (a second micro-batch with
    # the same rows) adds the same gradient again
    e.head_bwd_fused(c["probs"], c["t"], c["x"], c["w_t"], float(M), gw, gb)
    g0w64, g0b64 = g0w.double().cpu(), g0b.double().cpu()
    assert_within(gw, g0w64 + 2 * (ref_w - g0w64), bnd_w, "fused gW twice")
    assert_within(gb, g0b64 + 2 * (ref_b - g0b64), bnd_b, "fused gb twice")


def test_fused_bwd_without_grads_leaves_buffers_alone(gpu_device):
    e = ext()
    M, K, C = 200, 256, 10
    c = head_case(M, K, C, gpu_device)
    # grad buffers laid out as in a model: one flat buffer, gW then gb
    flat = torch.full((C * K + C + 64,), -777.25, device=gpu_device)
    dz, dx = e.head_bwd_fused(c["probs"], c["t"], c["x"], c["w_t"], float(M),
                              EMPTY, EMPTY)
    torch.cuda.synchronize()
    assert torch.equal(dz, c["dz"]) and torch.equal(dx, c["dx"])
    assert (flat == -777.25).all()


def test_fused_contract_is_enforced(gpu_device):
    e = ext()
    x = rand_bf16(8, 40, device=gpu_device)
    w = rand_bf16(10, 40, device=gpu_device)
    b = rand_bf16(10, device=gpu_device)
    with pytest.raises(RuntimeError):
        e.head_fwd_fused(x, w, b)
    x = rand_bf16(8, 64, device=gpu_device)
    w = rand_bf16(17, 64, device=gpu_device)
    b = rand_bf16(17, device=gpu_device)
    with pytest.raises(RuntimeError):
        e.head_fwd_fused(x, w, b)


# ---------------------------------------------------------------- fallback

@pytest.mark.parametrize("sizes,loss", [
    ([48, 40, 10], "xent"),   # K = 40: not a multiple of 32
    ([64, 64, 17], "xent"),   # C = 17 > 16
    ([64, 64, 10], "mse"),    # softmax-MSE head
], ids=["K40", "C17", "mse"])
def test_fallback_takes_old_path(gpu_device, flags, monkeypatch, sizes, loss):
    from shallowspeed_amd.models import MLP

    F = flags
    F.set_head_fused(True)

    def boom(*a, **k):
        raise AssertionError("fused head op called outside its contract")

    monkeypatch.setattr(F, "head_fwd_fused", boom)
    monkeypatch.setattr(F, "head_bwd_fused", boom)
    B = 72
    x = torch.randn(B, sizes[0], generator=torch.Generator().manual_seed(5))
    t = one_hot(B, sizes[-1], "cpu", seed=6).float()

    def run(device):
        model = MLP(sizes, 0, 1, B, loss=loss).materialize_device(device)
        dt = BF if torch.device(device).type == "cuda" else torch.float32
        model.zero_grad()
        p = model.forward(x.to(device=device, dtype=dt), 0)
        model.backward(t.to(device=device, dtype=dt), 0)
        return p.float().cpu(), [q.grad.float().cpu()
                                 for q in model.parameters()]

    got_p, got_g = run(gpu_device)
    want_p, want_g = run("cpu")
    torch.testing.assert_close(got_p, want_p, **tol(want_p))
    for g, r in zip(got_g, want_g):
        torch.testing.assert_close(g, r, **tol(r))


# ------------------------------------------------------------- model level

B_MODEL = 200
SIZES = [64, 64, 10]


def _model_inputs(device):
    x = rand_bf16(B_MODEL, SIZES[0], device=device, seed=21)
    t = one_hot(B_MODEL, SIZES[-1], device, seed=22)
    return x, t


def _head_bound(model, x, t):
    """Reference and bound of the head Linear's gradients, from the
    unfused ops (x of the head and dz are the same bits on both paths)."""
    from shallowspeed_amd.ops import functional as F

    l0, l1 = model.layers[0], model.layers[1]
    xh = F.linear_fwd(x, l0.weight.compute(), l0.bias.compute(), relu=True)
    probs = F.softmax_fwd(F.linear_fwd(xh, l1.weight.compute(),
                                       l1.bias.compute()))
    dz = F.head_softmax_xent_bwd(probs, t, B_MODEL)
    z = torch.zeros(1)
    return grad_ref_and_bound(dz, xh, z, z, B_MODEL)


def _run_model(device, F, fused, det):
    from shallowspeed_amd.models import MLP

    F.set_head_fused(fused)
    F.set_deterministic(det)
    model = MLP(SIZES, 0, 1, B_MODEL, loss="xent").materialize_device(device)
    x, t = _model_inputs(device)
    model.zero_grad()
    probs = model.forward(x, 0)
    model.backward(t, 0)
    torch.cuda.synchronize()
    return model, probs, [p.grad.clone() for p in model.parameters()]


def _count_fused_calls(F, monkeypatch):
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = F.head_fwd_fused, F.head_bwd_fused

    def cf(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def cb(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(F, "head_fwd_fused", cf)
    monkeypatch.setattr(F, "head_bwd_fused", cb)
    return calls


@pytest.mark.parametrize("wgrad_in_kernel", [False, True],
                         ids=["wgrad_tn", "wgrad_in_kernel"])
def test_model_fused_vs_unfused(gpu_device, flags, monkeypatch,
                                wgrad_in_kernel):
    F = flags
    F.set_head_wgrad_fused(wgrad_in_kernel)
    calls = _count_fused_calls(F, monkeypatch)
    wgrads = []
    real_wgrad = F.linear_wgrad_acc
    monkeypatch.setattr(
        F, "linear_wgrad_acc",
        lambda dy, *a, **k: (wgrads.append(dy.shape[1]),
                             real_wgrad(dy, *a, **k))[1])
    model, p_on, g_on = _run_model(gpu_device, F, True, False)
    assert calls == {"fwd": 1, "bwd": 1}
    # the head's own wgrad launch (10 outputs) is there exactly when the
    # gradient does not ride in the fused kernel
    assert (SIZES[-1] in wgrads) == (not wgrad_in_kernel)
    _, p_off, g_off = _run_model(gpu_device, F, False, False)
    assert calls == {"fwd": 1, "bwd": 1}
    assert torch.equal(p_on, p_off)
    # parameters(): [W0, b0, W1, b1]; the non-head grads depend on dx only
    assert torch.equal(g_on[0], g_off[0])
    assert torch.equal(g_on[1], g_off[1])
    x, t = _model_inputs(gpu_device)
    ref_w, ref_b, bnd_w, bnd_b = _head_bound(model, x, t)
    for name, g in (("fused", g_on), ("unfused", g_off)):
        assert_within(g[2], ref_w, bnd_w, f"{name} head gW")
        assert_within(g[3], ref_b, bnd_b, f"{name} head gb")


def test_model_fused_deterministic_bitwise(gpu_device, flags):
    F = flags
    _, p_on, g_on = _run_model(gpu_device, F, True, True)
    _, p_off, g_off = _run_model(gpu_device, F, False, True)
    assert torch.equal(p_on, p_off)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)


def test_model_mixed_forward_backward_paths(gpu_device, flags):
    """Either backward path can follow either forward path."""
    from shallowspeed_amd.models import MLP

    F = flags
    F.set_deterministic(True)
    x, t = _model_inputs(gpu_device)
    grads = []
    for fwd_fused, bwd_fused in ((True, False), (False, True), (False, False)):
        model = MLP(SIZES, 0, 1, B_MODEL, loss="xent")
        model.materialize_device(gpu_device)
        model.zero_grad()
        F.set_head_fused(fwd_fused)
        model.forward(x, 0)
        F.set_head_fused(bwd_fused)
        model.backward(t, 0)
        grads.append([p.grad.clone() for p in model.parameters()])
    for other in grads[:2]:
        for a, b in zip(other, grads[2]):
            assert torch.equal(a, b)


def _run_worker(device, F, fused, det):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    F.set_head_fused(fused)
    F.set_deterministic(det)
    model = MLP(SIZES, 0, 1, B_MODEL, loss="xent").materialize_device(device)
    opt = SGD(model.parameters(), lr=0.0)  # keep the weights fixed
    ds = Dataset(B_MODEL, B_MODEL // 2, n_samples=B_MODEL, in_dim=SIZES[0],
                 n_classes=SIZES[-1], device=device).load(0, 1)
    w = Worker(Topology(device=device), model, ds, opt)
    w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), 0)
    torch.cuda.synchronize()
    assert w._defer_active, "two micro-batches should defer the wgrads"
    return model, ds, [p.grad.clone() for p in model.parameters()]


def test_worker_two_microbatches_deferred(gpu_device, flags, monkeypatch):
    F = flags
    calls = _count_fused_calls(F, monkeypatch)
    model, ds, g_on = _run_worker(gpu_device, F, True, False)
    assert calls == {"fwd": 2, "bwd": 2}
    _, _, g_off = _run_worker(gpu_device, F, False, False)
    assert calls == {"fwd": 2, "bwd": 2}
    # two chunks of one block each per element: a two-term f32 sum,
    # which is the same in either order
    assert torch.equal(g_on[0], g_off[0])
    assert torch.equal(g_on[1], g_off[1])
    x = ds.x_compute[:B_MODEL]
    t = ds.y_compute[:B_MODEL]
    ref_w, ref_b, bnd_w, bnd_b = _head_bound(model, x, t)
    for name, g in (("fused", g_on), ("unfused", g_off)):
        assert_within(g[2], ref_w, bnd_w, f"{name} deferred head gW")
        assert_within(g[3], ref_b, bnd_b, f"{name} deferred head gb")
    _, _, d_on = _run_worker(gpu_device, F, True, True)
    _, _, d_off = _run_worker(gpu_device, F, False, True)
    for a, b in zip(d_on, d_off):
        assert torch.equal(a, b)
