"""Backward chain kernel (csrc/bwd_chain.hip) against the unfused chain
of extension ops it replaces.

dz_head, every dz_l and the final dx must be BIT-identical to
head_bwd_fused -> relu_bwd -> gemm_nt(dz, W^T) -> ...: the kernel runs
the same MFMA with the same operand slots and K-step order, rounds at
the same points and masks by the same `>0` rule.  With the chain on, the
weight gradients run unmasked on dz instead of masked on dh; in
deterministic mode that must not change a bit of any gradient.  In
default mode the split-K partial sums meet in f32 atomics, so a gradient
element is held to the f32 reordering bound of its own sum,

    |g - g_det| <= M * 2^-23 * sum_r |dz[r,o]| * |x[r,i]|,

computed in f64 on the host from the deterministic run's dz and x.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()
H = 256
# (rows, waves, w_lds); zeros = the shipped choice
ARMS = [(0, 0, 0), (32, 4, 0), (32, 8, 0), (64, 4, 0), (64, 8, 0),
        (64, 8, 1)]


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def one_hot(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(M, C)
    t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
    return t


@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_bwd_chain(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    F.set_deterministic(False)


# ------------------------------------------------------------ kernel level

_CASES = {}


def mask_source(M, seed):
    """Post-ReLU-like mask source with positives and negatives and the
    values that pin the `>0` rule: an all-zero row, an all-zero column,
    a -0.0 and one NaN."""
    h = randn(M, H, seed=seed)
    h[:, 7] = 0.0
    if M > 1:
        h[M // 2, :] = 0.0
    h[0, 3] = -0.0
    h[M - 1, 5] = float("nan")
    return h


def chain_case(M, depth, C, device):
    """Seeded inputs and the unfused chain's outputs for `depth` ReLU
    layers with every dgrad run, computed once per shape and shared
    (never modified) by the tests below.  The first k layers' dz do not
    depend on whether layer k's dgrad runs, so a chain that ends early
    compares against a prefix."""
    key = (M, depth, C)
    if key not in _CASES:
        e = ext()
        probs = torch.softmax(randn(M, C, seed=10 + M), dim=1)
        probs = probs.to(device=device, dtype=BF)
        t = one_hot(M, C, seed=20 + M).to(device=device, dtype=BF)
        w_head = (randn(C, H, seed=30 + C) / H ** 0.5).to(device=device,
                                                          dtype=BF)
        w_head_t = w_head.t().contiguous()
        hs = [mask_source(M, seed=40 + 7 * l + M).to(device=device, dtype=BF)
              for l in range(depth)]
        # weights scaled as Linear does: N(0, 1) / sqrt(in_dims)
        w_ts = [(randn(H, H, seed=50 + l) / H ** 0.5)
                .to(device=device, dtype=BF).t().contiguous()
                for l in range(depth)]
        x = torch.zeros(M, H, device=device, dtype=BF)  # read by wgrad only
        dz_head, dh = e.head_bwd_fused(probs, t, x, w_head_t, float(M),
                                       EMPTY, EMPTY)
        dzs, dhs = [], []
        for h, w_t in zip(hs, w_ts):
            dzs.append(e.relu_bwd(dh, h))
            dh = e.gemm_nt(dzs[-1], w_t, EMPTY, EMPTY, False)
            dhs.append(dh)
        _CASES[key] = dict(probs=probs, t=t, w_head_t=w_head_t, hs=hs,
                           w_ts=w_ts, dz_head=dz_head, dzs=dzs, dhs=dhs)
    return _CASES[key]


def same_bits(a, b):
    """torch.equal on the bit patterns (a masked NaN source leaves no
    NaN behind, but a bit compare does not depend on that)."""
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


# M: 1 row; a partial 32-row tile; one 64-row tile (two 32-row tiles);
# 97 = multi-tile with a one-row last tile at both sizes; 200 = four
# 64-row tiles, the last partial
@pytest.mark.parametrize("C", [1, 10, 16])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 31, 64, 97, 200])
def test_chain_bit_identical(gpu_device, M, depth, C):
    from shallowspeed_amd.ops import functional as F

    c = chain_case(M, depth, C, gpu_device)
    for arm in ARMS:
        res = F.bwd_chain(c["probs"], c["t"], c["w_head_t"], M, c["hs"],
                          c["w_ts"], *arm)
        assert res is not None, arm
        dz_head, dzs, dx = res
        assert same_bits(dz_head, c["dz_head"]), arm
        assert len(dzs) == depth
        for l in range(depth):
            assert same_bits(dzs[l], c["dzs"][l]), (arm, l)
        assert same_bits(dx, c["dhs"][-1]), arm


@pytest.mark.parametrize("M", [31, 97])
def test_chain_mask_only_last_layer(gpu_device, M):
    """The last layer's dgrad is skipped (the flagship's first layer):
    its dz still comes out, and there is no dx."""
    from shallowspeed_amd.ops import functional as F

    c = chain_case(M, 3, 10, gpu_device)
    for arm in ARMS:
        dz_head, dzs, dx = F.bwd_chain(c["probs"], c["t"], c["w_head_t"], M,
                                       c["hs"], c["w_ts"][:2], *arm)
        assert dx is None
        assert same_bits(dz_head, c["dz_head"])
        for l in range(3):
            assert same_bits(dzs[l], c["dzs"][l]), (arm, l)


def test_chain_rejects_outside_contract(gpu_device):
    """Width 128, a non-contiguous input, a wrong count of weights and
    an unknown arm launch nothing and return None."""
    from shallowspeed_amd.ops import functional as F

    M = 64
    c = chain_case(M, 2, 10, gpu_device)
    args = (c["probs"], c["t"], c["w_head_t"], M)
    assert F.bwd_chain(*args, c["hs"], c["w_ts"]) is not None
    wide = torch.zeros(M, 2 * H, device=gpu_device, dtype=BF)
    assert F.bwd_chain(*args, [wide[:, ::2], c["hs"][1]], c["w_ts"]) is None
    assert F.bwd_chain(*args, [c["hs"][0].t().contiguous().t(), c["hs"][1]],
                       c["w_ts"]) is None
    assert F.bwd_chain(*args, c["hs"], []) is None
    assert F.bwd_chain(*args, c["hs"], c["w_ts"], 48, 4) is None
    assert F.bwd_chain(*args, c["hs"], c["w_ts"], 32, 4, 1) is None
    # width 128 everywhere
    h128 = torch.ones(M, 128, device=gpu_device, dtype=BF)
    w128 = torch.zeros(128, 128, device=gpu_device, dtype=BF)
    wh128 = torch.zeros(128, 10, device=gpu_device, dtype=BF)
    assert F.bwd_chain(c["probs"], c["t"], wh128, M, [h128], [w128]) is None
    assert ext().bwd_chain(c["probs"], c["t"], wh128, float(M), [h128],
                           [w128]) == []


# ------------------------------------------------------------- model level

B = 96
SIZES = [48, 256, 256, 256, 10]


def _inputs(device, in_dim=SIZES[0]):
    x = randn(B, in_dim, seed=71).to(device=device, dtype=BF)
    t = one_hot(B, SIZES[-1], seed=72).to(device=device, dtype=BF)
    return x, t


def _count_calls(F, monkeypatch):
    calls = {"chain": 0, "chain_ok": 0, "head_bwd": 0, "outs": []}
    chain, bwd = F.bwd_chain, F.head_bwd_fused

    def cc(*a, **k):
        calls["chain"] += 1
        res = chain(*a, **k)
        calls["chain_ok"] += res is not None
        calls["outs"].append(res)
        return res

    def cb(*a, **k):
        calls["head_bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(F, "bwd_chain", cc)
    monkeypatch.setattr(F, "head_bwd_fused", cb)
    return calls


def _train(device, F, chain, det, steps):
    from shallowspeed_amd.models import MLP, SGD

    F.set_bwd_chain(chain)
    F.set_deterministic(det)
    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(device)
    opt = SGD(model.parameters(), lr=0.05)
    x, t = _inputs(device)
    for _ in range(steps):
        model.zero_grad()
        model.forward(x, 0)
        model.backward(t, 0)
        opt.step()
    torch.cuda.synchronize()
    return ([p.data.clone() for p in model.parameters()],
            [p.grad.clone() for p in model.parameters()])


@pytest.mark.parametrize("steps", [1, 3])
def test_model_deterministic_bitwise(gpu_device, flags, monkeypatch, steps):
    F = flags
    calls = _count_calls(F, monkeypatch)
    p_on, g_on = _train(gpu_device, F, True, True, steps)
    assert (calls["chain_ok"], calls["head_bwd"]) == (steps, 0)
    p_off, g_off = _train(gpu_device, F, False, True, steps)
    assert (calls["chain"], calls["head_bwd"]) == (steps, steps)
    for a, b in zip(p_on + g_on, p_off + g_off):
        assert torch.equal(a, b)


def test_model_default_mode_within_reordering_bound(gpu_device, flags,
                                                    monkeypatch):
    from shallowspeed_amd.models import MLP

    F = flags
    # the deterministic run, chain on: record every wgrad's (dz, x)
    seen = {}
    real = F.linear_wgrad_acc

    def rec(dy, x, gw, gb=None, mask_src=None, split_k=0):
        assert mask_src is None, "the chain's wgrads run unmasked"
        seen[gw.data_ptr()] = (dy.double().cpu(), x.double().cpu())
        return real(dy, x, gw, gb, mask_src, split_k)

    def run(det):
        F.set_deterministic(det)
        model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(
            gpu_device)
        x, t = _inputs(gpu_device)
        model.zero_grad()
        model.forward(x, 0)
        model.backward(t, 0)
        torch.cuda.synchronize()
        return model

    monkeypatch.setattr(F, "linear_wgrad_acc", rec)
    ref = run(True)
    assert len(seen) == 4
    monkeypatch.setattr(F, "linear_wgrad_acc", real)
    got = run(False)
    eps = B * 2.0 ** -23
    for lr, lg in zip(ref.layers[:4], got.layers[:4]):
        dz, x = seen[lr.weight.grad.data_ptr()]
        for name, g, r, bound in (
                ("gW", lg.weight.grad, lr.weight.grad,
                 eps * (dz.abs().t() @ x.abs())),
                ("gb", lg.bias.grad, lr.bias.grad, eps * dz.abs().sum(0))):
            err = (g.double().cpu() - r.double().cpu()).abs()
            print(f"{lr.in_dims}->{lr.out_dims} {name}: max err "
                  f"{err.max().item():.3e}, max bound "
                  f"{bound.max().item():.3e}")
            assert (err <= bound).all(), (name, lr.in_dims, lr.out_dims)


def test_model_chain_stop_with_dx_needed(gpu_device, flags, monkeypatch):
    """First layer 48 wide whose dx IS needed (not pipeline stage 0):
    the chain ends at dz_1, which equals relu_bwd(dh_1, h_1), and the
    layer's dx from the ordinary unmasked gemm_nt on dz_1 equals today's
    masked gemm_nt on dh_1."""
    from shallowspeed_amd.models import MLP

    F = flags
    F.set_deterministic(True)
    calls = _count_calls(F, monkeypatch)
    x, t = _inputs(gpu_device)
    out = {}
    for chain in (True, False):
        F.set_bwd_chain(chain)
        model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(
            gpu_device)
        model._skip_input_grad = False
        assert model._bwd_chain_plan(B) == (
            [(2, True), (1, True), (0, False)] if chain else None)
        model.zero_grad()
        model.forward(x, 0)
        h1 = model.layers[0]._cache[("y", 0)]
        dx = model.backward(t, 0)
        out[chain] = (dx, [p.grad.clone() for p in model.parameters()], h1,
                      model.layers[1].weight.compute_t())
    assert (calls["chain_ok"], calls["head_bwd"]) == (1, 1)
    assert out[True][0].shape == (B, SIZES[0])
    assert same_bits(out[True][0], out[False][0])
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.equal(a, b)
    _, dzs, dx_chain = calls["outs"][0]
    assert dx_chain is None and len(dzs) == 3
    dh1 = ext().gemm_nt(dzs[1], out[True][3], EMPTY, EMPTY, False)
    assert same_bits(dzs[2], ext().relu_bwd(dh1, out[True][2]))


def _grads_of(model, x, t):
    model.zero_grad()
    model.forward(x, 0)
    model.backward(t, 0)
    torch.cuda.synchronize()
    return [p.grad.clone() for p in model.parameters()]


def test_model_falls_back_outside_contract(gpu_device, flags, monkeypatch):
    """Width 128 and a GELU layer under the head never reach the chain
    and take today's path (one head_bwd_fused call each); what the
    kernel itself turns down is in test_chain_rejects_outside_contract."""
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.models.layers import (Linear, Sequential,
                                                SoftmaxXent)

    F = flags
    F.set_deterministic(True)
    calls = _count_calls(F, monkeypatch)
    x, t = _inputs(gpu_device)

    narrow = MLP([48, 128, 128, 10], 0, 1, B).materialize_device(gpu_device)
    assert narrow._bwd_chain_plan(B) is None
    _grads_of(narrow, x, t)
    assert (calls["chain"], calls["head_bwd"]) == (0, 1)

    gelu = Sequential([Linear(48, H, "relu"), Linear(H, H, "gelu"),
                       Linear(H, 10), SoftmaxXent(B)])
    gelu.materialize_device(gpu_device)
    assert gelu._bwd_chain_plan(B) is None
    _grads_of(gelu, x, t)
    assert (calls["chain"], calls["head_bwd"]) == (0, 2)


def test_model_mixed_chain_paths(gpu_device, flags):
    """A backward with the chain on or off can follow either forward."""
    from shallowspeed_amd.models import MLP

    F = flags
    F.set_deterministic(True)
    x, t = _inputs(gpu_device)
    grads = []
    for fwd_fused, chain in ((True, True), (False, True), (True, False)):
        model = MLP(SIZES, 0, 1, B).materialize_device(gpu_device)
        model.zero_grad()
        F.set_head_fused(fwd_fused)
        model.forward(x, 0)
        F.set_head_fused(True)
        F.set_bwd_chain(chain)
        model.backward(t, 0)
        assert not any(l._cache for l in model.layers), "stash left behind"
        grads.append([p.grad.clone() for p in model.parameters()])
    for other in grads[:2]:
        for a, b in zip(other, grads[2]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ worker

def _run_worker(device, F, chain):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    F.set_bwd_chain(chain)
    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(device)
    opt = SGD(model.parameters(), lr=0.0)  # keep the weights fixed
    ds = Dataset(B, B // 2, n_samples=B, in_dim=SIZES[0],
                 n_classes=SIZES[-1], device=device).load(0, 1)
    w = Worker(Topology(device=device), model, ds, opt)
    w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), 0)
    torch.cuda.synchronize()
    assert w._defer_active, "two micro-batches should defer the wgrads"
    return [p.grad.clone() for p in model.parameters()]


def test_worker_two_microbatches_deferred(gpu_device, flags, monkeypatch):
    F = flags
    F.set_deterministic(True)
    calls = _count_calls(F, monkeypatch)
    g_on = _run_worker(gpu_device, F, True)
    assert (calls["chain_ok"], calls["head_bwd"]) == (2, 0)
    g_off = _run_worker(gpu_device, F, False)
    assert (calls["chain"], calls["head_bwd"]) == (2, 2)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)


# ----------------------------------------------------------------- metrics

def test_metrics_match_todays_path(gpu_device, flags):
    """With an accumulator set, the chain path (standalone metrics
    launch) and today's path (counted inside head_bwd_fused) agree: the
    integer counts exactly, loss_sum within the f32 reordering bound of
    its own sum, B * 2^-23 * sum_r |loss_r| (f64, host)."""
    from shallowspeed_amd.models import MLP

    F = flags
    x, t = _inputs(gpu_device)
    got = {}
    for chain in (True, False):
        F.set_bwd_chain(chain)
        model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(
            gpu_device)
        acc = F.new_metrics_acc(gpu_device)
        assert model.set_metrics(acc)
        model.zero_grad()
        probs = model.forward(x, 0)
        model.backward(t, 0)
        got[chain] = F.read_metrics_acc(acc)
    on, off = got[True], got[False]
    assert on["rows"] == off["rows"] == B
    assert on["nonfinite"] == off["nonfinite"] == 0
    assert on["correct"] == off["correct"]
    p, tt = probs.double().cpu(), t.double().cpu()
    terms = torch.where(tt != 0, -tt * torch.log(p.clamp(min=1e-38)),
                        torch.zeros_like(p)).sum(1)
    bound = B * 2.0 ** -23 * terms.abs().sum().item()
    print(f"loss_sum on {on['loss_sum']:.9g} off {off['loss_sum']:.9g} "
          f"bound {bound:.3e}")
    assert abs(on["loss_sum"] - off["loss_sum"]) <= bound
