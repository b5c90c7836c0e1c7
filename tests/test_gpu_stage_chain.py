"""Stage arms of the chain kernels (F.fwd_chain_stage / F.bwd_chain_stage:
a pipeline stage with no loss head) against the extension ops they
replace, bit for bit, and against float64.

The float64 checks take every layer's input from the kernel's own output
of the layer before (bf16 values, exact in f64), so errors do not
compound.  For one output, with v = sum_k a_k w_k (+ b) in f64,

    |out - f(v)| <= e + 2^-8 * (|f(v)| + e),
    e = K * 2^-23 * (sum_k |a_k||w_k| + |b|):

e covers any order of the f32 accumulation over K terms, 2^-8 is bf16's
unit roundoff for the one rounding, and f (ReLU, or the identity) is
1-Lipschitz.  Elements whose bound is not finite (a NaN or inf among the
inputs) or whose reference rounds to bf16 inf are compared by class.
"""

import pytest
import torch

from test_gpu_fwd_chain import (ARMS, BF, EMPTY, H, chain_case, ext, randn,
                                same_bits)

pytestmark = pytest.mark.gpu

U_BF, U_F32 = 2.0 ** -8, 2.0 ** -23
BF_INF_FROM = 2.0 ** 128 - 2.0 ** 119   # bf16_max + ulp/2 rounds to inf
MS = [1, 31, 64, 97, 200]               # as tests/test_gpu_fwd_chain.py
SCALE = 1 / 0.75


@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_fwd_chain(True)
    F.set_bwd_chain(True)
    F.set_deterministic(False)


def within_f64(got, a, w, b, relu, scale=1.0, kept=None):
    """The docstring's bound for got = bf16(f(a @ w^T + b)) on the
    elements `kept`; with scale != 1 the result is scaled in f32
    (2^-23) and rounded a second time (2^-8).  Returns how many elements
    of rows with finite inputs went to the class compare."""
    a, w = a.double().cpu(), w.double().cpu()
    bias = 0.0 if b is None else b.double().cpu()
    got = got.double().cpu()
    v = a @ w.t() + bias
    e = a.shape[1] * U_F32 * (a.abs() @ w.abs().t() + abs(bias))
    ref = torch.where(v > 0, v, torch.zeros_like(v)) if relu else v
    bound = e + U_BF * (ref.abs() + e)
    if scale != 1.0:
        bound = scale * bound + (U_BF + U_F32) * scale * (ref.abs() + bound)
        ref = ref * scale
    by_class = ~torch.isfinite(e) | (ref.abs() >= BF_INF_FROM)
    cls = torch.where(ref >= BF_INF_FROM, float("inf"), torch.where(
        ref <= -BF_INF_FROM, -float("inf"), torch.nan_to_num(ref, nan=0.0)))
    kept = torch.ones_like(by_class) if kept is None else kept.cpu()
    num = kept & ~by_class
    assert ((got - ref).abs() <= bound)[num].all()
    sel = kept & by_class & ~torch.isnan(v)
    assert torch.equal(got[sel], cls[sel])
    if relu:  # a NaN pre-activation leaves +0
        assert (got[kept & torch.isnan(v)] == 0).all()
    return int((by_class & torch.isfinite(a).all(1)[:, None]).sum())


# --------------------------------------------------------------- forward

@pytest.mark.parametrize("K0", [256, 784, 40])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("M", MS)
def test_fwd_stage_bits_and_f64(gpu_device, M, depth, K0):
    from shallowspeed_amd.ops import functional as F

    c = chain_case(M, depth, 10, K0, gpu_device)
    for arm in ARMS:
        for l1 in ((0, 1, 2) if K0 == H else (0, 2)):
            hs = F.fwd_chain_stage(c["x"], c["ws"], c["bs"], *arm, l1=l1)
            assert hs is not None and len(hs) == depth, (arm, l1)
            for l, (h, ref) in enumerate(zip(hs, c["hs"])):
                assert same_bits(h, ref), (arm, l1, l)
    a = c["x"]
    for h, w, b in zip(hs, c["ws"], c["bs"]):
        # left to the class compare among rows with finite inputs: the
        # one element built to round to bf16 inf (layer 0, M > 3)
        left_out = within_f64(h, a, w, b, relu=True)
        assert left_out <= 1 and left_out < 0.01 * h.numel()
        a = h


# -------------------------------------------------------------- backward

_BWD = {}


def bwd_case(M, depth, device):
    """hs from a forward (realistic masks) with a -0.0 and a NaN planted,
    a seeded dout with an inf at a kept and at a masked position, and the
    unfused chain's outputs for both scales; shared, never modified."""
    if (M, depth) not in _BWD:
        from shallowspeed_amd.ops import functional as F

        c = chain_case(M, 3, 10, H, device)
        hs = [h.clone() for h in c["hs"][::-1][:depth]]   # top first
        hs[0][0, 3] = -0.0
        hs[-1][M - 1, 5] = float("nan")
        hs[0][0, 11], hs[0][0, 12] = 1.0, 0.0
        w_ts = [w.t().contiguous() for w in c["ws"][::-1][:depth]]
        dout = (randn(M, H, seed=90 + M) / 64).to(device=device, dtype=BF)
        dout[0, 11] = dout[0, 12] = float("inf")          # kept, masked
        ref = {}
        for s in (1.0, SCALE):
            dzs, dh = [], dout
            for h, w_t in zip(hs, w_ts):
                dzs.append(F.relu_bwd(dh, h, scale=s))
                dh = ext().gemm_nt(dzs[-1], w_t, EMPTY, EMPTY, False)
            ref[s] = (dzs, dh)
        _BWD[M, depth] = dict(hs=hs, w_ts=w_ts, dout=dout, ref=ref)
    return _BWD[M, depth]


@pytest.mark.parametrize("scale", [1.0, SCALE])
@pytest.mark.parametrize("last_in", [True, False])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("M", MS)
def test_bwd_stage_bits_and_f64(gpu_device, M, depth, last_in, scale):
    from shallowspeed_amd.ops import functional as F

    c = bwd_case(M, depth, gpu_device)
    hs, dout = c["hs"], c["dout"]
    w_ts = c["w_ts"] if last_in else c["w_ts"][:-1]
    ref_dzs, ref_dx = c["ref"][scale]
    for rows, waves in ARMS:
        for w_lds in ((0, 1) if (rows, waves) == (64, 8) else (0,)):
            res = F.bwd_chain_stage(dout, hs, w_ts, rows, waves, w_lds,
                                    dz_scale=scale)
            if scale != 1.0 and (waves == 4 or w_lds):
                assert res is None  # scaled: the arms that ship only
                continue
            dzs, dx = res
            assert len(dzs) == depth and (dx is not None) == last_in
            for l, (dz, ref) in enumerate(zip(dzs, ref_dzs)):
                assert same_bits(dz, ref), (rows, waves, w_lds, l)
            assert dx is None or same_bits(dx, ref_dx)
    assert torch.isinf(dzs[0][0, 11]) and dzs[0][0, 12] == 0
    # dz_0 is dout itself where kept (scaled: one more rounding), else +0
    kept = hs[0].float() > 0
    d0, want = dzs[0].double(), dout.double() * scale
    assert (d0[~kept] == 0).all() and not torch.signbit(d0[~kept]).any()
    fin = kept & torch.isfinite(want)
    u = (U_BF + U_F32) * (scale != 1.0)   # f32 product, one rounding
    assert ((d0 - want).abs() <= u * want.abs())[fin].all()
    # every dh from the kernel's own dz above it, seen through the next mask
    for l in range(1, depth):
        within_f64(dzs[l], dzs[l - 1], w_ts[l - 1], None, relu=False,
                   scale=scale, kept=hs[l].float() > 0)
    if last_in:
        within_f64(dx, dzs[-1], w_ts[-1], None, relu=False)


def test_stage_ops_reject_outside_contract(gpu_device):
    """Nothing is allocated or launched (the bindings return [] before an
    output tensor exists) and None comes back."""
    from shallowspeed_amd.ops import functional as F

    M = 64
    c, b = chain_case(M, 2, 10, H, gpu_device), bwd_case(M, 2, gpu_device)
    x, ws, bs = c["x"], c["ws"], c["bs"]
    dout, hs, w_ts = b["dout"], b["hs"], b["w_ts"]
    assert F.fwd_chain_stage(x, ws, bs) is not None
    assert F.bwd_chain_stage(dout, hs, w_ts) is not None

    def zeros(*shape):
        return torch.zeros(*shape, device=gpu_device, dtype=BF)

    def off(t):  # contiguous, two bytes off a 16-byte boundary
        o = zeros(t.numel() + 8)[1:1 + t.numel()].view(t.shape)
        assert o.is_contiguous() and o.data_ptr() % 16 == 2
        return o

    fwd_bad = [
        (x, [zeros(128, H)], [zeros(128)]),              # width 128
        (x, [ws[0], zeros(H, 128)], bs),
        (x, [ws[1]] * 9, [bs[1]] * 9),                   # nine layers
        (off(x), ws, bs), (x, [ws[0], off(ws[1])], bs),  # misaligned
        (zeros(M, 2 * H)[:, ::2], ws, bs), (x.float(), ws, bs),
        (x, ws, bs[:1]), (x, [], []),
        (zeros(M, 36), [zeros(H, 36)], bs[:1]),          # K0 = 36
    ]
    for args in fwd_bad:
        assert F.fwd_chain_stage(*args) is None
        assert ext().fwd_chain_stage(*args, 0, 0, 0, 0) == []
    assert F.fwd_chain_stage(x, [ws[1]] * 8, [bs[1]] * 8) is not None
    c784 = chain_case(M, 1, 10, 784, gpu_device)
    assert F.fwd_chain_stage(c784["x"], c784["ws"], c784["bs"], l1=1) is None
    bwd_bad = [
        (zeros(M, 128), [zeros(M, 128)], [zeros(128, 128)]),  # width 128
        (dout, [hs[0]] * 9, [w_ts[0]] * 9),                   # nine layers
        (off(dout), hs, w_ts), (dout, hs, [w_ts[0], off(w_ts[1])]),
        (dout, [hs[0], off(hs[1])], w_ts),
        (zeros(M, 2 * H)[:, ::2], hs, w_ts), (dout.float(), hs, w_ts),
        (dout, hs, []), (dout, hs, w_ts * 2), (dout, [], []),
    ]
    for args in bwd_bad:
        assert F.bwd_chain_stage(*args) is None
        assert ext().bwd_chain_stage(*args, 0, 0, 0, 1.0) == []
    for arm in ((48, 4), (64, 2)):                            # unknown arms
        assert F.fwd_chain_stage(x, ws, bs, *arm) is None
        assert F.bwd_chain_stage(dout, hs, w_ts, *arm) is None
    assert F.bwd_chain_stage(dout, hs, w_ts, 32, 8, 1) is None


# ----------------------------------------------------------- model level

B = 200


def stage_models():
    """(model, layers in the plan, whether backward returns dx)."""
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.models.layers import Linear, Sequential

    return {
        "pp2_stage0": lambda: (MLP([784] + [256] * 4 + [10], 0, 2, B), 3,
                               False),
        "pp3_stage1": lambda: (MLP([256] * 8 + [10], 1, 3, B), 3, True),
        "bottom_48": lambda: (Sequential(
            [Linear(48, H, "relu"), Linear(H, H, "relu")]), 2, True),
    }


def run_stage(make, device, F, fwd, bwd, det=True):
    """One forward + backward of a fresh stage model: (stashes after the
    forward, h_top, dx, gradients)."""
    model, n, _ = make()
    model.materialize_device(device)
    x = randn(B, model.layers[0].in_dims, seed=71).to(device=device, dtype=BF)
    dout = (randn(B, H, seed=72) / 64).to(device=device, dtype=BF)
    F.set_deterministic(det)
    model.zero_grad()
    F.set_fwd_chain(fwd)
    h_top = model.forward(x, 0)
    stash = [dict(l._cache) for l in model.layers]
    F.set_bwd_chain(bwd)
    dx = model.backward(dout, 0)
    torch.cuda.synchronize()
    assert not any(l._cache for l in model.layers), "stash left behind"
    return stash, h_top, dx, [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("name", ["pp2_stage0", "pp3_stage1", "bottom_48"])
def test_model_stage_one_launch_each_way_bitwise(gpu_device, flags,
                                                 monkeypatch, name):
    F = flags
    make = stage_models()[name]
    _, n, has_dx = make()
    calls = dict.fromkeys(("fwd_chain_stage", "bwd_chain_stage",
                           "linear_fwd", "linear_dgrad"), 0)
    for op in calls:
        def counted(*a, _op=op, _real=getattr(F, op), **k):
            calls[_op] += 1
            return _real(*a, **k)
        monkeypatch.setattr(F, op, counted)
    off = run_stage(make, gpu_device, F, False, False)
    dgrads = calls["linear_dgrad"]
    assert (calls["fwd_chain_stage"], calls["bwd_chain_stage"],
            calls["linear_fwd"]) == (0, 0, n)
    # either backward can follow either forward
    for fwd, bwd in ((True, True), (True, False), (False, True)):
        for op in calls:
            calls[op] = 0
        stash, h_top, dx, grads = run_stage(make, gpu_device, F, fwd, bwd)
        assert calls["fwd_chain_stage"] == fwd and calls["bwd_chain_stage"] \
            == bwd and calls["linear_fwd"] == (0 if fwd else n)
        # the 48-wide bottom layer's dgrad is the one that stays a launch
        assert calls["linear_dgrad"] == (name == "bottom_48" if bwd
                                         else dgrads)
        for la, lb in zip(stash, off[0]):
            assert la.keys() == lb.keys() == {("x", 0), ("y", 0)}
            assert all(same_bits(la[k], lb[k]) for k in la)
        assert same_bits(h_top, off[1])
        assert (dx is not None) == has_dx
        assert dx is None or same_bits(dx, off[2])
        assert all(torch.equal(a, b) for a, b in zip(grads, off[3]))


def test_model_stage_default_mode_within_reordering_bound(gpu_device, flags,
                                                          monkeypatch):
    """Grouped, non-deterministic wgrads after the stage launch: each
    element within M * 2^-23 * |dz|^T |x| of the deterministic run."""
    F = flags
    make = stage_models()["pp2_stage0"]
    seen = []
    real = F.linear_wgrad_acc

    def rec(dy, x, *a, **k):
        seen.append((dy.double().cpu(), x.double().cpu()))
        return real(dy, x, *a, **k)

    monkeypatch.setattr(F, "linear_wgrad_acc", rec)
    det = run_stage(make, gpu_device, F, True, True)[3]
    monkeypatch.setattr(F, "linear_wgrad_acc", real)
    got = run_stage(make, gpu_device, F, True, True, det=False)[3]
    assert len(seen) == 3
    for k, (dz, x) in enumerate(seen[::-1]):   # wgrads ran top first
        for g, r, bound in ((got[2 * k], det[2 * k], dz.abs().t() @ x.abs()),
                            (got[2 * k + 1], det[2 * k + 1], dz.abs().sum(0))):
            err = (g.double().cpu() - r.double().cpu()).abs()
            assert (err <= B * U_F32 * bound).all(), k


def test_model_stage_falls_back(gpu_device, flags, monkeypatch):
    """A GELU top layer, a 128-wide stage, dropout on the forward and the
    two switches reach neither stage op."""
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.models.layers import Linear, Sequential

    F = flags

    def boom(*a, **k):
        raise AssertionError("stage op reached")

    def fwd_bwd(model, in_dims, out_dims=H):
        model.materialize_device(gpu_device)
        model.zero_grad()
        x = randn(B, in_dims, seed=1).to(device=gpu_device, dtype=BF)
        model.forward(x, 0)
        model.backward(torch.ones(B, out_dims, device=gpu_device, dtype=BF), 0)

    flagship = [784] + [256] * 4 + [10]
    drop = MLP(flagship, 0, 2, B, dropout=0.25)
    monkeypatch.setattr(F, "fwd_chain_stage", boom)
    fwd_bwd(drop, 784)      # its backward may chain: one p for all layers
    monkeypatch.setattr(F, "bwd_chain_stage", boom)
    fwd_bwd(Sequential([Linear(H, H, "relu"), Linear(H, H, "gelu")]), H)
    fwd_bwd(MLP([784, 128, 128, 128, 128, 10], 0, 2, B), 784, 128)
    F.set_fwd_chain(False)
    F.set_bwd_chain(False)
    fwd_bwd(MLP(flagship, 0, 2, B), 784)
