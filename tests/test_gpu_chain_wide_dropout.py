"""Wide chain kernels under dropout (csrc/fwd_chain_wide_drop.hip and the
scaled form of csrc/bwd_chain_wide_kernel.h, H = 128 and 512): bit for bit
against the per-layer ops, against float64 with the CPU (numpy Philox)
mask, their refusals, and through the model.

Float64, forward: tests/test_gpu_chain_wide.py's bound with z and S
multiplied by scale_l; a dropped element is +0 exactly.  Backward: with t
= the kernel's own dz_{l+1} · W in f64, E = (K + 16)·2^-24·S and B1 = E +
2^-8 (|t| + E) (the tile's rounding), a kept element allows
|dz_l - s·t| <= s·B1 + (2^-8 + 2^-23)·s·(|t| + B1): the f32 multiply and
the second rounding.  No measured constant."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, STEP, LAYERS = 0x9E3779B97F4A7C15, 3, (2, 7, 11)
GB = 256
_BUILT = {}


def F_():
    from shallowspeed_amd.ops import functional as F

    return F


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def case(device, H, M, K0, depth, C, rows, ps):
    """Seeded inputs and the per-layer path's forward, built once per
    shape and shared, never modified."""
    key = (H, M, K0, depth, C, rows, ps)
    if key not in _BUILT:
        F = F_()
        dev = lambda t: t.to(device=device, dtype=BF)
        dims = [K0] + [H] * depth
        c = dict(x=dev(randn(M, K0, seed=M + K0)),
                 ws=[dev(randn(H, k, seed=50 + l) / k ** 0.5)
                     for l, k in enumerate(dims[:-1])],
                 bs=[dev(randn(H, seed=60 + l) * 0.1) for l in range(depth)],
                 w_head=dev(randn(C, H, seed=30) / H ** 0.5),
                 b_head=dev(randn(C, seed=31) * 0.1),
                 target=dev(torch.eye(C)[torch.arange(M) % C]), hs=[])
        h = c["x"]
        for w, b, layer, p in zip(c["ws"], c["bs"], LAYERS, ps):
            h = F.linear_fwd_dropout(h, w, b, SEED, STEP, layer, *rows, p) \
                if p else F.linear_fwd(h, w, b, relu=True)
            c["hs"].append(h)
        c["probs"] = F.head_fwd_fused(h, c["w_head"], c["b_head"])
        c["w_head_t"] = c["w_head"].t().contiguous()
        # top first; the first layer's dgrad is in the chain iff K0 == H
        c["w_ts"] = [w.t().contiguous()
                     for w in c["ws"][:0 if K0 != H else None:-1]]
        _BUILT[key] = c
    return _BUILT[key]


def fwd(c, ps, rows, arm=(0, 0), **k):
    a = [k.get(n, c[n]) for n in ("x", "ws", "bs", "w_head", "b_head")]
    return F_().fwd_chain_wide_dropout(*a, SEED, STEP, LAYERS[:len(a[1])],
                                       ps, *rows, *arm)


MIX, EVEN = (0.5, 0.0, 0.1), (0.25,) * 3
# H, arm, M, K0, depth, C, (row_first, row_stride), ps
FWD = [
    (128, (0, 0), 130, 40, 3, 10, (0, 1), EVEN),
    (128, (32, 4), 33, 8, 2, 16, (5, 3), MIX),
    (128, (64, 4), 65, 128, 3, 10, (5, 3), MIX),
    (128, (64, 4), 1, 136, 1, 1, (0, 1), EVEN),
    (128, (32, 4), 130, 136, 3, 10, (0, 1), MIX),
    (512, (0, 0), 65, 512, 2, 10, (5, 3), EVEN),
    (512, (32, 8), 33, 40, 3, 16, (0, 1), MIX),
    (512, (64, 8), 130, 136, 2, 10, (5, 3), EVEN),  # two mask registers
    (512, (64, 8), 65, 512, 3, 1, (0, 1), MIX),
    (512, (64, 16), 130, 8, 3, 10, (0, 1), MIX),
    (512, (64, 16), 1, 40, 1, 16, (5, 3), EVEN),
    (512, (32, 8), 130, 512, 2, 10, (5, 3), EVEN),
]


@pytest.mark.parametrize("H,arm,M,K0,depth,C,rows,ps", FWD)
def test_forward_bits(gpu_device, H, arm, M, K0, depth, C, rows, ps):
    c = case(gpu_device, H, M, K0, depth, C, rows, ps[:depth])
    hs, probs = fwd(c, ps[:depth], rows, arm)
    for l in range(depth):
        assert same_bits(hs[l], c["hs"][l]), l
    assert same_bits(probs, c["probs"])


@pytest.mark.parametrize("H", [128, 512])
def test_forward_against_float64(gpu_device, H):
    F, M, rows = F_(), 70, (5, 3)
    c = case(gpu_device, H, M, 136, 3, 10, rows, MIX)
    hs, _ = fwd(c, MIX, rows)
    ids = rows[0] + rows[1] * torch.arange(M)
    for l, p in enumerate(MIX):
        a = (c["x"] if l == 0 else hs[l - 1]).double().cpu()
        w, b = c["ws"][l].double().cpu(), c["bs"][l].double().cpu()
        keep = F.dropout_keep_mask(SEED, STEP, LAYERS[l], ids, H, p)
        s = F.dropout_params(p)[1]
        ref = torch.relu(a @ w.t() + b) * s
        E = (a.shape[1] + 16) * 2.0 ** -24 * s * (a.abs() @ w.abs().t()
                                                   + b.abs())
        y = hs[l].cpu()
        assert (y.view(torch.int16)[~keep] == 0).all(), l
        err, bound = (y.double() - ref).abs(), E + 2.0 ** -8 * (ref + E)
        print(l, err[keep].max().item(), bound[keep].max().item())
        assert (err <= bound)[keep].all(), l


def bwd_ref(c, s, loss):
    F = F_()
    dz_head, dh = F.head_bwd_fused(c["probs"], c["target"], c["hs"][-1],
                                   c["w_head_t"], GB, loss=loss)
    dzs = []
    for l, h in enumerate(c["hs"][::-1]):
        dzs.append(F.relu_bwd(dh, h, scale=s))
        dh = F.linear_fwd(dzs[-1], c["w_ts"][l]) if l < len(c["w_ts"]) \
            else None
    return dz_head, dzs, dh


# H, arm, M, K0 (H: the first layer's dgrad is in the chain), p, loss
BWD = [
    (128, (0, 0), 65, 128, 0.25, "xent"), (128, (32, 4), 130, 40, 0.5, "mse"),
    (128, (64, 4), 1, 128, 0.5, "xent"), (512, (0, 0), 130, 512, 0.5, "xent"),
    (512, (32, 8), 65, 40, 0.25, "mse"), (512, (64, 8), 130, 512, 0.25, "mse"),
    (512, (64, 16), 1, 40, 0.5, "xent"),
    (512, (64, 16), 65, 512, 0.25, "xent"),
]


@pytest.mark.parametrize("H,arm,M,K0,p,loss", BWD)
def test_backward_bits(gpu_device, H, arm, M, K0, p, loss):
    F = F_()
    c = case(gpu_device, H, M, K0, 2, 10, (0, 1), (p, p))
    args = (c["probs"], c["target"], c["w_head_t"], GB, c["hs"][::-1],
            c["w_ts"], *arm)
    s = F.dropout_params(p)[1]
    for got, ref in ((F.bwd_chain_wide(*args, loss=loss, dz_scale=s),
                      bwd_ref(c, s, loss)),
                     (F.bwd_chain_wide(*args, loss=loss, dz_scale=1.0),
                      F.bwd_chain_wide(*args, loss=loss))):
        assert same_bits(got[0], ref[0])
        assert all(same_bits(a, b) for a, b in zip(got[1], ref[1]))
        assert (got[2] is None) == (ref[2] is None) == (K0 != H)
        assert got[2] is None or same_bits(got[2], ref[2])


@pytest.mark.parametrize("H", [128, 512])
def test_backward_against_float64(gpu_device, H):
    F, p = F_(), 0.25
    c = case(gpu_device, H, 70, H, 2, 10, (0, 1), (p, p))
    s = F.dropout_params(p)[1]
    dz_head, dzs, _ = F.bwd_chain_wide(
        c["probs"], c["target"], c["w_head_t"], GB, c["hs"][::-1], c["w_ts"],
        dz_scale=s)
    up, w_up = dz_head, c["w_head"]
    for l, dz in enumerate(dzs):
        kept = c["hs"][1 - l] > 0
        t = (up.double() @ w_up.double()).abs()
        E = (H + 16) * 2.0 ** -24 * (up.double().abs() @ w_up.double().abs())
        B1 = E + 2.0 ** -8 * (t + E)
        bound = s * B1 + (2.0 ** -8 + 2.0 ** -23) * s * (t + B1)
        err = (dz.double() - s * (up.double() @ w_up.double())).abs()
        print(l, err[kept].max().item(), bound[kept].max().item())
        assert (dz.view(torch.int16)[~kept] == 0).all(), l
        assert (err <= bound)[kept].all(), l
        up, w_up = dz, c["ws"][1 - l]


@pytest.mark.parametrize("why", ["no p", "id 2^32", "H 256", "misaligned",
                                 "arm"])
def test_refusals_launch_nothing(gpu_device, why):
    H, M = 128, 70
    c = case(gpu_device, H, M, 40, 2, 10, (0, 1), (0.5, 0.5))
    z = lambda *s: torch.zeros(*s, device=gpu_device, dtype=BF)
    ps, rows, kw = (0.5, 0.5), (0, 1), {}
    if why == "no p":
        ps = (0.0, 0.0)
    elif why == "id 2^32":
        assert fwd(c, ps, (2 ** 32 - M, 1)) is not None  # last id 2^32 - 1
        rows = (2 ** 32 - M + 1, 1)
    elif why == "H 256":
        kw = dict(ws=[z(256, 40), z(256, 256)], bs=[z(256)] * 2,
                  w_head=z(10, 256))
    elif why == "misaligned":
        kw = dict(x=z(M * 40 + 8)[1:1 + M * 40].view(M, 40))
    else:
        kw = dict(arm=(64, 8))
    assert fwd(c, ps, rows, **kw) is None


@pytest.mark.parametrize("sizes", [[40, 128, 128, 10], [784, 512, 512, 10]])
def test_model_switch_on_equals_off(gpu_device, sizes, monkeypatch):
    from shallowspeed_amd.models import MLP

    F, B = F_(), 96
    x = randn(B, sizes[0], seed=7).to(gpu_device, BF)
    t = torch.eye(10)[torch.arange(B) % 10].to(gpu_device, BF)
    calls = []
    for name in ("fwd_chain_wide_dropout", "fwd_chain_wide", "bwd_chain_wide"):
        real = getattr(F, name)
        monkeypatch.setattr(F, name, lambda *a, _r=real, _n=name, **k: (
            calls.append(_n), _r(*a, **k))[1])
    for flag in ("_CHAIN_WIDE", "_CHAIN_WIDE_DROPOUT", "_DETERMINISTIC",
                 "_DET_WGRAD"):
        monkeypatch.setattr(F, flag, getattr(F, flag))  # restored after
    F.set_chain_wide(True)
    F.set_deterministic(True)
    out = {}
    for on in (True, False):
        F.set_chain_wide_dropout(on)
        model = MLP(sizes, 0, 1, B, dropout=0.25,
                    dropout_seed=SEED).materialize_device(gpu_device)
        model.zero_grad()
        probs = model.forward(x, 0)
        model.backward(t, 0)
        torch.cuda.synchronize()
        assert not any(l._cache for l in model.layers), "stash left behind"
        out[on] = [probs] + [p.grad.clone() for p in model.parameters()]
        if on:
            assert calls == ["fwd_chain_wide_dropout", "bwd_chain_wide"]
            model.eval()
            model.forward(x, 0)
            assert calls[2:] == ["fwd_chain_wide"]
    assert len(calls) == 3
    assert same_bits(out[True][0], out[False][0])
    assert all(torch.equal(a, b) for a, b in zip(out[True][1:], out[False][1:]))
