"""Forward chain under dropout (csrc/fwd_chain_drop.hip, its stage arm
csrc/fwd_chain_stage_drop.hip) against the ops it replaces, against
float64 with the CPU (numpy Philox) mask, and through the model.

Bits: every h_l and probs must equal linear_fwd_dropout(fused) per layer
(linear_fwd(relu) where p = 0) followed by head_fwd_fused.  Float64: a
dropped element is +0 exactly; a kept one carries one bf16 rounding
(2^-8 relative) of an f32 accumulation over K terms, scaled:

    |y - ref| <= 2^-8 |ref| + K 2^-23 scale (|x| |W|^T + |b|).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H = 256
SEED = 0x9E3779B97F4A7C15  # non-zero high word
STEP = 3
LAYERS = (2, 7, 11)        # distinct, non-consecutive counter words
FLAGSHIP = [784, 256, 256, 256, 10]
PP2 = [784, 256, 256, 256, 256, 10]  # the flagship, padded for two stages


def F_():
    from shallowspeed_amd.ops import functional as F

    return F


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def inputs(M, K0, depth, C, device):
    dims = [K0] + [H] * depth
    ws = [randn(H, k, seed=50 + l) / k ** 0.5 for l, k in enumerate(dims[:-1])]
    bs = [randn(H, seed=60 + l) * 0.1 for l in range(depth)]
    ts = [randn(M, K0, seed=M + K0), randn(C, H, seed=30) / 16,
          randn(C, seed=31) * 0.1]
    return [t.to(device=device, dtype=BF) if torch.is_tensor(t) else
            [u.to(device=device, dtype=BF) for u in t]
            for t in (ts[0], ws, bs, ts[1], ts[2])]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def probs_of(mixed, depth):
    return ((0.5, 0.0, 0.1) if mixed else (0.25,) * 3)[:depth]


# arm, M, (K0, depth), C, (row_first, row_stride), mixed ps
CASES = [
    ((0, 0), 70, (256, 3), 10, (0, 1), False),
    ((32, 4), 33, (48, 2), 16, (5, 3), True),
    ((32, 8), 1, (136, 3), 10, (5, 3), True),
    ((64, 4), 70, (136, 3), 16, (0, 1), True),
    ((64, 8), 70, (256, 1), 10, (5, 3), False),
    ((64, 8), 33, (48, 2), 10, (0, 1), False),
    ((32, 8), 70, (256, 3), 16, (0, 1), True),
    ((64, 4), 1, (256, 3), 10, (5, 3), False),
    ((32, 4), 70, (136, 3), 10, (0, 1), False),
    ((0, 0), 33, (256, 1), 16, (5, 3), True),
]


@pytest.mark.parametrize("arm,M,shape,C,rows,mixed", CASES)
def test_bits_of_the_unfused_chain(gpu_device, arm, M, shape, C, rows, mixed):
    F = F_()
    (K0, depth), ps = shape, probs_of(mixed, shape[1])
    x, ws, bs, w_head, b_head = inputs(M, K0, depth, C, gpu_device)
    ref, h = [], x
    for w, b, layer, p in zip(ws, bs, LAYERS, ps):
        h = F.linear_fwd_dropout(h, w, b, SEED, STEP, layer, *rows, p) if p \
            else F.linear_fwd(h, w, b, relu=True)
        ref.append(h)
    key = (SEED, STEP, LAYERS[:depth], ps, *rows)
    hs, probs = F.fwd_chain_dropout(x, ws, bs, w_head, b_head, *key, *arm)
    stage = F.fwd_chain_stage_dropout(x, ws, bs, *key, *arm)
    for l in range(depth):
        assert same_bits(hs[l], ref[l]), l
        assert same_bits(stage[l], ref[l]), l
    assert same_bits(probs, F.head_fwd_fused(h, w_head, b_head))


@pytest.mark.parametrize("K0,depth", [(256, 1), (256, 3), (48, 2), (136, 3)])
def test_against_float64(gpu_device, K0, depth):
    F = F_()
    M, rows, ps = 70, (5, 3), probs_of(True, depth)
    x, ws, bs, w_head, b_head = inputs(M, K0, depth, 10, gpu_device)
    hs, _ = F.fwd_chain_dropout(x, ws, bs, w_head, b_head, SEED, STEP,
                                LAYERS[:depth], ps, *rows)
    ids = rows[0] + rows[1] * torch.arange(M)
    for l, (w, b, p) in enumerate(zip(ws, bs, ps)):
        a = (x if l == 0 else hs[l - 1]).double().cpu()
        w, b, y = w.double().cpu(), b.double().cpu(), hs[l].cpu()
        keep = F.dropout_keep_mask(SEED, STEP, LAYERS[l], ids, H, p)
        scale = F.dropout_params(p)[1]
        ref = torch.where(keep, torch.relu(a @ w.t() + b) * scale, 0.0)
        bound = 2.0 ** -8 * ref.abs() + w.shape[1] * 2.0 ** -23 * scale * (
            a.abs() @ w.abs().t() + b.abs())
        zeros = (y == 0).double().mean().item()
        assert (y.view(torch.int16)[~keep] == 0).all(), (l, zeros)
        assert ((y.double() - ref).abs() <= bound)[keep].all(), (l, zeros)


def test_refusals_launch_and_zero_nothing(gpu_device):
    F = F_()
    M = 70
    x, ws, bs, w_head, b_head = inputs(M, H, 2, 10, gpu_device)
    zero = torch.full((1000,), 7.0, device=gpu_device)
    off = torch.zeros(M * H + 1, device=gpu_device, dtype=BF)[1:].view(M, H)
    narrow = [w[:128].contiguous() for w in ws]
    key = (SEED, STEP, LAYERS[:2])
    for args, drop in [
            ((x, ws, bs), (*key, (0.0, 0.0), 0, 1)),           # all p = 0
            ((x, ws, bs), (*key, (0.5, 0.5), 2 ** 32 - M + 1, 1)),  # id 2^32
            ((x, narrow, bs), (*key, (0.5, 0.5), 0, 1)),        # H != 256
            ((off, ws, bs), (*key, (0.5, 0.5), 0, 1))]:         # misaligned
        assert F.fwd_chain_dropout(*args, w_head, b_head, *drop,
                                   zero=zero) is None
        assert F.fwd_chain_stage_dropout(*args, *drop) is None
    assert (zero == 7.0).all()
    ok = F.fwd_chain_dropout(x, ws, bs, w_head, b_head, *key, (0.5, 0.5),
                             2 ** 32 - M, 1, zero=zero)  # last id 2^32 - 1
    assert ok is not None and (zero == 0.0).all()


# ------------------------------------------------------------------ model

B = 70


@pytest.fixture
def flags():
    F = F_()
    F.set_deterministic(True)
    yield F
    F.set_fwd_chain_dropout(False)
    F.set_deterministic(False)


def run_model(F, monkeypatch, device, on, n_stages, train=True):
    """Two steps of the model's stage 0; returns what they left (stashes
    of the last forward, outputs, gradients) and the forward's launches."""
    from shallowspeed_amd.models import MLP

    F.set_fwd_chain_dropout(on)
    model = MLP(FLAGSHIP if n_stages == 1 else PP2, 0, n_stages, B,
                dropout=0.25,
                dropout_seed=SEED).materialize_device(device)
    if not train:
        model.eval()
    calls, kept = [], []
    for name in ("fwd_chain_dropout", "fwd_chain_stage_dropout", "fwd_chain",
                 "fwd_chain_stage", "head_fwd_fused", "linear_fwd_dropout"):
        real = getattr(F, name)
        monkeypatch.setattr(F, name, lambda *a, _n=name, _r=real, **k:
                            (calls.append(_n), _r(*a, **k))[1])
    x = randn(B, 784, seed=1).to(device=device, dtype=BF)
    out_dims = 10 if n_stages == 1 else H
    t = torch.eye(out_dims)[torch.arange(B) % out_dims].to(device=device,
                                                           dtype=BF)
    for _ in range(2):
        model.zero_grad()
        kept.append(model.forward(x, 0).clone())
        kept += [v.clone() for l in model.layers
                 for _, v in sorted(l._cache.items())]
        if train:
            model.backward(t, 0)
            kept += [p.grad.clone() for p in model.parameters()]
        model.dropout_step += 1
    monkeypatch.undo()
    return kept, calls


@pytest.mark.parametrize("n_stages,launch,old", [
    (1, "fwd_chain_dropout", ["linear_fwd_dropout"] * 3 + ["head_fwd_fused"]),
    (2, "fwd_chain_stage_dropout", ["linear_fwd_dropout"] * 3)])
def test_model_switch_on_equals_off(gpu_device, flags, monkeypatch, n_stages,
                                    launch, old):
    on, calls_on = run_model(flags, monkeypatch, gpu_device, True, n_stages)
    off, calls_off = run_model(flags, monkeypatch, gpu_device, False, n_stages)
    assert calls_on == [launch] * 2 and calls_off == old * 2
    assert len(on) == len(off) and len(on) > 8
    assert all(same_bits(a, b) if a.dtype == BF else torch.equal(a, b)
               for a, b in zip(on, off))


def test_model_eval_takes_the_plain_chain(gpu_device, flags, monkeypatch):
    on, calls_on = run_model(flags, monkeypatch, gpu_device, True, 1, False)
    off, calls_off = run_model(flags, monkeypatch, gpu_device, False, 1, False)
    assert calls_on == ["fwd_chain"] * 2
    assert calls_off == ["head_fwd_fused"] * 2
    assert len(on) == 2 and all(same_bits(a, b) for a, b in zip(on, off))
