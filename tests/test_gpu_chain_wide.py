"""Wide chain kernels (csrc/fwd_chain_wide.hip, csrc/bwd_chain_wide.hip,
H = 128 and 512): against float64 layer by layer, bit for bit against
the per-layer extension ops, their refusals, and the model that plans
them.

The float64 bound has no measured constant.  With a the kernel's own
bf16 input of a layer, z = a·w^T + b and S = |a|·|w|^T + |b| in f64 and
E = (K + 16)·2^-24·S (an f32 sum of K products in any order), one bf16
rounding allows |h - relu(z)| <= E + 2^-8·(relu(z) + E).  The same with
K = H and no bias holds dh at the kept positions of every dz_l (and
dx); a masked position, !(h_l > 0), must be +0 exactly."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()
GB = 256  # global batch of the head backward

# (H, M, in_dims, n, C, edge): M = 1 row, a partial tile, one row past a
# 64-row tile, several tiles at both R; in_dims = one partial chunk, not a
# multiple of the chunk, the width itself, many chunks.  edge: the inputs
# carry a -0.0, an all-zero row, a NaN row and a column whose bias makes
# every pre-activation negative (bit identity only: they are not finite).
CASES = [
    (128, 1, 8, 1, 1, False), (128, 63, 40, 3, 10, False),
    (128, 65, 128, 8, 16, False), (128, 130, 784, 3, 10, False),
    (512, 1, 784, 1, 16, False), (512, 63, 512, 3, 10, False),
    (512, 65, 40, 8, 1, False), (512, 130, 8, 3, 10, False),
    (128, 130, 40, 2, 10, True), (512, 130, 512, 2, 10, True),
]
FINITE = [c for c in CASES if not c[5]]
_BUILT = {}


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def case(key, device):
    """Seeded inputs (N(0,1) x, N(0,1)/sqrt(in) weights, 0.1-scale
    biases) and the per-layer path's outputs, computed once per case and
    shared, never modified."""
    if key in _BUILT:
        return _BUILT[key]
    H, M, K0, n, C, edge = key
    e = ext()
    g = torch.Generator().manual_seed(sum(key))
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(M, K0)
    dims = [K0] + [H] * n
    ws = [rnd(H, dims[l]) / dims[l] ** 0.5 for l in range(n)]
    bs = [rnd(H) * 0.1 for _ in range(n)]
    if edge:
        x[0, 3] = -0.0
        x[M // 2] = 0.0
        x[M - 1, 5] = float("nan")
        for b in bs:
            b[7] = -1e4
    w_head, b_head = rnd(C, H) / H ** 0.5, rnd(C) * 0.1
    target = torch.zeros(M, C)
    target[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
    dev = lambda t: t.to(device=device, dtype=BF)
    x, w_head, b_head, target = map(dev, (x, w_head, b_head, target))
    ws, bs = [dev(w) for w in ws], [dev(b) for b in bs]
    hs, h = [], x
    for w, b in zip(ws, bs):
        h = e.gemm_nt(h, w, b, EMPTY, True)
        hs.append(h)
    probs = e.head_fwd_fused(h, w_head, b_head)
    w_head_t = w_head.t().contiguous()
    # top first; the first layer's dgrad is in the chain iff K0 == H
    w_ts = [ws[l].t().contiguous() for l in range(n - 1, 0 if K0 != H else -1,
                                                  -1)]
    dz_head, dh = e.head_bwd_fused(probs, target, h, w_head_t, float(GB),
                                   EMPTY, EMPTY)
    dzs = []
    for l in range(n):
        dzs.append(e.relu_bwd(dh, hs[n - 1 - l]))
        dh = e.gemm_nt(dzs[-1], w_ts[l], EMPTY, EMPTY, False) \
            if l < len(w_ts) else None
    _BUILT[key] = dict(x=x, ws=ws, bs=bs, w_head=w_head, b_head=b_head,
                       w_head_t=w_head_t, target=target, w_ts=w_ts, hs=hs,
                       probs=probs, dz_head=dz_head, dzs=dzs, dx=dh)
    return _BUILT[key]


def run(c, arm):
    from shallowspeed_amd.ops import functional as F

    fwd = F.fwd_chain_wide(c["x"], c["ws"], c["bs"], c["w_head"], c["b_head"],
                           *arm)
    assert fwd is not None, arm
    bwd = F.bwd_chain_wide(c["probs"], c["target"], c["w_head_t"], GB,
                           c["hs"][::-1], c["w_ts"], *arm)
    assert bwd is not None, arm
    return fwd, bwd


def arms(H):
    from shallowspeed_amd.ops import functional as F

    return [(0, 0)] + list(F.CHAIN_WIDE_ARMS[H])


def within(got, z, S, K, relu):
    """The module docstring's bound, every element."""
    E = (K + 16) * 2.0 ** -24 * S
    ref = z.clamp(min=0) if relu else z
    err = (got.double() - ref).abs()
    bound = E + 2.0 ** -8 * (ref.abs() + E)
    print(f"max err {err.max().item():.3e} max bound {bound.max().item():.3e}")
    return bool((err <= bound).all())


@pytest.mark.parametrize("key", FINITE, ids=str)
def test_against_float64(gpu_device, key):
    H, M, K0, n, C, _ = key
    c = case(key, gpu_device)
    for arm in arms(H):
        (hs, _), (_, dzs, dx) = run(c, arm)
        a = c["x"]
        for l, h in enumerate(hs):
            ad, wd = a.double(), c["ws"][l].double()
            bd = c["bs"][l].double()
            assert within(h, ad @ wd.t() + bd,
                          ad.abs() @ wd.abs().t() + bd.abs(), a.shape[1],
                          True), (arm, l)
            a = h
        # dh of layer l from the kernel's own dz of the layer above; the
        # top layer's from dz_head (K = C <= H products)
        up, w_up = c["dz_head"], c["w_head"]
        for l, dz in enumerate(dzs):
            kept = c["hs"][n - 1 - l] > 0
            z = up.double() @ w_up.double()
            S = up.double().abs() @ w_up.double().abs()
            assert same_bits(dz[~kept], torch.zeros_like(dz[~kept])), (arm, l)
            assert within(dz[kept], z[kept], S[kept], H, False), (arm, l)
            up, w_up = dz, c["ws"][n - 1 - l]
        assert (dx is not None) == (K0 == H)
        if dx is not None:
            assert within(dx, up.double() @ w_up.double(),
                          up.double().abs() @ w_up.double().abs(), H, False)


@pytest.mark.parametrize("key", CASES, ids=str)
def test_bit_identical_to_per_layer_ops(gpu_device, key):
    c = case(key, gpu_device)
    if key[5]:  # the reference shows what the edge inputs pin
        h0 = c["hs"][0]
        assert (h0[:, 7] == 0).all() and torch.isnan(c["x"][-1, 5])
        assert same_bits(h0[-1], torch.zeros_like(h0[-1]))
    for arm in arms(key[0]):
        (hs, probs), (dz_head, dzs, dx) = run(c, arm)
        assert len(hs) == len(c["hs"]) and len(dzs) == len(c["dzs"])
        for l, (got, ref) in enumerate(zip(hs + dzs, c["hs"] + c["dzs"])):
            assert same_bits(got, ref), (arm, l)
        assert same_bits(probs, c["probs"]), arm
        assert same_bits(dz_head, c["dz_head"]), arm
        assert (dx is None) == (c["dx"] is None)
        assert dx is None or same_bits(dx, c["dx"]), arm


def test_refusals(gpu_device):
    """Each launches nothing and allocates nothing: None from the op, an
    empty list from the binding."""
    from shallowspeed_amd.ops import functional as F

    H, M, K0, n, C, _ = key = CASES[1]
    c = case(key, gpu_device)
    z = lambda *s: torch.zeros(*s, device=gpu_device, dtype=BF)
    off = lambda t: z(t.numel() + 8)[1:1 + t.numel()].view(t.shape)
    fwd = lambda **k: F.fwd_chain_wide(*[k.get(a, c[a]) for a in (
        "x", "ws", "bs", "w_head", "b_head")], k.get("rows", 0),
        k.get("waves", 0))
    bwd = lambda **k: F.bwd_chain_wide(
        k.get("probs", c["probs"]), k.get("target", c["target"]),
        k.get("w_head_t", c["w_head_t"]), GB, k.get("hs", c["hs"][::-1]),
        k.get("w_ts", c["w_ts"]), k.get("rows", 0), k.get("waves", 0))
    assert fwd() is not None and bwd() is not None
    w9, h9 = [c["ws"][1]] * 9, [c["hs"][1]] * 9
    for bad in (
            dict(w_head=z(C, 256), ws=[z(256, K0)], bs=[z(256)]),  # other H
            dict(w_head=z(17, H), b_head=z(17)),                   # C > 16
            dict(x=z(M, H), ws=w9, bs=[c["bs"][1]] * 9),           # n > 8
            dict(x=z(M, 36), ws=[z(H, 36)], bs=c["bs"][:1]),       # in % 8
            dict(x=c["x"].float()), dict(x=z(M, 2 * K0)[:, ::2]),
            dict(x=off(c["x"])), dict(ws=[c["ws"][0], off(c["ws"][1]),
                                          c["ws"][2]]),
            dict(x=c["x"].cpu()),
            dict(rows=64, waves=8), dict(rows=32), dict(waves=4)):
        assert fwd(**bad) is None, list(bad)
    for bad in (
            dict(w_head_t=z(256, C), hs=[z(M, 256)], w_ts=[]),
            dict(probs=z(M, 17), target=z(M, 17), w_head_t=z(H, 17)),
            dict(hs=h9, w_ts=[c["w_ts"][0]] * 8),
            dict(probs=c["probs"].float()), dict(probs=off(c["probs"])),
            dict(hs=[off(c["hs"][2])] + c["hs"][1::-1]),
            dict(w_ts=[z(H, 2 * H)[:, ::2], c["w_ts"][1]]),
            dict(probs=c["probs"].cpu()), dict(w_ts=[]),
            dict(rows=64, waves=8), dict(waves=4)):
        assert bwd(**bad) is None, list(bad)
    assert ext().fwd_chain_wide(c["x"], c["ws"], c["bs"], c["w_head"],
                                c["b_head"], 64, 8) == []
    assert ext().bwd_chain_wide(c["probs"], c["target"], c["w_head_t"], GB,
                                c["hs"][::-1], c["w_ts"], 64, 8) == []


@pytest.mark.parametrize("sizes", [[40, 128, 128, 10], [784, 512, 512, 10]])
def test_model_takes_the_wide_chains_and_keeps_its_bits(gpu_device, sizes,
                                                        monkeypatch):
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.ops import functional as F

    B = 96
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, sizes[0], generator=g).to(gpu_device, BF)
    t = torch.zeros(B, 10)
    t[torch.arange(B), torch.randint(0, 10, (B,), generator=g)] = 1
    t = t.to(gpu_device, BF)
    calls = []
    for name in ("fwd_chain_wide", "bwd_chain_wide"):
        real = getattr(F, name)
        monkeypatch.setattr(F, name, lambda *a, _r=real, _n=name, **k: (
            calls.append(_n), _r(*a, **k))[1])
    for flag in ("_CHAIN_WIDE", "_DETERMINISTIC", "_DET_WGRAD"):
        monkeypatch.setattr(F, flag, getattr(F, flag))  # restored after
    F.set_deterministic(True)
    out = {}
    for on in (True, False):
        F.set_chain_wide(on)
        model = MLP(sizes, 0, 1, B, loss="xent").materialize_device(gpu_device)
        assert (model._fwd_wide_plan() is not None) == on
        assert (model._bwd_wide_plan(B) is not None) == on
        model.zero_grad()
        probs = model.forward(x, 0)
        model.backward(t, 0)
        torch.cuda.synchronize()
        assert not any(l._cache for l in model.layers), "stash left behind"
        out[on] = (probs, [p.grad.clone() for p in model.parameters()])
    assert calls == ["fwd_chain_wide", "bwd_chain_wide"]
    assert same_bits(out[True][0], out[False][0])
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.equal(a, b)
