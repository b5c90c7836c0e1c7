"""Forward chain kernel (csrc/fwd_chain.hip) against the extension ops
it replaces.

Every h_l and probs must be BIT-identical to gemm_nt(x, W, b, relu) per
layer followed by head_fwd_fused: the kernel runs the same MFMA with the
same operand slots and K-step order, zero-fills K past in_dims in both
operands as gemm_nt does, and runs the gemm_nt epilogue
(v = acc + bias; v = v > 0 ? v : 0; one rounding) and the head's
register epilogue.  The forward changes no bit, so with the chain on a
deterministic backward must not change a bit of any gradient; in default
mode the split-K partial sums meet in f32 atomics, so a gradient element
is held to the f32 reordering bound of its own sum,

    |g - g_det| <= M * 2^-23 * sum_r |dz[r,o]| * |x[r,i]|,

computed in f64 on the host from the deterministic run's dz and x (the
bound of tests/test_gpu_bwd_chain.py).

A refusal launches nothing and allocates nothing: the binding returns an
empty list before any output tensor exists, so there is no output a
refused call could have written.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()
H = 256
# (rows, waves); zeros = the shipped choice
ARMS = [(0, 0), (32, 4), (32, 8), (64, 4), (64, 8)]
FROM_TILE, STREAMED = 1, 2  # the launcher's l1 argument


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

    saved = (F._FWD_CHAIN, F._FWD_CHAIN_L1)
    yield F
    F._FWD_CHAIN, F._FWD_CHAIN_L1 = saved
    F.set_bwd_chain(True)
    F.set_head_fused(True)
    F.set_deterministic(False)


# ------------------------------------------------------------ kernel level

_CASES = {}


def chain_case(M, depth, C, K0, device):
    """Seeded inputs and the unfused chain's outputs, computed once per
    shape and shared (never modified) by the tests below.  Weights are
    N(0, 1)/sqrt(in), as Linear scales them.  The inputs pin the
    epilogue: column 7 of every layer has a bias that makes every
    pre-activation negative, and x holds an all-zero row, a -0.0, one
    NaN (its pre-activations are NaN, which v > 0 ? v : 0 sends to 0)
    and a row whose pre-activation in column 9 of the first layer is
    bf16_max + half an ulp in f32, which rounds to bf16 +inf."""
    key = (M, depth, C, K0)
    if key not in _CASES:
        e = ext()
        x = randn(M, K0, seed=100 + M + K0)
        x[0, 3] = -0.0
        if M > 1:
            x[M // 2, :] = 0.0
        if M > 2:
            x[M - 1, 5] = float("nan")
        ws = [randn(H, K0, seed=50) / K0 ** 0.5]
        ws += [randn(H, H, seed=50 + l) / H ** 0.5 for l in range(1, depth)]
        bs = [randn(H, seed=60 + l) * 0.1 for l in range(depth)]
        for b in bs:
            b[7] = -1e4
        if M > 3:
            # row 1: 2^127 * (2 - 2^-7) + 2^119 * 1 = bf16_max + ulp/2
            x[1, :] = 0.0
            x[1, 0], x[1, 1] = 2.0 ** 127, 2.0 ** 119
            ws[0][9, 0], ws[0][9, 1] = 2.0 - 2.0 ** -7, 1.0
            bs[0][9] = 0.0
        w_head = randn(C, H, seed=30 + C) / H ** 0.5
        b_head = randn(C, seed=31 + C) * 0.1
        x, w_head, b_head = (t.to(device=device, dtype=BF)
                             for t in (x, w_head, b_head))
        ws = [w.to(device=device, dtype=BF) for w in ws]
        bs = [b.to(device=device, dtype=BF) for b in bs]
        hs, h = [], x
        for w, b in zip(ws, bs):
            h = e.gemm_nt(h, w, b, EMPTY, True)
            hs.append(h)
        probs = e.head_fwd_fused(h, w_head, b_head)
        _CASES[key] = dict(x=x, ws=ws, bs=bs, w_head=w_head, b_head=b_head,
                           hs=hs, probs=probs)
    return _CASES[key]


def same_bits(a, b):
    """torch.equal on the bit patterns: the NaN and inf cases compare
    like any other value."""
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def check_chain(c, arm, l1):
    from shallowspeed_amd.ops import functional as F

    res = F.fwd_chain(c["x"], c["ws"], c["bs"], c["w_head"], c["b_head"],
                      *arm, l1=l1)
    assert res is not None, (arm, l1)
    hs, probs = res
    assert len(hs) == len(c["hs"])
    for l, (h, ref) in enumerate(zip(hs, c["hs"])):
        assert same_bits(h, ref), (arm, l1, l)
    assert same_bits(probs, c["probs"]), (arm, l1)


def test_case_holds_the_edge_values(gpu_device):
    """The reference itself shows what the inputs are meant to pin."""
    c = chain_case(97, 2, 10, H, gpu_device)
    h0 = c["hs"][0].float()
    assert (h0[:, 7] == 0).all()                    # negative column
    assert torch.isinf(h0[1, 9]) and h0[1, 9] > 0   # rounds to bf16 inf
    assert (h0[96] == 0).all()                      # NaN row: all to +0
    assert torch.isnan(c["x"].float()[96, 5])
    assert same_bits(c["hs"][0][96], torch.zeros_like(c["hs"][0][96]))


# M: 1 row; a partial 32-row tile; one 64-row tile (two 32-row tiles);
# 97 = multi-tile with a one-row last tile at both sizes; 200 = four
# 64-row tiles, the last partial
@pytest.mark.parametrize("C", [1, 10, 16])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 31, 64, 97, 200])
def test_chain_bit_identical(gpu_device, M, depth, C):
    """The chain starts from a stored 256-wide activation."""
    c = chain_case(M, depth, C, H, gpu_device)
    for arm in ARMS:
        check_chain(c, arm, 0)
        check_chain(c, arm, FROM_TILE)


# in_dims of the streamed first layer: 784 = 24 K-steps and a 16-element
# tail (and a partial last chunk); 256 = no tail; 40 = one K-step and an
# 8-element tail; 8 = less than one K-step
@pytest.mark.parametrize("K0", [784, 256, 40, 8])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 31, 64, 97, 200])
def test_chain_streamed_first_layer_bit_identical(gpu_device, M, depth, K0):
    for C in ((1, 10, 16) if M == 97 else (10,)):
        c = chain_case(M, depth, C, K0, gpu_device)
        for arm in ARMS:
            check_chain(c, arm, STREAMED)
            if K0 != H:
                check_chain(c, arm, 0)  # the only arm that fits


def test_chain_rejects_outside_contract(gpu_device):
    """Width != 256, C = 17, nine layers, a misaligned tensor, an
    unknown arm and a 784-wide input for the stored-activation arm
    launch nothing and return None / an empty list."""
    from shallowspeed_amd.ops import functional as F

    M = 64
    c = chain_case(M, 2, 10, H, gpu_device)
    x, ws, bs, wh, bh = c["x"], c["ws"], c["bs"], c["w_head"], c["b_head"]
    assert F.fwd_chain(x, ws, bs, wh, bh) is not None

    def zeros(*shape):
        return torch.zeros(*shape, device=gpu_device, dtype=BF)

    # width 128: the layer's output, the head's input, the inner input
    assert F.fwd_chain(x, [zeros(128, H)], [zeros(128)], zeros(10, 128),
                       bh) is None
    assert F.fwd_chain(x, ws, bs, zeros(10, 128), bh) is None
    assert F.fwd_chain(x, [ws[0], zeros(H, 128)], bs, wh, bh) is None
    assert ext().fwd_chain(x, [zeros(128, H)], [zeros(128)], zeros(10, 128),
                           bh) == []
    # C = 17
    assert F.fwd_chain(x, ws, bs, zeros(17, H), zeros(17)) is None
    # nine layers (eight pass)
    assert F.fwd_chain(x, [ws[1]] * 8, [bs[1]] * 8, wh, bh) is not None
    assert F.fwd_chain(x, [ws[1]] * 9, [bs[1]] * 9, wh, bh) is None
    # misaligned: contiguous, two bytes off a 16-byte boundary
    buf = zeros(M * H + 8)
    off = buf[1:1 + M * H].view(M, H)
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    assert F.fwd_chain(off, ws, bs, wh, bh) is None
    woff = zeros(H * H + 8)[1:1 + H * H].view(H, H)
    assert F.fwd_chain(x, [ws[0], woff], bs, wh, bh) is None
    # non-contiguous, wrong dtype, counts that differ
    assert F.fwd_chain(zeros(M, 2 * H)[:, ::2], ws, bs, wh, bh) is None
    assert F.fwd_chain(x.float(), ws, bs, wh, bh) is None
    assert F.fwd_chain(x, ws, bs[:1], wh, bh) is None
    assert F.fwd_chain(x, [], [], wh, bh) is None
    # unknown arms
    assert F.fwd_chain(x, ws, bs, wh, bh, 48, 4) is None
    assert F.fwd_chain(x, ws, bs, wh, bh, 64, 2) is None
    # in_dims: not a multiple of 8; 784 into the stored-activation arm
    assert F.fwd_chain(zeros(M, 36), [zeros(H, 36)], bs[:1], wh, bh) is None
    c784 = chain_case(M, 1, 10, 784, gpu_device)
    assert F.fwd_chain(c784["x"], c784["ws"], c784["bs"], wh, bh,
                       l1=FROM_TILE) is None


# ------------------------------------------------------------- model level

B = 200
SIZES = [784, 256, 256, 256, 10]


def _inputs(device):
    x = randn(B, SIZES[0], seed=71).to(device=device, dtype=BF)
    t = one_hot(B, SIZES[-1], seed=72).to(device=device, dtype=BF)
    return x, t


def _count_calls(F, monkeypatch):
    calls = {"chain": 0, "chain_ok": 0, "head_fwd": 0}
    chain, head = F.fwd_chain, F.head_fwd_fused

    def cc(*a, **k):
        calls["chain"] += 1
        res = chain(*a, **k)
        calls["chain_ok"] += res is not None
        return res

    def ch(*a, **k):
        calls["head_fwd"] += 1
        return head(*a, **k)

    monkeypatch.setattr(F, "fwd_chain", cc)
    monkeypatch.setattr(F, "head_fwd_fused", ch)
    return calls


def _fwd_bwd(device, F, fwd_chain, bwd_chain=True):
    """One forward + backward of a fresh flagship-shaped model: (stashes
    after the forward, probs, gradients)."""
    from shallowspeed_amd.models import MLP

    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(device)
    x, t = _inputs(device)
    model.zero_grad()
    F.set_fwd_chain(fwd_chain)
    probs = model.forward(x, 0)
    stash = [dict(l._cache) for l in model.layers]
    F.set_bwd_chain(bwd_chain)
    model.backward(t, 0)
    torch.cuda.synchronize()
    assert not any(l._cache for l in model.layers), "stash left behind"
    return stash, probs, [p.grad.clone() for p in model.parameters()]


def _same_stashes(a, b):
    assert len(a) == len(b)
    for la, lb in zip(a, b):
        assert la.keys() == lb.keys()
        for k in la:
            assert same_bits(la[k], lb[k]), k


@pytest.mark.parametrize("l1", [False, True])
def test_model_stashes_and_deterministic_grads_bitwise(gpu_device, flags,
                                                       monkeypatch, l1):
    from shallowspeed_amd.models import MLP

    F = flags
    F._FWD_CHAIN_L1 = l1
    F.set_fwd_chain(True)
    assert MLP(SIZES, 0, 1, B)._fwd_chain_plan() == \
        ([0, 1, 2] if l1 else [1, 2])
    F.set_deterministic(True)
    calls = _count_calls(F, monkeypatch)
    s_on, p_on, g_on = _fwd_bwd(gpu_device, F, True)
    assert (calls["chain_ok"], calls["head_fwd"]) == (1, 0)
    s_off, p_off, g_off = _fwd_bwd(gpu_device, F, False)
    assert (calls["chain"], calls["head_fwd"]) == (1, 1)
    assert [sorted(k for k, _ in s) for s in s_on] == \
        [["x", "y"], ["x", "y"], ["x", "y"], ["x"], ["s"]]
    _same_stashes(s_on, s_off)
    assert same_bits(p_on, p_off)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)


def test_model_default_mode_within_reordering_bound(gpu_device, flags,
                                                    monkeypatch):
    from shallowspeed_amd.models import MLP

    F = flags
    F.set_fwd_chain(True)
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


def test_model_mixed_chain_paths(gpu_device, flags):
    """Either backward can follow either forward: with one chain on and
    the other off the results equal the all-off path."""
    F = flags
    F.set_deterministic(True)
    s_off, p_off, g_off = _fwd_bwd(gpu_device, F, False, False)
    for fwd, bwd in ((True, False), (False, True), (True, True)):
        s, p, g = _fwd_bwd(gpu_device, F, fwd, bwd)
        _same_stashes(s, s_off)
        assert same_bits(p, p_off)
        for a, b in zip(g, g_off):
            assert torch.equal(a, b), (fwd, bwd)


def test_model_falls_back_outside_contract(gpu_device, flags, monkeypatch):
    """Width 128, GELU under the head, dropout and set_head_fused(False)
    never reach the chain and take the per-layer path."""
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.models.layers import (Linear, Sequential,
                                                SoftmaxXent)

    F = flags
    F.set_fwd_chain(True)
    calls = _count_calls(F, monkeypatch)
    x, _ = _inputs(gpu_device)

    narrow = MLP([784, 128, 128, 10], 0, 1, B).materialize_device(gpu_device)
    gelu = Sequential([Linear(784, H, "relu"), Linear(H, H, "gelu"),
                       Linear(H, 10), SoftmaxXent(B)])
    gelu.materialize_device(gpu_device)
    drop = MLP(SIZES, 0, 1, B, dropout=0.25).materialize_device(gpu_device)
    for n, model in enumerate((narrow, gelu, drop), 1):
        assert model._fwd_chain_plan() is None
        model.forward(x, 0)
        assert (calls["chain"], calls["head_fwd"]) == (0, n)
    F.set_head_fused(False)
    flagship = MLP(SIZES, 0, 1, B).materialize_device(gpu_device)
    assert flagship._fwd_chain_plan() is None
    flagship.forward(x, 0)
    assert (calls["chain"], calls["head_fwd"]) == (0, 3)
