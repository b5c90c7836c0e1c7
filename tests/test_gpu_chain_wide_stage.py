"""Stage arms of the wide chain kernels (csrc/fwd_chain_wide_stage.hip,
fwd_chain_wide_stage_drop.hip, bwd_chain_wide_stage.hip; H = 128 and 512,
a pipeline stage with no head): bit for bit against the per-layer ops,
against float64 with tests/test_gpu_chain_wide.py's bound, their refusals,
and the model that plans them.

Backward bound: with t = dz_{l-1} · W in f64 (t = dout, exact, for dz_0),
E = (H + 16)·2^-24·|dz_{l-1}|·|W| and B1 = E + 2^-8·(|t| + E), a kept
element allows B1, and under dz_scale s, tests/test_gpu_stage_chain.py's
scale terms: s·B1 + (2^-8 + 2^-23)·s·(|t| + B1).  A masked one is +0."""

import pytest
import torch

from shallowspeed_amd.ops import functional as F
from test_gpu_chain_wide import BF, EMPTY, arms, case, ext, same_bits, within

pytestmark = pytest.mark.gpu

SCALE = 1 / 0.75
SEED, STEP, LAYERS = 0x9E3779B97F4A7C15, 3, (2, 7, 11)
# (H, M, K0, n): one row, a partial tile, one row past a 64-row tile; a
# partial x chunk, many chunks, K0 == H (both starts)
FWD = [(128, 1, 8, 1), (128, 63, 128, 3), (128, 130, 784, 8),
       (512, 1, 784, 1), (512, 65, 512, 2), (512, 130, 40, 3)]
EDGE = [(128, 130, 40, 2), (512, 130, 512, 2)]
_BWD = {}


starts = lambda H, K0: (0, 1, 2) if K0 == H else (0, 1)  # noqa: E731


@pytest.mark.parametrize("H,M,K0,n", FWD + EDGE)
def test_forward_bits_and_float64(gpu_device, H, M, K0, n):
    edge = (H, M, K0, n) in EDGE
    c = case((H, M, K0, n, 10, edge), gpu_device)
    for arm in arms(H):
        for start in starts(H, K0):
            hs = F.fwd_chain_wide_stage(c["x"], c["ws"], c["bs"], *arm,
                                           start)
            assert hs is not None and len(hs) == n, (arm, start)
            a = c["x"]
            for l, h in enumerate(hs):
                assert same_bits(h, c["hs"][l]), (arm, start, l)
                if not edge:
                    ad, wd = a.double(), c["ws"][l].double()
                    bd = c["bs"][l].double()
                    assert within(h, ad @ wd.t() + bd, ad.abs() @ wd.abs().t()
                                  + bd.abs(), a.shape[1], True), (arm, l)
                a = h


def bwd_case(device, H, M, depth, last_in, scale, edge):
    """dout, hs (top first), w_ts and the per-layer path's dz / dx, built
    once and shared.  edge: a -0.0 and a NaN in hs, an inf in dout at a
    kept and at a masked position."""
    key = (H, M, depth, last_in, scale, edge)
    if key not in _BWD:
        c = case((H, M, H, 3, 10, False), device)
        hs = [h.clone() for h in c["hs"][:depth][::-1]]
        g = torch.Generator().manual_seed(H + M)
        dout = (torch.randn(M, H, generator=g) / 64).to(device, BF)
        if edge:
            kept = (hs[0] > 0).nonzero()
            dout[tuple(kept[0])] = float("inf")
            hs[0][tuple(kept[-1])] = 0.0
            dout[tuple(kept[-1])] = float("inf")
            hs[0][0, 3], hs[-1][M - 1, 5] = -0.0, float("nan")
        w_ts = [c["ws"][l].t().contiguous()
                for l in range(depth - 1, -1 if last_in else 0, -1)]
        dzs, dh = [], dout
        for l in range(depth):
            dzs.append(F.relu_bwd(dh, hs[l], scale=scale))
            dh = ext().gemm_nt(dzs[-1], w_ts[l], EMPTY, EMPTY, False) \
                if l < len(w_ts) else None
        _BWD[key] = dict(dout=dout, hs=hs, w_ts=w_ts, dzs=dzs, dx=dh,
                         ws=c["ws"][:depth][::-1])
    return _BWD[key]


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("scale", [1.0, SCALE])
@pytest.mark.parametrize("last_in", [True, False])
@pytest.mark.parametrize("H,M,depth", [(h, m, 1 + k % 3) for k, (h, m, _, _)
                                       in enumerate(FWD)])
def test_backward_bits_and_float64(gpu_device, H, M, depth, last_in, scale,
                                   edge):
    c = bwd_case(gpu_device, H, M, depth, last_in, scale, edge)
    for arm in arms(H):
        res = F.bwd_chain_wide_stage(c["dout"], c["hs"], c["w_ts"], *arm,
                                        dz_scale=scale)
        assert res is not None, arm
        dzs, dx = res
        assert (dx is not None) == last_in and len(dzs) == depth
        for l, (got, ref) in enumerate(zip(dzs + [dx], c["dzs"] + [c["dx"]])):
            assert got is ref is None or same_bits(got, ref), (arm, l)
        if edge:
            continue
        up = None
        for l, dz in enumerate(dzs + ([dx] if last_in else [])):
            s = scale if l < depth else 1.0
            kept = c["hs"][l] > 0 if l < depth else torch.ones_like(dz) > 0
            if up is None:
                t, B1 = c["dout"].double(), 0.0
            else:
                t = up.double() @ c["ws"][l - 1].double()
                E = (H + 16) * 2.0 ** -24 * (
                    up.double().abs() @ c["ws"][l - 1].double().abs())
                B1 = E + 2.0 ** -8 * (t.abs() + E)
            bound = B1 if s == 1.0 else \
                s * B1 + (2.0 ** -8 + 2.0 ** -23) * s * (t.abs() + B1)
            err = (dz.double() - s * t).abs()
            print(l, err[kept].max().item(), (bound + 0 * t)[kept].max().item())
            assert (dz.view(torch.int16)[~kept] == 0).all(), (arm, l)
            assert (err <= bound)[kept].all(), (arm, l)
            up = dz


@pytest.mark.parametrize("H,M,ps", [(128, 130, (0.25,) * 3),
                                    (512, 65, (0.25,) * 3),
                                    (128, 70, (0.25, 0.0, 0.25))])
def test_dropout_forward_bits(gpu_device, H, M, ps):
    rows = (5, 3)
    c = case((H, M, H, 3, 10, False), gpu_device)
    ref, h = [], c["x"]
    for w, b, layer, p in zip(c["ws"], c["bs"], LAYERS, ps):
        h = F.linear_fwd_dropout(h, w, b, SEED, STEP, layer, *rows, p) if p \
            else F.linear_fwd(h, w, b, relu=True)
        ref.append(h)
    for arm in arms(H):
        for start in starts(H, H):
            hs = F.fwd_chain_wide_stage_dropout(
                c["x"], c["ws"], c["bs"], SEED, STEP, LAYERS, ps, *rows, *arm,
                start)
            assert hs is not None, (arm, start)
            assert all(same_bits(a, b) for a, b in zip(hs, ref)), (arm, start)


@pytest.mark.parametrize("why", ["H 256", "nine layers", "K0 12", "misaligned",
                                 "start 2", "wt / dx"])
def test_refusals_launch_and_allocate_nothing(gpu_device, why):
    """The ops allocate their outputs, so a refusal shows as None from the
    op, [] from the binding and no byte allocated in between."""
    H, M = 128, 63
    c = case((H, M, H, 3, 10, False), gpu_device)
    z = lambda *s: torch.zeros(*s, device=gpu_device, dtype=BF)
    off = lambda t: z(t.numel() + 8)[1:1 + t.numel()].view(t.shape)
    x, ws, bs, start = c["x"], c["ws"], c["bs"], 0
    dout, hs = c["hs"][2], c["hs"][::-1]
    w_ts = [w.t().contiguous() for w in c["ws"][::-1]]
    assert F.fwd_chain_wide_stage(x, ws, bs) is not None
    assert F.bwd_chain_wide_stage(dout, hs, w_ts) is not None
    if why == "H 256":
        x, ws, bs = z(M, 256), [z(256, 256)], [z(256)]
        dout, hs, w_ts = x, [x], [ws[0]]
    elif why == "nine layers":
        ws, bs, hs, w_ts = [ws[1]] * 9, [bs[1]] * 9, [hs[0]] * 9, [w_ts[0]] * 9
    elif why == "K0 12":
        x, ws = z(M, 12), [z(H, 12)] + ws[1:]
        dout = z(M, 2 * H)[:, ::2]  # and a strided gradient
    elif why == "misaligned":
        x, dout = off(x), off(dout)
    elif why == "start 2":
        x, ws, start = z(M, 40), [z(H, 40)] + ws[1:], 2
        hs = [off(hs[0])] + hs[1:]
    else:  # neither all of the dgrads nor all but the last
        x, w_ts = x.float(), w_ts[:1]
    before = torch.cuda.memory_allocated()
    assert F.fwd_chain_wide_stage(x, ws, bs, 0, 0, start) is None
    assert F.bwd_chain_wide_stage(dout, hs, w_ts) is None
    assert ext().fwd_chain_wide_stage(x, ws, bs, 0, 0, start) == []
    assert ext().bwd_chain_wide_stage(dout, hs, w_ts, 0, 0, 1.0) == []
    assert F.fwd_chain_wide_stage(c["x"], c["ws"], c["bs"], 64, 8) is None
    assert torch.cuda.memory_allocated() == before


B = 200
OPS = ("fwd_chain_wide_stage", "fwd_chain_wide_stage_dropout",
       "bwd_chain_wide_stage", "linear_fwd")


def stage_models(p=0.0):
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.models.layers import Linear, Sequential

    return {
        "pp2_stage0": lambda: (MLP([784, 512, 512, 512, 512, 10], 0, 2, B,
                                   dropout=p, dropout_seed=SEED), 3, False),
        "pp3_stage1": lambda: (MLP([128] * 8 + [10], 1, 3, B, dropout=p,
                                   dropout_seed=SEED), 3, True),
        "bottom_48": lambda: (Sequential(
            [Linear(48, 128, "relu", dropout=p, layer_index=0),
             Linear(128, 128, "relu", dropout=p, layer_index=1)]), 2, True),
    }


def run_stage(make, device, fwd, bwd, calls, train=True):
    """A fresh stage model's (stashes, h_top, dx, gradients, op counts)."""
    model, _, _ = make()
    model.materialize_device(device)
    model.train() if train else model.eval()
    W = model.layers[-1].out_dims
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, model.layers[0].in_dims, generator=g).to(device, BF)
    dout = (torch.randn(B, W, generator=g) / 64).to(device, BF)
    model.zero_grad()
    calls.update(dict.fromkeys(OPS, 0))
    F.set_chain_wide(fwd)
    h_top = model.forward(x, 0)
    stash = [dict(l._cache) for l in model.layers]
    if not train:  # eval stashes nothing: forward only
        return stash, h_top, None, [], dict(calls)
    F.set_chain_wide(bwd)
    dx = model.backward(dout, 0)
    torch.cuda.synchronize()
    assert not any(l._cache for l in model.layers), "stash left behind"
    return (stash, h_top, dx, [p.grad.clone() for p in model.parameters()],
            dict(calls))


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("name", ["pp2_stage0", "pp3_stage1", "bottom_48"])
def test_model_stage_one_launch_each_way_bitwise(gpu_device, monkeypatch,
                                                 name, p):
    make = stage_models(p)[name]
    _, n, has_dx = make()
    calls = {}
    for op in OPS:
        def counted(*a, _op=op, _real=getattr(F, op), **k):
            calls[_op] += 1
            return _real(*a, **k)
        monkeypatch.setattr(F, op, counted)
    for flag in ("_CHAIN_WIDE", "_CHAIN_WIDE_DROPOUT", "_DETERMINISTIC",
                 "_DET_WGRAD"):
        monkeypatch.setattr(F, flag, getattr(F, flag))  # restored after
    F.set_deterministic(True)
    F.set_chain_wide_dropout(True)
    fwd_op = OPS[1] if p else OPS[0]
    off = run_stage(make, gpu_device, False, False, calls)
    assert [off[4][o] for o in OPS] == [0, 0, 0, 0 if p else n]
    # either backward can follow either forward
    for fwd, bwd in ((True, True), (True, False), (False, True)):
        stash, h_top, dx, grads, cnt = run_stage(make, gpu_device, fwd, bwd,
                                                 calls)
        assert cnt[fwd_op] == fwd and cnt[OPS[2]] == bwd
        assert cnt["linear_fwd"] == (0 if fwd or p else n)
        assert cnt[OPS[0]] + cnt[OPS[1]] == fwd
        for la, lb in zip(stash, off[0]):
            assert la.keys() == lb.keys() == {("x", 0), ("y", 0)}
            assert all(same_bits(la[k], lb[k]) for k in la)
        assert same_bits(h_top, off[1])
        assert (dx is not None) == has_dx
        assert dx is None or same_bits(dx, off[2])
        assert all(torch.equal(a, b) for a, b in zip(grads, off[3]))
    if p:  # eval mode: the plain stage op, the plain model's bits
        ev = run_stage(make, gpu_device, True, True, calls, train=False)
        assert (ev[4][OPS[0]], ev[4][OPS[1]]) == (1, 0)
        assert same_bits(ev[1], run_stage(make, gpu_device, False, False,
                                          calls, train=False)[1])
