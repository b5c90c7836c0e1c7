"""Ordered grouped weight gradient (wgrad_group_part_kernel +
wgrad_group_fold_kernel, csrc/wgrad.hip): against float64 within the
bound of an f32 sum of Kb exact bf16 x bf16 products taken in any order,

    |g - ref| <= (Kb + 8) * 2^-24 * (|dz|^T |x| + |g0|)

(grad_ref_and_bound of test_gpu_head_fused), the fold's tree order
exactly, bit equality with the ordered path where the contract promises
it (S <= W), and the model under set_deterministic(True, wgrad="grouped").
"""

import functools

import pytest
import torch

from test_gpu_head_fused import (assert_within, ext, grad_ref_and_bound,
                                 rand_bf16)

BF = torch.bfloat16
SIZES = [784, 256, 256, 256, 10]
HEAD3 = lambda Kb: [(Kb, 10, 256), (Kb, 256, 256), (Kb, 256, 256)]

# problems as (Kb, Mo, N), splits (None = the group rule)
GROUPS = {
    "small-auto": (HEAD3(200), None),       # ragged slice, head remainder
    "explicit": (HEAD3(1064), (5, 3, 2)),
    "odd-widths": ([(130, 30, 37), (130, 7, 66)], (4, 4)),  # element paths
    "collapse": ([(64, 64, 64), (256, 64, 64)], (4, 4)),  # split 1 beside 4
    "run-of-one": ([(200, 256, 784)], None),              # 128 x 128 form
    "two-launches": ([(200, 10, 256), (200, 256, 784)], None),
    "flagship-splits": (HEAD3(4096), None),
}


@functools.lru_cache(maxsize=None)
def _case(name, device):
    """Operands, seeded g0 and the float64 reference of a group, once."""
    out = []
    for i, (Kb, Mo, N) in enumerate(GROUPS[name][0]):
        dy = rand_bf16(Kb, Mo, device=device, seed=Kb + Mo + i)
        x = rand_bf16(Kb, N, device=device, seed=Kb + N + 1 + i)
        g0w = torch.randn(Mo, N, generator=torch.Generator().manual_seed(3))
        g0b = torch.randn(Mo, generator=torch.Generator().manual_seed(4))
        g0w, g0b = g0w.to(device), g0b.to(device)
        out.append((dy, x, g0w, g0b, grad_ref_and_bound(dy, x, g0w, g0b, Kb)))
    return out


def _run(call, case, pad, calls=1):
    """`calls` accumulations into copies of every g0 that sit inside
    sentinel buffers; returns [(gW, gb)] after checking the sentinels."""
    bufs, probs = [], []
    for dy, x, g0w, g0b, _ in case:
        views = []
        for g0 in (g0w, g0b):
            flat = torch.full((g0.numel() + 2 * pad,), -7.0, device=dy.device)
            flat[pad:pad + g0.numel()] = g0.flatten()
            bufs.append((flat, g0.numel()))
            views.append(flat[pad:pad + g0.numel()].view(g0.shape))
        probs.append((dy, x, *views))
    for _ in range(calls):
        call(probs)
    torch.cuda.synchronize()
    for flat, n in bufs:
        assert (flat[:pad] == -7).all() and (flat[pad + n:] == -7).all()
    return [(gw.clone(), gb.clone()) for _, _, gw, gb in probs]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [8, 7], ids=["align16", "align4"])
@pytest.mark.parametrize("name", list(GROUPS))
def test_against_float64(gpu_device, name, pad):
    from shallowspeed_amd.ops import functional as F

    case, splits = _case(name, gpu_device), GROUPS[name][1]
    print(ext().wgrad_group_ordered_plan(GROUPS[name][0], splits))
    call = lambda p: F.linear_wgrad_group(p, splits, ordered=True)
    got = _run(call, case, pad)
    twice = _run(call, case, pad, calls=2)
    for k, ((gw, gb), (gw2, gb2), (_, _, g0w, g0b, ref)) in enumerate(
            zip(got, twice, case)):
        ref_w, ref_b, bnd_w, bnd_b = ref
        assert_within(gw, ref_w, bnd_w, f"gW {k}")
        assert_within(gb, ref_b, bnd_b, f"gb {k}")
        assert_within(gw2, 2 * ref_w - g0w.double().cpu(), bnd_w, "gW twice")
        assert_within(gb2, 2 * ref_b - g0b.double().cpu(), bnd_b, "gb twice")
    for (a, b), (c, d) in zip(got, _run(call, case, pad)):
        assert torch.equal(a, c) and torch.equal(b, d)


@pytest.mark.gpu
def test_fold_order_exact(gpu_device):
    """S = 2 W slices contribute 2^24, 1, 1, -2^24, 0, ... to the one
    element of gW and of gb; g0 = 1.  By the contract (docs/KERNELS.md)
    wave w sums slices [2w, 2w + 2) and wave 0 the run sums in wave
    order: 1 + ((2^24 + 1) + (1 - 2^24)) = 2.0; the serial order gives 1.0."""
    from shallowspeed_amd.ops import functional as F

    W = ext().WGRAD_FOLD_WAVES
    S = 2 * W
    p = torch.zeros(S)
    p[:4] = torch.tensor([2.0 ** 24, 1.0, 1.0, -2.0 ** 24])
    c = -(-S // W)
    t = None
    for w in range(-(-S // c)):
        q = p[w * c]
        for s in range(w * c + 1, min(S, (w + 1) * c)):
            q = q + p[s]
        t = q if t is None else t + q
    want = (torch.ones(()) + t).item()
    assert want == 2.0
    dy = torch.zeros(64 * S, 1)
    dy[:64], dy[64], dy[128], dy[192:256] = 2.0 ** 18, 1.0, 1.0, -2.0 ** 18
    dy = dy.to(device=gpu_device, dtype=BF)
    x = torch.ones(64 * S, 1, device=gpu_device, dtype=BF)
    launches, _ = ext().wgrad_group_ordered_plan([(64 * S, 1, 1)], [S])
    assert [tuple(la[1]) for la in launches] == [(S,)]
    one = torch.ones(1, 1, device=gpu_device)
    case = [(dy, x, one, one[0], None)]
    (gw, gb), = _run(lambda pr: F.linear_wgrad_group(pr, [S], ordered=True),
                     case, 8)
    assert gw.item() == want and gb.item() == want


@pytest.mark.gpu
@pytest.mark.parametrize("Kb,Mo,N,S", [(1064, 10, 256, 4), (256, 64, 64, 4)])
def test_equals_ordered_up_to_w_slices(gpu_device, Kb, Mo, N, S):
    from shallowspeed_amd.ops import functional as F

    assert S <= ext().WGRAD_FOLD_WAVES
    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=Kb)
    x = rand_bf16(Kb, N, device=gpu_device, seed=N)
    g0w = torch.randn(Mo, N, generator=torch.Generator().manual_seed(3))
    g0b = torch.randn(Mo, generator=torch.Generator().manual_seed(4))
    case = [(dy, x, g0w.to(gpu_device), g0b.to(gpu_device), None)]
    (gw, gb), = _run(lambda p: F.linear_wgrad_group(p, [S], ordered=True),
                     case, 8)
    (rw, rb), = _run(lambda p: F.linear_wgrad_acc(*p[0], split_k=S,
                                                  ordered=True), case, 8)
    assert torch.equal(gw, rw) and torch.equal(gb, rb)


# ------------------------------------------------------------ model level

@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_deterministic(False)


def _worker_grads(device, graphed):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import (NaiveParallelSchedule, Topology,
                                           Worker)

    B = 200
    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(device)
    opt = SGD(model.parameters(), lr=0.0)  # keep the weights fixed
    ds = Dataset(B, B, n_samples=B, in_dim=SIZES[0], n_classes=SIZES[-1],
                 device=device).load(0, 1)
    w = Worker(Topology(device=device), model, ds, opt)
    sched = NaiveParallelSchedule(ds.num_mubatches(), 1, 0)
    for _ in range(2):
        (w.execute_graphed if graphed else w.execute)(sched, 0)
    torch.cuda.synchronize()
    if graphed:
        assert all(isinstance(g, torch.cuda.CUDAGraph)
                   for g in w._graphs.values()), "capture fell back to eager"
    return [p.grad.clone() for p in model.parameters()]


@pytest.mark.gpu
def test_model_grouped_mode(gpu_device, flags, monkeypatch):
    F = flags
    # the "ordered" run's wgrad operands give the float64 reference
    e, seen, calls = ext(), [], []
    real = e.wgrad_tn_ordered
    monkeypatch.setattr(e, "wgrad_tn_ordered", lambda dy, x, gw, gb, m, s: (
        seen.append((dy, x, gw, gb)), real(dy, x, gw, gb, m, s))[1])
    F.set_deterministic(True, wgrad="ordered")
    _worker_grads(gpu_device, False)
    monkeypatch.undo()
    seen = seen[-4:]  # the second step's: head, then top to bottom

    real_group = F.linear_wgrad_group
    monkeypatch.setattr(F, "linear_wgrad_group", lambda p, s=None, **kw: (
        calls.append(kw), real_group(p, s, **kw))[1])
    F.set_deterministic(True, wgrad="grouped")
    eager = _worker_grads(gpu_device, False)
    graphed = _worker_grads(gpu_device, True)
    assert calls and all(kw == {"ordered": True} for kw in calls)
    assert all(torch.equal(a, b) for a, b in zip(eager, graphed))
    # parameters: W1, b1, ..., W4, b4
    for (dz, x, gw, gb), k in zip(seen, (3, 2, 1, 0)):
        assert eager[2 * k].shape == gw.shape
        ref_w, ref_b, bnd_w, bnd_b = grad_ref_and_bound(
            dz, x, torch.zeros_like(gw), torch.zeros_like(gb), dz.shape[0])
        assert_within(eager[2 * k], ref_w, bnd_w, f"gW {k}")
        assert_within(eager[2 * k + 1], ref_b, bnd_b, f"gb {k}")


@pytest.mark.gpu
def test_model_grouped_mode_hooks(gpu_device, flags):
    """Every parameter's hook fires once, after the launch that holds
    its gradient: what it reads on the stream is the final value."""
    from shallowspeed_amd.models import MLP

    flags.set_deterministic(True, wgrad="grouped")
    model = MLP(SIZES, 0, 1, 200, loss="xent").materialize_device(gpu_device)
    index = {id(p): k for k, p in enumerate(model.parameters())}
    fired = []
    model.register_grad_hook(
        lambda p: fired.append((index[id(p)], p.grad.clone())))
    x = rand_bf16(200, SIZES[0], device=gpu_device, seed=1)
    t = torch.zeros(200, SIZES[-1], device=gpu_device, dtype=BF)
    t[:, 3] = 1
    model.zero_grad()
    model.forward(x, 0)
    model.backward(t, 0)
    torch.cuda.synchronize()
    grads = [p.grad for p in model.parameters()]
    assert sorted(k for k, _ in fired) == list(range(len(grads)))
    for k, g in fired:
        assert g.abs().max() > 0 and torch.equal(g, grads[k])


# -------------------------------------------------------------------- CPU

def test_cpu_ordered_equals_plain_and_mode_is_accepted(monkeypatch):
    from shallowspeed_amd.ops import functional as F

    g = torch.Generator().manual_seed(5)
    probs = [(torch.randn(33, m, generator=g), torch.randn(33, n, generator=g))
             for m, n in ((7, 12), (5, 9))]
    out = []
    for kw in ({}, {"ordered": True}):
        grads = [(torch.ones(dy.shape[1], x.shape[1]), torch.ones(dy.shape[1]))
                 for dy, x in probs]
        F.linear_wgrad_group([(dy, x, gw, gb) for (dy, x), (gw, gb)
                              in zip(probs, grads)], **kw)
        out.append(grads)
    for (a, b), (c, d) in zip(*out):
        assert torch.equal(a, c) and torch.equal(b, d)
    for name in ("_DETERMINISTIC", "_DET_WGRAD"):
        monkeypatch.setattr(F, name, getattr(F, name))  # restored after
    F.set_deterministic(True, wgrad="grouped")
    assert F.deterministic() and F.deterministic_wgrad() == "grouped"
