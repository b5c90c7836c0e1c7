"""Ordered split-K weight gradient (wgrad_part_kernel + wgrad_fold_kernel,
csrc/wgrad.hip): against float64 within the bound of an f32 sum of Kb
exact bf16 x bf16 products taken in any order,

    |g - ref| <= (Kb + 8) * 2^-24 * (|dz|^T |x| + |g0|)

(grad_ref_and_bound of test_gpu_head_fused), the fold's summation order
exactly, and run-to-run and path-to-path bit equality at model level.
"""

import pytest
import torch

from test_gpu_head_fused import (assert_within, ext, grad_ref_and_bound,
                                 rand_bf16)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SIZES = [784, 256, 256, 256, 10]

# (Kb, Mo, N, split, masked)
CASES = [
    (200, 256, 784, 2, False),   # 128 tiles, remainder n-tile, ragged slice
    (200, 256, 784, 0, True),    # the same shape, auto split
    (1064, 10, 256, 5, True),    # head remainder tile, last slice 40 rows
    (256, 64, 64, 4, False),     # one full 64 x 64 tile (LDS-DMA staging)
    (130, 72, 100, 4, True),     # split lowered to 3, remainder tiles
    (130, 30, 37, 4, False),     # odd widths: element stores and fold
    (64, 64, 64, 8, False),      # split collapses to 1: single owner
    (50, 10, 256, 3, True),      # the same at the head's shape
    (4096, 256, 256, 0, False),  # auto split 16, 256 blocks
]


def _run(F, dz_in, x, mask, g0w, g0b, split, pad, calls=1):
    """`calls` accumulations into copies of g0 that sit inside sentinel
    buffers; returns (gW, gb) after checking the sentinels."""
    Mo, N = g0w.shape
    bufs = []
    for g0 in (g0w, g0b):
        flat = torch.full((g0.numel() + 2 * pad,), -7.0, device=g0.device)
        flat[pad:pad + g0.numel()] = g0.flatten()
        bufs.append(flat)
    gw = bufs[0][pad:pad + Mo * N].view(Mo, N)
    gb = bufs[1][pad:pad + Mo]
    for _ in range(calls):
        F.linear_wgrad_acc(dz_in, x, gw, gb, mask, split_k=split,
                           ordered=True)
    torch.cuda.synchronize()
    for flat, n in zip(bufs, (Mo * N, Mo)):
        assert (flat[:pad] == -7).all() and (flat[pad + n:] == -7).all()
    return gw.clone(), gb.clone()


@pytest.mark.parametrize("Kb,Mo,N,split,masked", CASES)
def test_against_float64(gpu_device, Kb, Mo, N, split, masked):
    from shallowspeed_amd.ops import functional as F

    dy = rand_bf16(Kb, Mo, device=gpu_device, seed=Kb + Mo)
    x = rand_bf16(Kb, N, device=gpu_device, seed=Kb + N + 1)
    mask = rand_bf16(Kb, Mo, device=gpu_device, seed=7) if masked else None
    dz = dy * (mask > 0).to(BF) if masked else dy
    g0w = torch.randn(Mo, N, generator=torch.Generator().manual_seed(3))
    g0b = torch.randn(Mo, generator=torch.Generator().manual_seed(4))
    g0w, g0b = g0w.to(gpu_device), g0b.to(gpu_device)
    ref_w, ref_b, bnd_w, bnd_b = grad_ref_and_bound(dz, x, g0w, g0b, Kb)
    eff = ext().wgrad_ordered_plan(Kb, Mo, N, split)[0]
    print(f"effective split {eff}")
    # masked cases: 16-byte aligned gW; unmasked: 4-byte aligned only
    pad = 8 if masked else 7
    gw, gb = _run(F, dy, x, mask, g0w, g0b, split, pad)
    assert_within(gw, ref_w, bnd_w, "gW")
    assert_within(gb, ref_b, bnd_b, "gb")
    gw1, gb1 = _run(F, dy, x, mask, g0w, g0b, split, pad)
    assert torch.equal(gw, gw1) and torch.equal(gb, gb1)
    gw2, gb2 = _run(F, dy, x, mask, g0w, g0b, split, pad, calls=2)
    assert_within(gw2, 2 * ref_w - g0w.double().cpu(), bnd_w, "gW twice")
    assert_within(gb2, 2 * ref_b - g0b.double().cpu(), bnd_b, "gb twice")


def test_fold_order_exact(gpu_device):
    """Slices contribute 2^24, 1, -2^24 to the one element of gW and of
    gb; g0 = 1.  1 + ((2^24 + 1) - 2^24) is exactly 1.0 in f32."""
    from shallowspeed_amd.ops import functional as F

    dy = torch.zeros(192, 1)
    dy[:64], dy[64], dy[128:] = 2.0 ** 18, 1.0, -2.0 ** 18
    dy = dy.to(device=gpu_device, dtype=BF)
    x = torch.ones(192, 1, device=gpu_device, dtype=BF)
    assert tuple(ext().wgrad_ordered_plan(192, 1, 1, 3))[:2] == (3, 3)
    one = torch.ones(1, 1, device=gpu_device)
    gw, gb = _run(F, dy, x, None, one, one[0], 3, 8)
    assert gw.item() == 1.0 and gb.item() == 1.0


# ------------------------------------------------------------ model level

@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_deterministic(False)
    F.set_bwd_chain(True)
    F.set_fwd_chain(True)
    F.set_wgrad_group(True)


def _worker_grads(device, graphed=False, steps=1):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import (NaiveParallelSchedule, Topology,
                                           Worker)

    B = 192
    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device(device)
    opt = SGD(model.parameters(), lr=0.0)  # keep the weights fixed
    ds = Dataset(B, B, n_samples=B, in_dim=SIZES[0], n_classes=SIZES[-1],
                 device=device).load(0, 1)
    w = Worker(Topology(device=device), model, ds, opt)
    sched = NaiveParallelSchedule(ds.num_mubatches(), 1, 0)
    for _ in range(steps):
        (w.execute_graphed if graphed else w.execute)(sched, 0)
    torch.cuda.synchronize()
    if graphed:
        assert all(isinstance(g, torch.cuda.CUDAGraph)
                   for g in w._graphs.values()), "capture fell back to eager"
    return [p.grad.clone() for p in model.parameters()]


def test_model_paths_agree_bitwise(gpu_device, flags, monkeypatch):
    F = flags
    # the "single" run's wgrad operands give the float64 reference
    e, seen = ext(), []
    real = e.wgrad_tn
    monkeypatch.setattr(e, "wgrad_tn", lambda dy, x, gw, gb, m, s: (
        seen.append((dy, x, gw, gb, m)), real(dy, x, gw, gb, m, s))[1])
    F.set_deterministic(True, wgrad="single")
    _worker_grads(gpu_device)
    monkeypatch.undo()
    assert len(seen) == 4 and all(not m.numel() for *_, m in seen)

    F.set_deterministic(True, wgrad="ordered")
    got = _worker_grads(gpu_device)
    # launches: head, then top to bottom; parameters: W1, b1, ..., W4, b4
    for (dz, x, gw, gb, _), k in zip(seen, (3, 2, 1, 0)):
        assert got[2 * k].shape == gw.shape
        ref_w, ref_b, bnd_w, bnd_b = grad_ref_and_bound(
            dz, x, torch.zeros_like(gw), torch.zeros_like(gb), dz.shape[0])
        assert_within(got[2 * k], ref_w, bnd_w, f"gW {k}")
        assert_within(got[2 * k + 1], ref_b, bnd_b, f"gb {k}")

    def same(other):
        assert all(torch.equal(a, b) for a, b in zip(got, other))

    same(_worker_grads(gpu_device, graphed=True, steps=3))
    F.set_wgrad_group(False)
    same(_worker_grads(gpu_device))
    F.set_wgrad_group(True)
    F.set_bwd_chain(False)
    F.set_fwd_chain(False)
    same(_worker_grads(gpu_device))
