"""The flagship model's backward with the grouped weight-gradient call:
after the backward chain, Sequential issues the head's and the planned
layers' wgrads through ONE F.linear_wgrad_group call, which runs the
head and the two hidden layers in one launch and the first layer alone.

Gradients are held against the per-layer path (set_wgrad_group(False))
to the bound of test_wgrad_onchip_reduce's normal-data test,
atol = 1e-2 + 1e-3 * max|ref|, rtol = 2e-2; deterministic mode and
deferred wgrad keep the per-layer launches.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SIZES = [784, 256, 256, 256, 10]
ROWS = [192, 97]


def _ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


@pytest.fixture
def flags():
    from shallowspeed_amd.ops import functional as F

    yield F
    F.set_wgrad_group(True)
    F.set_deterministic(False)


@pytest.fixture
def spy(monkeypatch):
    """Records the (Kb, Mo, N) shapes of every wgrad_tn_group call."""
    e = _ext()
    real, calls = e.wgrad_tn_group, []

    def rec(problems, splits=None):
        calls.append([(dy.shape[0], dy.shape[1], x.shape[1])
                      for dy, x, _, _ in problems])
        return real(problems, splits)

    monkeypatch.setattr(e, "wgrad_tn_group", rec)
    return calls


def _inputs(device, rows):
    g = torch.Generator().manual_seed(71 + rows)
    x = torch.randn(rows, SIZES[0], generator=g).to(device=device, dtype=BF)
    t = torch.zeros(rows, SIZES[-1])
    t[torch.arange(rows), torch.randint(0, SIZES[-1], (rows,), generator=g)] = 1
    return x, t.to(device=device, dtype=BF)


def _grads(device, rows, defer=False):
    from shallowspeed_amd.models import MLP

    model = MLP(SIZES, 0, 1, rows, loss="xent").materialize_device(device)
    if defer:
        model.set_defer_wgrad(True)
    x, t = _inputs(device, rows)
    model.zero_grad()
    model.forward(x, 0)
    model.backward(t, 0)
    if defer:
        model.flush_wgrads()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in model.parameters()]


def _close(got, ref):
    for g, r in zip(got, ref):
        torch.testing.assert_close(
            g, r, atol=1e-2 + 1e-3 * r.abs().max().item(), rtol=2e-2)


@pytest.mark.parametrize("rows", ROWS)
def test_one_group_call_per_backward(gpu_device, flags, spy, rows):
    F = flags
    got = _grads(gpu_device, rows)
    assert len(spy) == 1
    shapes = spy[0]
    assert shapes == [(rows, 10, 256), (rows, 256, 256), (rows, 256, 256),
                      (rows, 256, 784)]  # head, L3, L2, L1
    assert [la["problems"] for la in F.wgrad_group_plan(shapes)] == \
        [[0, 1, 2], [3]]
    F.set_wgrad_group(False)
    ref = _grads(gpu_device, rows)
    assert len(spy) == 1
    assert all(r.abs().max() > 0 for r in ref)
    _close(got, ref)


@pytest.mark.parametrize("rows", ROWS)
def test_deterministic_mode_keeps_the_per_layer_launches(gpu_device, flags,
                                                         spy, rows):
    F = flags
    F.set_deterministic(True)
    got = _grads(gpu_device, rows)
    assert spy == []
    F.set_wgrad_group(False)
    ref = _grads(gpu_device, rows)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_deferred_wgrad_does_not_take_the_group_call(gpu_device, flags, spy):
    F = flags
    got = _grads(gpu_device, 192, defer=True)
    assert spy == []
    F.set_wgrad_group(False)
    _close(got, _grads(gpu_device, 192))


def _worker_grads(device, graphed, steps):
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
    return w, [p.grad.clone() for p in model.parameters()]


def test_execute_graphed_replays_the_group_launch(gpu_device, flags, spy):
    F = flags
    w, got = _worker_grads(gpu_device, True, 3)
    assert all(isinstance(g, torch.cuda.CUDAGraph)
               for g in w._graphs.values()), "capture fell back to eager"
    assert len(spy) >= 1  # eager warm-up and capture; replays call nothing
    F.set_wgrad_group(False)
    n = len(spy)
    _, ref = _worker_grads(gpu_device, False, 1)
    assert len(spy) == n
    _close(got, ref)
