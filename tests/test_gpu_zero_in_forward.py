"""zero_grad(defer=True): the step's first forward chain launch writes
the zeros of the flat gradient buffer (F.fwd_chain(zero=...)).

The buffer is filled with NaN first, so a single element the launch
missed, or a kernel that added to the buffer ahead of the zeros, shows
in the gradients, which must equal a run with zero_grad(defer=False) bit
for bit (deterministic mode: no atomics, so the bits are defined).

The deferral ships switched off (F.fwd_zero_grads(), SS_FWD_ZERO_GRADS);
the fixture below turns it on.

Model [40, 256, 256, 10]: 78858 gradient floats = 315432 bytes, not a
multiple of 16, so the launch ends in 4-byte stores; 97 rows per
micro-batch = two 64-row tiles, four 32-row tiles, the last ragged.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SIZES = [40, 256, 256, 10]
B = 97  # rows per micro-batch


@pytest.fixture
def F():
    from shallowspeed_amd.ops import functional as F

    saved = (F._FWD_CHAIN, F._FWD_ZERO_GRADS)
    F.set_fwd_chain(True)
    F._FWD_ZERO_GRADS = True
    F.set_deterministic(True)
    yield F
    F._FWD_CHAIN, F._FWD_ZERO_GRADS = saved
    F.set_deterministic(False)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def inputs(device, n_mu):
    g = torch.Generator().manual_seed(7)
    xs, ts = [], []
    for m in range(n_mu):
        xs.append(randn(B, SIZES[0], seed=11 + m).to(device=device, dtype=BF))
        t = torch.zeros(B, SIZES[-1])
        t[torch.arange(B), torch.randint(0, SIZES[-1], (B,), generator=g)] = 1
        ts.append(t.to(device=device, dtype=BF))
    return xs, ts


def spy_zero(F, monkeypatch, refuse=False):
    """Counts the chain launches that carried the gradient buffer."""
    seen = {"calls": 0, "zero": 0}
    real = F.fwd_chain

    def chain(*a, **k):
        seen["calls"] += 1
        seen["zero"] += k.get("zero") is not None
        return None if refuse else real(*a, **k)

    monkeypatch.setattr(F, "fwd_chain", chain)
    return seen


def step(device, n_mu, defer, sizes=SIZES, after_forward=None):
    """NaN into the flat buffer, zero_grad, then one step's forwards and
    backwards in naive (n_mu = 1) or GPipe order (all forwards, then the
    backwards last micro-batch first).  Returns (model, grads)."""
    from shallowspeed_amd.models import MLP

    model = MLP(sizes, 0, 1, B * n_mu, loss="xent").materialize_device(device)
    assert model._flat_grad.numel() * 4 % 16 != 0
    xs, ts = inputs(device, n_mu)
    model._flat_grad.fill_(float("nan"))
    model.zero_grad(defer=defer)
    for m in range(n_mu):
        model.forward(xs[m], m)
        if after_forward is not None:
            after_forward(model, m)
    for m in reversed(range(n_mu)):
        model.backward(ts[m], m)
    torch.cuda.synchronize()
    return model, [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("n_mu", [1, 2], ids=["naive", "gpipe2"])
def test_deferred_zero_equals_memset(gpu_device, F, monkeypatch, n_mu):
    seen = spy_zero(F, monkeypatch)
    _, want = step(gpu_device, n_mu, defer=False)
    assert seen == {"calls": n_mu, "zero": 0}

    def marks(model, m):
        # the first forward took the buffer along; nothing is owed
        assert not model._zero_pending

    model, got = step(gpu_device, n_mu, defer=True, after_forward=marks)
    assert seen == {"calls": 2 * n_mu, "zero": 1}
    assert torch.isfinite(model._flat_grad).all()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert any(g.abs().sum() > 0 for g in got)


def test_mark_stays_until_the_forward(gpu_device, F):
    from shallowspeed_amd.models import MLP

    model = MLP(SIZES, 0, 1, B).materialize_device(gpu_device)
    model._flat_grad.fill_(float("nan"))
    model.zero_grad(defer=True)
    assert model._zero_pending
    assert torch.isnan(model._flat_grad).all()  # nothing launched yet
    model.zero_grad()  # without defer: the memset, and no mark
    assert not model._zero_pending
    assert (model._flat_grad == 0).all()
    # a reader ahead of any forward gets the memset
    model._flat_grad.fill_(float("nan"))
    model.zero_grad(defer=True)
    model.flush_wgrads()
    assert not model._zero_pending and (model._flat_grad == 0).all()


def test_switched_off(gpu_device, F):
    from shallowspeed_amd.models import MLP

    F._FWD_ZERO_GRADS = False
    model = MLP(SIZES, 0, 1, B).materialize_device(gpu_device)
    model._flat_grad.fill_(float("nan"))
    model.zero_grad(defer=True)
    assert not model._zero_pending and (model._flat_grad == 0).all()


def test_no_chain_plan_zeroes_at_once(gpu_device, F):
    from shallowspeed_amd.models import MLP

    narrow = [40, 128, 128, 10]
    model = MLP(narrow, 0, 1, B).materialize_device(gpu_device)
    assert model._fwd_chain_plan() is None
    model._flat_grad.fill_(float("nan"))
    model.zero_grad(defer=True)
    assert not model._zero_pending
    assert (model._flat_grad == 0).all()


def test_refused_launch_zeroes_before_the_backward(gpu_device, F,
                                                   monkeypatch):
    _, want = step(gpu_device, 1, defer=False)
    seen = spy_zero(F, monkeypatch, refuse=True)

    def zeroed(model, m):
        assert not model._zero_pending
        assert (model._flat_grad == 0).all()

    _, got = step(gpu_device, 1, defer=True, after_forward=zeroed)
    assert seen == {"calls": 1, "zero": 1}
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n_mu", [1, 2], ids=["naive", "gpipe2"])
def test_worker_defers(gpu_device, F, monkeypatch, n_mu):
    """Worker._zero_grad defers: one launch per step carries the buffer
    and the step's gradients equal those with the deferral off."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import (GPipeSchedule,
                                           NaiveParallelSchedule, Topology,
                                           Worker)

    seen = spy_zero(F, monkeypatch)

    def run(on):
        F._FWD_ZERO_GRADS = on
        model = MLP(SIZES, 0, 1, B * n_mu).materialize_device(gpu_device)
        opt = SGD(model.parameters(), lr=0.0)
        ds = Dataset(B * n_mu, B, n_samples=B * n_mu, in_dim=SIZES[0],
                     n_classes=SIZES[-1], device=gpu_device).load(0, 1)
        w = Worker(Topology(device=gpu_device), model, ds, opt)
        sched = (NaiveParallelSchedule if n_mu == 1 else GPipeSchedule)(
            ds.num_mubatches(), 1, 0)
        model._flat_grad.fill_(float("nan"))
        w.execute(sched, 0)
        torch.cuda.synchronize()
        return [p.grad.clone() for p in model.parameters()]

    want = run(False)
    assert seen["zero"] == 0
    got = run(True)
    assert seen["zero"] == 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n,lead", [(78858, 0), (78858, 1), (3, 0), (5, 3),
                                    (131072 * 4 + 7, 0)])
def test_kernel_zeroes_exactly_the_buffer(gpu_device, F, n, lead):
    """n floats starting `lead` floats past a 16-byte boundary: all of
    them become zero, the floats on either side stay NaN, and the
    forward's own outputs are what they are without the buffer."""
    M, K0, H, C = 97, 40, 256, 10
    x = randn(M, K0, seed=1).to(device=gpu_device, dtype=BF)
    ws = [(randn(H, K0, seed=2) / K0 ** 0.5).to(device=gpu_device, dtype=BF)]
    bs = [randn(H, seed=3).to(device=gpu_device, dtype=BF)]
    wh = (randn(C, H, seed=4) / 16).to(device=gpu_device, dtype=BF)
    bh = randn(C, seed=5).to(device=gpu_device, dtype=BF)
    hs0, p0 = F.fwd_chain(x, ws, bs, wh, bh)
    pad = 4
    buf = torch.full((pad + lead + n + pad,), float("nan"),
                     device=gpu_device)
    assert buf.data_ptr() % 16 == 0
    zero = buf[pad + lead:pad + lead + n]
    for arm in ((0, 0), (64, 8), (32, 8), (64, 4)):
        buf.fill_(float("nan"))
        hs, p = F.fwd_chain(x, ws, bs, wh, bh, *arm, zero=zero)
        assert (zero == 0).all(), arm
        assert torch.isnan(buf[:pad + lead]).all(), arm
        assert torch.isnan(buf[pad + lead + n:]).all(), arm
        assert torch.equal(hs[0].view(torch.int16), hs0[0].view(torch.int16))
        assert torch.equal(p.view(torch.int16), p0.view(torch.int16))
    # not a float buffer, or on another device: refused, nothing written
    buf.fill_(float("nan"))
    assert F.fwd_chain(x, ws, bs, wh, bh, zero=buf.double()) is None
    assert F.fwd_chain(x, ws, bs, wh, bh, zero=buf[::2]) is None
    assert torch.isnan(buf).all()
