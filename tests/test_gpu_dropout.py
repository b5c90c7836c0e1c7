"""Dropout on the GPU: the mask kernel against the CPU definition, the
fused GEMM epilogue through each register-staged tier, the standalone
pass, the scaled ReLU backward, the scaled backward chain, and the model.

The mask is exact everywhere (bit for bit against F.dropout_keep_mask on
the CPU).  Values:

  * p = 0.5: the scale 2 is exact, so y_drop == 2 * y_plain bit for bit.
  * p = 0.1 / 0.25: the epilogue rounds relu(acc + b) * scale ONCE, the
    plain kernel followed by a scaling rounds twice.  With v the f32
    value, |bf16(v) * s - v * s| <= s/2 ulp and each final rounding adds
    at most 1/2 ulp, so the two bf16 results are less than two grid
    steps apart: on the bf16 grid, at most ONE step (one bf16 ulp).  The
    tests compare bit patterns (monotone for the non-negative values
    here) and print the worst step count before asserting.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()
SEED = 0xFEED_F00D_0000_5EED
STEP, LAYER = 3, 2
ROW_FIRST, ROW_STRIDE = 7, 3


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def F_():
    from shallowspeed_amd.ops import functional as F

    return F


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.view(torch.int16).to(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def scale_of(p):
    return F_().dropout_params(p)[1]


def gpu_mask(rows, cols, p, device, first=ROW_FIRST, stride=ROW_STRIDE):
    ids = first + stride * torch.arange(rows, dtype=torch.int64, device=device)
    return F_().dropout_keep_mask(SEED, STEP, LAYER, ids, cols, p)


# ------------------------------------------------------------------- mask

@pytest.mark.parametrize("shape", [(96, 256), (33, 40), (1, 8)])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_mask_gpu_equals_cpu(gpu_device, shape, p):
    """Bit for bit; 33 x 40 has ragged columns (the last col >> 2 group
    is cut by N); ids include the top of the 32-bit range."""
    F = F_()
    rows, cols = shape
    ids = ROW_FIRST + ROW_STRIDE * torch.arange(rows, dtype=torch.int64)
    ids[-1] = (1 << 32) - 1
    want = F.dropout_keep_mask(SEED, STEP, LAYER, ids, cols, p)
    got = F.dropout_keep_mask(SEED, STEP, LAYER, ids.to(gpu_device), cols, p)
    assert got.is_cuda and got.dtype == torch.bool
    assert torch.equal(got.cpu(), want)
    if cols == 40:
        got37 = F.dropout_keep_mask(SEED, STEP, LAYER, ids.to(gpu_device),
                                    37, p)
        assert torch.equal(got37.cpu(), want[:, :37])


# --------------------------------------------------------- fused epilogue

_GEMM = {}


def gemm_case(shape, device):
    """Inputs and the plain bias+ReLU output, once per shape."""
    if shape not in _GEMM:
        M, N, K = shape
        a = randn(M, K, seed=100).to(device=device, dtype=BF)
        b = randn(N, K, seed=101).to(device=device, dtype=BF)
        bias = randn(N, seed=102).to(device=device, dtype=BF)
        y = ext().gemm_nt(a, b, bias, EMPTY, True)
        _GEMM[shape] = (a, b, bias, y)
    return _GEMM[shape]


def check_dropped(y_drop, y_plain, keep, p, what):
    """Zero pattern exact; kept values exact for p = 0.5, else within one
    bf16 grid step of the twice-rounded bf16(float(y_plain) * scale)."""
    assert torch.equal(y_drop == 0, ~keep | (y_plain == 0)), what
    s = scale_of(p)
    twice = torch.where(keep, (y_plain.float() * s).to(BF),
                        torch.zeros_like(y_plain))
    steps = (bits(y_drop) - bits(twice)).abs()
    print(f"{what}: p={p} kept {int(keep.sum())}/{keep.numel()} "
          f"max grid steps from the twice-rounded value {int(steps.max())} "
          f"({int((steps > 0).sum())} elements differ)")
    if p == 0.5:
        assert same_bits(y_drop, twice), what
    else:
        assert int(steps.max()) <= 1, what
    return int((steps > 0).sum())


# the shapes by which test_gemm_nt_epilogue_ladder reaches the three
# register-staged tiers, plus ragged M and N on the 32- and 64-row tiers
# (33 x 40: column quads cut by N; 1000 x 1000: partial last tiles)
@pytest.mark.parametrize("shape", [
    (32, 64, 32), (1024, 768, 32), (8200, 1024, 32), (33, 40, 48),
    (1000, 1000, 64),
], ids=["rows32", "rows64", "reg128", "ragged32", "ragged64"])
@pytest.mark.parametrize("p", [0.5, 0.1, 0.25])
def test_fused_epilogue(gpu_device, shape, p):
    F = F_()
    M, N, K = shape
    a, b, bias, y_plain = gemm_case(shape, gpu_device)
    keep = gpu_mask(M, N, p, gpu_device)
    assert 0 < int(keep.sum()) < keep.numel()
    key = (SEED, STEP, LAYER, ROW_FIRST, ROW_STRIDE, p)
    y = F.linear_fwd_dropout(a, b, bias, *key)
    differ = check_dropped(y, y_plain, keep, p, f"{shape}")
    # rounded once, in the epilogue: with an inexact scale some of the
    # >= 1000 kept values differ from the twice-rounded ones (a GEMM
    # followed by the standalone pass would match them all)
    assert p == 0.5 or differ > 0, "not the fused epilogue"
    again = F.linear_fwd_dropout(a, b, bias, *key)
    assert same_bits(y, again), "two runs differ"
    # another step draws another mask
    other = F.linear_fwd_dropout(a, b, bias, SEED, STEP + 1, LAYER,
                                 ROW_FIRST, ROW_STRIDE, p)
    assert not torch.equal(other == 0, y == 0)


# ------------------------------------------------------- standalone pass

@pytest.mark.parametrize("shape", [(8192, 1024, 32), (33, 40, 48)],
                         ids=["glds", "ragged"])
@pytest.mark.parametrize("p", [0.5, 0.25])
def test_dropout_fwd_standalone(gpu_device, shape, p):
    """Same mask as the fused path; values are the twice-rounded ones
    exactly.  8192 x 1024 x 32 is the ladder test's glds-tier shape:
    there linear_fwd_dropout itself takes GEMM + standalone pass."""
    F = F_()
    M, N, K = shape
    a, b, bias, y_plain = gemm_case(shape, gpu_device)
    keep = gpu_mask(M, N, p, gpu_device)
    key = (SEED, STEP, LAYER, ROW_FIRST, ROW_STRIDE, p)
    y = y_plain.clone()
    assert F.dropout_fwd_(y, *key) is y
    want = torch.where(keep, (y_plain.float() * scale_of(p)).to(BF),
                       torch.zeros_like(y_plain))
    assert same_bits(y, want)
    assert torch.equal(y == 0, ~keep | (y_plain == 0))
    via_linear = F.linear_fwd_dropout(a, b, bias, *key)
    if shape[0] == 8192:
        assert same_bits(via_linear, y), "glds tier: GEMM + standalone"
    else:
        check_dropped(via_linear, y_plain, keep, p, "fused vs standalone")
    forced = F.linear_fwd_dropout(a, b, bias, *key, fused=False)
    assert same_bits(forced, y)


# ------------------------------------------------------ scaled ReLU backward

@pytest.mark.parametrize("p", [0.5, 0.1])
def test_relu_bwd_scaled(gpu_device, p):
    """bf16(dy * scale) where y > 0, rounded once, else +0 — bit for bit,
    with -0.0, NaN and zeros in y; 33 x 41 leaves a scalar tail."""
    F = F_()
    s = scale_of(p)
    dy = randn(33, 41, seed=5).to(device=gpu_device, dtype=BF)
    y = randn(33, 41, seed=6)
    y[0, 3] = -0.0
    y[1, 5] = float("nan")
    y[2, :] = 0.0
    y[32, 40] = float("nan")
    y = y.to(device=gpu_device, dtype=BF)
    got = F.relu_bwd(dy, y, scale=s)
    want = torch.where(y > 0, (dy.float() * s).to(BF), torch.zeros_like(dy))
    assert same_bits(got, want)
    assert same_bits(F.relu_bwd(dy, y, scale=1.0), ext().relu_bwd(dy, y))


# ------------------------------------------------------------ scaled chain

H = 256
_CHAIN = {}


def one_hot(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(M, C)
    t[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1
    return t


def mask_source(M, seed):
    """As tests/test_gpu_bwd_chain.py: positives, negatives, an all-zero
    row and column, a -0.0 and one NaN."""
    h = randn(M, H, seed=seed)
    h[:, 7] = 0.0
    if M > 1:
        h[M // 2, :] = 0.0
    h[0, 3] = -0.0
    h[M - 1, 5] = float("nan")
    return h


def chain_case(M, depth, C, scale, device):
    """Seeded inputs and the unfused scaled chain head_bwd_fused ->
    relu_bwd(scale) -> gemm_nt(dz, W^T) -> ..., once per case."""
    key = (M, depth, C, scale)
    if key not in _CHAIN:
        e, F = ext(), F_()
        probs = torch.softmax(randn(M, C, seed=10 + M), dim=1)
        probs = probs.to(device=device, dtype=BF)
        t = one_hot(M, C, seed=20 + M).to(device=device, dtype=BF)
        w_head_t = (randn(C, H, seed=30 + C) / H ** 0.5).to(
            device=device, dtype=BF).t().contiguous()
        hs = [mask_source(M, seed=40 + 7 * l + M).to(device=device, dtype=BF)
              for l in range(depth)]
        w_ts = [(randn(H, H, seed=50 + l) / H ** 0.5)
                .to(device=device, dtype=BF).t().contiguous()
                for l in range(depth)]
        x = torch.zeros(M, H, device=device, dtype=BF)
        dz_head, dh = e.head_bwd_fused(probs, t, x, w_head_t, float(M),
                                       EMPTY, EMPTY)
        dzs = []
        for h, w_t in zip(hs, w_ts):
            dzs.append(F.relu_bwd(dh, h, scale=scale))
            dh = e.gemm_nt(dzs[-1], w_t, EMPTY, EMPTY, False)
        _CHAIN[key] = dict(probs=probs, t=t, w_head_t=w_head_t, hs=hs,
                           w_ts=w_ts, dz_head=dz_head, dzs=dzs, dx=dh)
    return _CHAIN[key]


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("M", [1, 31, 64, 97, 200])
def test_scaled_chain_bit_identical(gpu_device, M, depth, p):
    F = F_()
    scale = scale_of(p)
    c = chain_case(M, depth, 10, scale, gpu_device)
    args = (c["probs"], c["t"], c["w_head_t"], M)
    for arm in ((0, 0, 0), (64, 8, 0)):
        res = F.bwd_chain(*args, c["hs"], c["w_ts"], *arm, dz_scale=scale)
        assert res is not None, arm
        dz_head, dzs, dx = res
        assert same_bits(dz_head, c["dz_head"])
        for l in range(depth):
            assert same_bits(dzs[l], c["dzs"][l]), (arm, l)
        assert same_bits(dx, c["dx"])
    # the chain may end at dz of the last layer
    _, dzs, dx = F.bwd_chain(*args, c["hs"], c["w_ts"][:-1], dz_scale=scale)
    assert dx is None
    for l in range(depth):
        assert same_bits(dzs[l], c["dzs"][l])
    # the scale is real: the unscaled kernel gives other bits
    _, dzs1, _ = F.bwd_chain(*args, c["hs"], c["w_ts"])
    if M > 1:
        assert not same_bits(dzs1[0], c["dzs"][0])


def test_scaled_chain_other_arms_return_none(gpu_device):
    F = F_()
    M = 64
    c = chain_case(M, 1, 10, 2.0, gpu_device)
    args = (c["probs"], c["t"], c["w_head_t"], M, c["hs"], c["w_ts"])
    for arm in ((32, 4, 0), (32, 8, 0), (64, 4, 0), (64, 8, 1)):
        assert F.bwd_chain(*args, *arm) is not None, arm
        assert F.bwd_chain(*args, *arm, dz_scale=2.0) is None, arm


# ------------------------------------------------------------------- model

B = 96
SIZES = [48, 256, 256, 256, 10]
P = 0.25


@pytest.fixture
def flags():
    F = F_()
    yield F
    F.set_bwd_chain(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    F.set_deterministic(False)


def _inputs(device):
    x = randn(B, SIZES[0], seed=71).to(device=device, dtype=BF)
    t = one_hot(B, SIZES[-1], seed=72).to(device=device, dtype=BF)
    return x, t


def _model(device, dropout=P):
    from shallowspeed_amd.models import MLP

    return MLP(SIZES, 0, 1, B, loss="xent", dropout=dropout,
               dropout_seed=SEED).materialize_device(device)


def _train(device, F, chain, steps, calls):
    from shallowspeed_amd.models import SGD

    F.set_bwd_chain(chain)
    F.set_deterministic(True)
    model = _model(device)
    assert model._bwd_chain_plan(B) == (
        [(2, True), (1, True), (0, False)] if chain else None)
    opt = SGD(model.parameters(), lr=0.05)
    x, t = _inputs(device)
    real = F.bwd_chain

    def counted(*a, **k):
        res = real(*a, **k)
        calls.append((k.get("dz_scale", 1.0), res is not None))
        return res

    F.bwd_chain = counted
    try:
        for _ in range(steps):
            model.zero_grad()
            model.forward(x, 0)
            model.backward(t, 0)
            opt.step()
            model.dropout_step += 1
    finally:
        F.bwd_chain = real
    torch.cuda.synchronize()
    return ([p.data.clone() for p in model.parameters()],
            [p.grad.clone() for p in model.parameters()])


@pytest.mark.parametrize("steps", [1, 3])
def test_model_chain_equals_per_layer(gpu_device, flags, steps):
    """The scaled chain is taken (plan and launch), and deterministic
    training is bitwise equal to the per-layer path."""
    F = flags
    calls = []
    p_on, g_on = _train(gpu_device, F, True, steps, calls)
    assert calls == [(F.dropout_params(P)[1], True)] * steps
    calls = []
    p_off, g_off = _train(gpu_device, F, False, steps, calls)
    assert calls == []
    for a, b in zip(p_on + g_on, p_off + g_off):
        assert torch.equal(a, b)


def _stack(device, ps):
    """The model's layers with one drop probability per ReLU layer."""
    from shallowspeed_amd.models.layers import (Linear, Sequential,
                                                SoftmaxXent)

    dims = list(zip(SIZES[:-1], SIZES[1:]))
    layers = [Linear(a, b, "relu", dropout=p, layer_index=i)
              for i, ((a, b), p) in enumerate(zip(dims[:-1], ps))]
    layers += [Linear(*dims[-1]), SoftmaxXent(B)]
    model = Sequential(layers)
    model._skip_input_grad = True
    return model.materialize_device(device)


def test_model_mixed_p_takes_per_layer_path(gpu_device, flags):
    full = [(2, True), (1, True), (0, False)]
    assert _stack(gpu_device, (P, 0.0, P))._bwd_chain_plan(B) is None
    assert _stack(gpu_device, (P, 0.5, P))._bwd_chain_plan(B) is None
    assert _stack(gpu_device, (0.5, 0.5, 0.5))._bwd_chain_plan(B) == full
    assert _stack(gpu_device, (0.0, 0.0, 0.0))._bwd_chain_plan(B) == full
    x, t = _inputs(gpu_device)
    model = _stack(gpu_device, (P, 0.0, P))
    model.zero_grad()
    model.forward(x, 0)
    model.backward(t, 0)
    torch.cuda.synchronize()
    assert not any(l._cache for l in model.layers)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def _worker_run(device, F, nmu, graphed=False, steps=1, record=None):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import SGD
    from shallowspeed_amd.parallel import GPipeSchedule, Topology, Worker

    model = _model(device)
    opt = SGD(model.parameters(), lr=0.05)
    ds = Dataset(B, B // nmu, n_samples=B * 2, in_dim=SIZES[0],
                 n_classes=SIZES[-1], device=device).load(0, 1)
    w = Worker(Topology(device=device), model, ds, opt)
    real = F.linear_fwd_dropout
    if record is not None:
        def rec(x, wt, b, seed, step, layer, first, stride, p, fused=True):
            y = real(x, wt, b, seed, step, layer, first, stride, p, fused)
            record.append((layer, first, stride, y))
            return y

        F.linear_fwd_dropout = rec
    try:
        for s in range(steps):
            sched = GPipeSchedule(ds.num_mubatches(), 1, 0)
            (w.execute_graphed if graphed else w.execute)(sched, s % 2)
    finally:
        F.linear_fwd_dropout = real
    torch.cuda.synchronize()
    assert model.dropout_step == steps
    return model, w


def test_worker_one_vs_two_mubatches_same_activations(gpu_device, flags):
    """Each sample's hidden activations do not depend on how the batch
    is cut: the Worker tells the model which samples a µbatch holds."""
    F = flags
    F.set_deterministic(True)
    one, two = [], []
    _worker_run(gpu_device, F, 1, record=one)
    _worker_run(gpu_device, F, 2, record=two)
    assert [(l, f, s) for l, f, s, _ in one] == [(0, 0, 1), (1, 0, 1),
                                                 (2, 0, 1)]
    assert sorted((l, f, s) for l, f, s, _ in two) == sorted(
        (l, f, 1) for l in range(3) for f in (0, B // 2))
    for layer, _, _, y in one:
        halves = {f: yy for l, f, _, yy in two if l == layer}
        assert same_bits(y, torch.cat([halves[0], halves[B // 2]]))
        assert 0.5 < float((y == 0).float().mean()) < 0.75  # relu + p=0.25


def test_worker_graphed_equals_eager(gpu_device, flags):
    """execute_graphed runs eager under dropout (the step counter is a
    kernel argument): three steps equal execute, bitwise."""
    F = flags
    F.set_deterministic(True)
    m_e, _ = _worker_run(gpu_device, F, 1, graphed=False, steps=3)
    m_g, w = _worker_run(gpu_device, F, 1, graphed=True, steps=3)
    assert not getattr(w, "_graphs", {})
    for a, b in zip(m_e.parameters(), m_g.parameters()):
        assert torch.equal(a.data, b.data)


def test_model_eval_forward_is_plain(gpu_device, flags):
    x, _ = _inputs(gpu_device)
    drop, plain = _model(gpu_device), _model(gpu_device, dropout=0.0)
    train_out = drop.forward(x, 0)
    drop.eval()
    plain.eval()
    assert same_bits(drop.forward(x, 0), plain.forward(x, 0))
    assert not same_bits(train_out, plain.forward(x, 0))
