"""Training metrics on device (csrc/head.hip): head_metrics_kernel and
the METRICS instantiations of head_bwd_fused_kernel, then the Worker.

Reference: float64 on the CPU from the SAME bf16 tensors.  Counts
(correct, rows, nonfinite) must be exactly equal.  The loss sum is an f32
sum of M non-negative row terms taken in an order the kernels are free to
choose, so it is held to the worst case of such a sum,

    |got - ref| <= (M + 16) * 2^-24 * sum|row_loss|,

M roundings for the row sum in any order plus 16 for logf, the product
and the sum inside a row.  The bound does not depend on the code under
test.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMPTY = torch.Tensor()
FLT_MIN = 1.1754943508222875e-38


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def fn():
    from shallowspeed_amd.ops import functional as F

    return F


def ref_totals(probs, target, kind):
    """f64 totals of the metric definition, plus the loss bound."""
    p, t = probs.double().cpu(), target.double().cpu()
    M = p.shape[0]
    fin = torch.isfinite(p).all(dim=1)
    if kind == "xent":
        logp = torch.log(torch.clamp(p, min=FLT_MIN))
        terms = torch.where(t != 0, -t * logp, torch.zeros_like(p))
    else:
        terms = (t - p) ** 2
    row = torch.where(fin, terms.sum(dim=1), torch.zeros(M, dtype=p.dtype))
    hit = (p.argmax(dim=1) == t.argmax(dim=1)) & fin
    return dict(loss_sum=row.sum().item(), correct=int(hit.sum()), rows=M,
                nonfinite=int((~fin).sum()),
                bound=(M + 16) * 2.0 ** -24 * row.abs().sum().item())


def check(got, ref, what, scale=1):
    """got (a read_metrics_acc dict) against `scale` times ref."""
    err = abs(got["loss_sum"] - scale * ref["loss_sum"])
    print(f"{what}: loss_sum {got['loss_sum']!r} ref "
          f"{scale * ref['loss_sum']!r} err {err:.3e} bound "
          f"{scale * ref['bound']:.3e}; counts "
          f"{got['correct']}/{got['rows']}/{got['nonfinite']}")
    for k in ("correct", "rows", "nonfinite"):
        assert got[k] == scale * ref[k], (what, k, got[k], scale * ref[k])
    assert err <= scale * ref["bound"], (what, err, scale * ref["bound"])


_CASES = {}


def case(M, C, device):
    """Seeded softmax probs and one-hot targets in bf16, with the special
    rows where they fit; computed once per shape and never modified."""
    key = (M, C)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * M + C)
        p = torch.softmax(torch.randn(M, C, generator=g) * 2.0, dim=1)
        lab = torch.randint(0, C, (M,), generator=g)
        t = torch.zeros(M, C)
        t[torch.arange(M), lab] = 1
        if M >= 5:
            p[0, :] = 0.25          # all tied: argmax is column 0
            t[0, :] = 0
            t[0, 0] = 1             # ... which the target names
            if C >= 3:
                p[1, :] = 0.125
                p[1, 1] = p[1, 2] = 0.375   # tie: the lower index 1 wins
                t[1, :] = 0
                t[1, 2] = 1                 # ... so this row is wrong
            p[2, lab[2]] = 0.0      # zero prob under the 1: -log FLT_MIN
            p[3, C // 2] = float("nan")
            p[4, 0] = float("inf")
        if M >= 257:
            p[200, C - 1] = float("-inf")
            p[256, 0] = float("nan")  # the last row, alone in its block
        _CASES[key] = (p.to(device=device, dtype=BF),
                       t.to(device=device, dtype=BF))
    return _CASES[key]


def shipped_slots():
    return fn().METRICS_SLOTS


# ---------------------------------------------------------- standalone

@pytest.mark.parametrize("kind", ["xent", "mse"])
@pytest.mark.parametrize("C", [1, 10, 16, 17, 65, 130])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 257])
def test_standalone_matches_f64(gpu_device, M, C, kind):
    F = fn()
    p, t = case(M, C, gpu_device)
    ref = ref_totals(p, t, kind)
    if M >= 5:
        assert ref["nonfinite"] >= 2 and ref["correct"] >= 1
    for slots in (1, shipped_slots()):
        acc = F.new_metrics_acc(gpu_device, slots=slots)
        assert acc.shape == (slots, 4)
        F.head_metrics(p, t, acc, kind)
        check(F.read_metrics_acc(acc), ref, f"M{M} C{C} {kind} S{slots}")


def test_special_rows(gpu_device):
    """Each special row on its own, so that a wrong one is named."""
    F = fn()
    p, t = case(5, 10, gpu_device)
    want = [  # (row, correct, nonfinite, loss or None)
        (0, 1, 0, None), (1, 0, 0, None),
        (2, None, 0, 87.33654475), (3, 0, 1, 0.0), (4, 0, 1, 0.0)]
    for r, correct, bad, loss in want:
        acc = F.new_metrics_acc(gpu_device, slots=1)
        F.head_metrics(p[r:r + 1].contiguous(), t[r:r + 1].contiguous(), acc)
        got = F.read_metrics_acc(acc)
        print(r, got)
        assert got["rows"] == 1 and got["nonfinite"] == bad
        if correct is not None:
            assert got["correct"] == correct
        if loss is not None:
            assert abs(got["loss_sum"] - loss) <= 17 * 2.0 ** -24 * loss
            assert got["loss_sum"] == got["loss_sum"]  # finite, not NaN


def test_two_calls_add_up_and_reset(gpu_device):
    F = fn()
    p, t = case(257, 10, gpu_device)
    ref = ref_totals(p, t, "xent")
    acc = F.new_metrics_acc(gpu_device)
    F.head_metrics(p, t, acc)
    F.head_metrics(p, t, acc)
    check(F.read_metrics_acc(acc, reset=False), ref, "two calls", scale=2)
    check(F.read_metrics_acc(acc, reset=True), ref, "again", scale=2)
    assert F.read_metrics_acc(acc) == dict(loss_sum=0.0, correct=0, rows=0,
                                           nonfinite=0)
    assert not acc.any()


def test_near_uniform_ties_follow_torch_argmax(gpu_device):
    """bf16 softmax of N(0, 0.05^2) logits ties its maxima in several
    percent of the rows; the lowest index must win, as in torch."""
    F = fn()
    M, C, K = 4096, 10, 32
    g = torch.Generator().manual_seed(5)
    p = torch.softmax(torch.randn(M, C, generator=g) * 0.05, dim=1).to(BF)
    lab = torch.randint(0, C, (M,), generator=g)
    t = torch.zeros(M, C)
    t[torch.arange(M), lab] = 1
    pf = p.float()
    tied = (pf == pf.max(dim=1, keepdim=True).values).sum(dim=1) > 1
    assert tied.float().mean().item() > 0.01, "the case has no ties"
    want = int((pf.argmax(dim=1) == lab).sum())
    pd, td = p.to(gpu_device), t.to(device=gpu_device, dtype=BF)
    acc = F.new_metrics_acc(gpu_device)
    F.head_metrics(pd, td, acc)
    assert F.read_metrics_acc(acc)["correct"] == want
    x = torch.zeros(M, K, device=gpu_device, dtype=BF)
    w_t = torch.zeros(K, C, device=gpu_device, dtype=BF)
    F.head_bwd_fused(pd, td, x, w_t, M, metrics=acc)
    assert F.read_metrics_acc(acc)["correct"] == want


# --------------------------------------------------------------- fused

def fused_inputs(M, K, C, device):
    g = torch.Generator().manual_seed(7 * M + K + C)
    x = torch.randn(M, K, generator=g).to(device=device, dtype=BF)
    w_t = (torch.randn(K, C, generator=g) * K ** -0.5).to(device=device,
                                                          dtype=BF)
    return x, w_t


@pytest.mark.parametrize("K", [32, 256, 288, 512])
@pytest.mark.parametrize("C", [1, 10, 16])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 65, 300])
def test_fused_metrics(gpu_device, M, C, K):
    e, F = ext(), fn()
    p, t = case(M, C, gpu_device)
    x, w_t = fused_inputs(M, K, C, gpu_device)
    ref = ref_totals(p, t, "xent")
    alone = F.new_metrics_acc(gpu_device)
    F.head_metrics(p, t, alone)
    alone = F.read_metrics_acc(alone)
    check(alone, ref, "standalone")
    for rb in (32, 64):
        dz0, dx0 = e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY, rb)
        for slots in (1, shipped_slots()):
            acc = F.new_metrics_acc(gpu_device, slots=slots)
            dz, dx = e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY,
                                      rb, acc, 0)
            # NaN rows make NaN dz: compare the bits
            assert torch.equal(dz.view(torch.int16), dz0.view(torch.int16))
            assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16))
            got = F.read_metrics_acc(acc)
            check(got, ref, f"fused rb{rb} S{slots}")
            for k in ("correct", "rows", "nonfinite"):
                assert got[k] == alone[k]
    # the `slots` argument narrows a wider accumulator to its first slots
    acc = F.new_metrics_acc(gpu_device, slots=shipped_slots())
    e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY, 0, acc, 1)
    assert not acc[1:].any()
    check(F.read_metrics_acc(acc), ref, "fused slots=1 of S")


@pytest.mark.parametrize("rb", [32, 64])
def test_fused_metrics_with_in_kernel_wgrad(gpu_device, rb):
    """M = 16448: 257 tiles of 64 rows on the 256 blocks the in-kernel
    weight gradient allows, so a block walks more than one tile."""
    e, F = ext(), fn()
    M, K, C = 16448, 32, 10
    p, t = case(M, C, gpu_device)
    x, w_t = fused_inputs(M, K, C, gpu_device)
    ref = ref_totals(p, t, "xent")
    gw0 = torch.zeros(C, K, device=gpu_device)
    gb0 = torch.zeros(C, device=gpu_device)
    dz0, dx0 = e.head_bwd_fused(p, t, x, w_t, float(M), gw0, gb0, rb)
    for slots in (1, shipped_slots()):
        acc = F.new_metrics_acc(gpu_device, slots=slots)
        gw = torch.zeros(C, K, device=gpu_device)
        gb = torch.zeros(C, device=gpu_device)
        dz, dx = e.head_bwd_fused(p, t, x, w_t, float(M), gw, gb, rb, acc, 0)
        assert torch.equal(dz.view(torch.int16), dz0.view(torch.int16))
        assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16))
        check(F.read_metrics_acc(acc), ref, f"wgrad arm rb{rb} S{slots}")


def test_fused_positional_call_unchanged(gpu_device):
    """The pre-metrics call forms still work and count nothing."""
    e = ext()
    M, K, C = 65, 32, 10
    p, t = case(M, C, gpu_device)
    x, w_t = fused_inputs(M, K, C, gpu_device)
    a = e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY)
    b = e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY, 32)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    with pytest.raises(RuntimeError):
        bad = torch.zeros(3, 4, dtype=torch.int32, device=gpu_device)
        e.head_bwd_fused(p, t, x, w_t, float(M), EMPTY, EMPTY, 0, bad, 0)


# -------------------------------------------------------------- worker

SIZES = [784, 64, 10]
B, MUB = 256, 64


@pytest.fixture
def flags():
    F = fn()
    yield F
    F.set_head_fused(True)
    F.set_head_metrics_fused(True)


def make_worker(device, loss="xent", metrics=True):
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.models import MLP, SGD
    from shallowspeed_amd.parallel import Topology, Worker

    model = MLP(SIZES, 0, 1, B, loss=loss).materialize_device(device)
    opt = SGD(model.parameters(), lr=0.0)  # every step sees the same model
    ds = Dataset(B, MUB, n_samples=2 * B, in_dim=SIZES[0],
                 n_classes=SIZES[-1], device=device).load(0, 1)
    topo = Topology(device=device)
    return Worker(topo, model, ds, opt, metrics=metrics), model, ds, topo


def output_buffer_totals(model, ds, topo, kind):
    """Standalone kernel on the output buffer of an inference pass over
    batch 0, taken in one µbatch."""
    from shallowspeed_amd.data import Dataset
    from shallowspeed_amd.parallel import InferenceSchedule, Worker

    F = fn()
    full = Dataset(B, B, n_samples=2 * B, in_dim=SIZES[0],
                   n_classes=SIZES[-1], device=topo.device).load(0, 1)
    vw = Worker(topo, model, full, None, use_dp=False)
    assert vw.read_metrics() is None  # no optimizer: does not count
    model.eval()
    vw.execute(InferenceSchedule(1, 1, 0), 0)
    model.train()
    probs, target = vw._out_bufs[0], full.micro_batch_target(0, 0)
    acc = F.new_metrics_acc(topo.device)
    F.head_metrics(probs, target, acc, kind)
    return F.read_metrics_acc(acc), ref_totals(probs, target, kind)


def test_worker_eager_and_graphed(gpu_device, flags):
    from shallowspeed_amd.parallel import NaiveParallelSchedule

    w, model, ds, topo = make_worker(gpu_device)
    alone, ref = output_buffer_totals(model, ds, topo, "xent")
    check(alone, ref, "output buffer")
    sched = NaiveParallelSchedule(ds.num_mubatches(), 1, 0)
    w.execute(sched, 0)
    got = w.read_metrics()
    check(got, ref, "eager batch")
    assert got["rows"] == B and got["correct"] == alone["correct"]
    assert got["acc"] == got["correct"] / B
    assert abs(got["loss"] - got["loss_sum"] / B) < 1e-12
    assert w.read_metrics()["rows"] == 0

    w.execute_graphed(sched, 0)  # eager warm-up, capture, first replay
    assert all(isinstance(g, torch.cuda.CUDAGraph)
               for g in w._graphs.values()), "capture fell back to eager"
    w.read_metrics(reset=True)
    for _ in range(3):
        w.execute_graphed(sched, 0)
    got = w.read_metrics()
    check(got, ref, "3 graph replays", scale=3)
    assert got["rows"] == 3 * B and got["correct"] == 3 * alone["correct"]

    # turning metrics off drops the captured graphs and stops counting
    w.set_metrics(False)
    assert w._graphs == {} and w.read_metrics() is None
    assert model.layers[-1]._metrics is None


def test_worker_metrics_default_off(gpu_device, monkeypatch):
    monkeypatch.delenv("SS_TRAIN_METRICS", raising=False)
    w, model, ds, topo = make_worker(gpu_device, metrics=None)
    assert w._metrics_acc is None and w.read_metrics() is None
    monkeypatch.setenv("SS_TRAIN_METRICS", "1")
    w, model, ds, topo = make_worker(gpu_device, metrics=None)
    assert w._metrics_acc is not None


@pytest.mark.parametrize("path", ["unfused", "standalone_launch", "mse"])
def test_other_head_paths_count_the_same(gpu_device, flags, path):
    from shallowspeed_amd.parallel import NaiveParallelSchedule

    F = flags
    w, model, ds, topo = make_worker(gpu_device)
    sched = NaiveParallelSchedule(ds.num_mubatches(), 1, 0)
    w.execute(sched, 0)
    fused = w.read_metrics()
    kind = "xent"
    if path == "unfused":
        F.set_head_fused(False)
    elif path == "standalone_launch":
        F.set_head_metrics_fused(False)
    else:
        kind = "mse"
    w2, model2, ds2, topo2 = make_worker(gpu_device, loss=kind)
    alone, ref = output_buffer_totals(model2, ds2, topo2, kind)
    w2.execute(sched, 0)
    got = w2.read_metrics()
    check(got, ref, path)
    for k in ("correct", "rows", "nonfinite"):
        assert got[k] == fused[k], (path, k)
