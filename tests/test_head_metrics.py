"""Training metrics on the CPU path: the metric definition
(F.head_metrics / new_metrics_acc / read_metrics_acc), the loss heads and
Worker.read_metrics, DP over gloo, and the train.py epoch line.

The functional tests compare with float64 from the same tensors.  The
CPU path takes each row's terms and their sum in f32 (C - 1 additions,
at most 3 roundings per term), sums the rows in f64 and rounds twice
more on the way into the f32 accumulator word, hence

    |got - ref| <= (C + 16) * 2^-24 * sum|row_loss|.
"""

import os
import random
import re
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from shallowspeed_amd.data import Dataset
from shallowspeed_amd.models import MLP, SGD
from shallowspeed_amd.ops import functional as F
from shallowspeed_amd.parallel import (
    GPipeSchedule,
    NaiveParallelSchedule,
    Topology,
    Worker,
)

ROOT = __file__.rsplit("/tests/", 1)[0]
FLT_MIN = 1.1754943508222875e-38


def ref_totals(p, t, kind):
    p, t = p.double(), t.double()
    M, C = p.shape
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
                bound=(C + 16) * 2.0 ** -24 * row.abs().sum().item())


def make_case(M, C, special):
    g = torch.Generator().manual_seed(100 * M + C)
    p = torch.softmax(torch.randn(M, C, generator=g) * 2.0, dim=1)
    lab = torch.randint(0, C, (M,), generator=g)
    t = torch.zeros(M, C)
    t[torch.arange(M), lab] = 1
    if special:
        assert M >= 5
        p[0, :] = 0.5               # tied maxima: the lower index wins
        t[0, :] = 0
        t[0, 1] = 1                 # ... so naming column 1 is wrong
        p[1, :] = 0.5
        t[1, :] = 0
        t[1, 0] = 1                 # ... and naming column 0 is right
        p[2, lab[2]] = 0.0          # zero prob under the 1
        p[3, C - 1] = float("nan")
        p[4, 0] = float("inf")
        if M > 5:
            p[5, 0] = float("-inf")
    return p, t


@pytest.mark.parametrize("kind", ["xent", "mse"])
@pytest.mark.parametrize("C", [2, 10, 17])
@pytest.mark.parametrize("M", [1, 7, 300])
def test_functional_matches_f64(M, C, kind):
    p, t = make_case(M, C, special=M >= 5)
    ref = ref_totals(p, t, kind)
    acc = F.new_metrics_acc("cpu")
    assert acc.shape == (1, 4) and acc.dtype == torch.int32
    F.head_metrics(p, t, acc, kind)
    got = F.read_metrics_acc(acc, reset=False)
    for k in ("correct", "rows", "nonfinite"):
        assert got[k] == ref[k], (k, got, ref)
    assert abs(got["loss_sum"] - ref["loss_sum"]) <= ref["bound"], (got, ref)
    if M >= 5:
        assert got["nonfinite"] == (3 if M > 5 else 2)
    # a second call adds; a read with reset zeroes
    F.head_metrics(p, t, acc, kind)
    twice = F.read_metrics_acc(acc, reset=True)
    assert twice["rows"] == 2 * M and twice["correct"] == 2 * ref["correct"]
    assert abs(twice["loss_sum"] - 2 * ref["loss_sum"]) <= 2 * ref["bound"] \
        + 2.0 ** -23 * 2 * abs(ref["loss_sum"])
    assert F.read_metrics_acc(acc) == dict(loss_sum=0.0, correct=0, rows=0,
                                           nonfinite=0)


def test_special_rows_one_by_one():
    p, t = make_case(7, 10, special=True)

    def one(r, kind="xent"):
        acc = F.new_metrics_acc("cpu")
        F.head_metrics(p[r:r + 1], t[r:r + 1], acc, kind)
        return F.read_metrics_acc(acc)

    assert one(0)["correct"] == 0 and one(1)["correct"] == 1
    zero = one(2)
    assert zero["nonfinite"] == 0
    assert zero["loss_sum"] == pytest.approx(87.33654475, rel=1e-6)
    for r in (3, 4, 5):
        for kind in ("xent", "mse"):
            assert one(r, kind) == dict(loss_sum=0.0, correct=0, rows=1,
                                        nonfinite=1)


def test_multi_slot_accumulator_folds():
    acc = F.new_metrics_acc("cpu", slots=4)
    assert acc.shape == (4, 4)
    acc[:, 1] = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    acc.view(torch.float32)[:, 0] = torch.tensor([0.5, 0.25, 1.0, 2.0])
    got = F.read_metrics_acc(acc)
    assert got["correct"] == 10 and got["loss_sum"] == 3.75
    with pytest.raises(AssertionError):
        F.new_metrics_acc("cpu", slots=3)


# -------------------------------------------------------- layers / worker

SIZES = [784, 32, 10]
GBS = 64


def make_worker(loss, mub, metrics=True, lr=0.05, sizes=SIZES, topo=None,
                stage=0, n_stages=1):
    model = MLP(sizes, stage, n_stages, GBS, loss=loss).materialize_device(
        "cpu")
    opt = SGD(model.parameters(), lr=lr)
    ds = Dataset(GBS, mub, n_samples=2 * GBS, in_dim=sizes[0],
                 n_classes=sizes[-1]).load(0, 1)
    w = Worker(topo or Topology(), model, ds, opt, metrics=metrics)
    return w, model, ds


def manual_totals(model, ds, loss, batch=0):
    lo = batch * ds.local_batch_size
    x = ds.x[lo:lo + ds.local_batch_size]
    y = ds.y[lo:lo + ds.local_batch_size]
    model.eval()
    probs = model.forward(x, 0)
    model.train()
    fn = F.xent_loss if loss == "xent" else F.mse_loss
    return (float(fn(probs, y, probs.shape[0])),
            int((probs.argmax(-1) == y.argmax(-1)).sum()))


@pytest.mark.parametrize("loss", ["xent", "mse"])
def test_worker_read_metrics(loss):
    w, model, ds = make_worker(loss, mub=GBS)
    want_loss, want_correct = manual_totals(model, ds, loss)
    w.execute(NaiveParallelSchedule(1, 1, 0), 0)
    m = w.read_metrics()
    assert m["rows"] == GBS and m["nonfinite"] == 0
    assert m["correct"] == want_correct
    assert m["acc"] == want_correct / GBS
    assert m["loss"] == pytest.approx(want_loss, rel=1e-5)
    assert m["loss"] == pytest.approx(m["loss_sum"] / GBS)
    again = w.read_metrics()
    assert again["rows"] == 0 and again["correct"] == 0
    assert again["loss_sum"] == 0.0 and again["nonfinite"] == 0

    # the same batch in 4 µbatches
    w4, model4, ds4 = make_worker(loss, mub=GBS // 4)
    w4.execute(GPipeSchedule(4, 1, 0), 0)
    m4 = w4.read_metrics()
    assert m4["rows"] == GBS and m4["correct"] == want_correct
    assert m4["loss_sum"] == pytest.approx(m["loss_sum"], rel=1e-5)


def test_metrics_off_and_eval_count_nothing(monkeypatch):
    monkeypatch.delenv("SS_TRAIN_METRICS", raising=False)
    w, model, ds = make_worker("xent", mub=GBS, metrics=None)
    assert w.read_metrics() is None and model.layers[-1]._metrics is None
    monkeypatch.setenv("SS_TRAIN_METRICS", "1")
    w, model, ds = make_worker("xent", mub=GBS, metrics=None)
    assert model.layers[-1]._metrics is w._metrics_acc is not None
    w.execute(NaiveParallelSchedule(1, 1, 0), 0)
    assert w.read_metrics(reset=False)["rows"] == GBS
    assert w.read_metrics(reset=False)["rows"] == GBS  # reset=False keeps
    w.set_metrics(False)
    assert w.read_metrics() is None and model.layers[-1]._metrics is None
    # a worker without an optimizer (validation) never counts
    vw = Worker(Topology(), model, ds, None, metrics=True)
    assert vw.read_metrics() is None


def test_non_last_stage_returns_none():
    sizes = [784, 32, 16, 10]
    topo = Topology(rank=0, world=2, pp=2)
    w, model, ds = make_worker("xent", mub=GBS, sizes=sizes, topo=topo,
                               stage=0, n_stages=2)
    assert topo.stage_id == 0
    assert w._metrics_acc is None and w.read_metrics() is None


# ------------------------------------------------------------- DP (gloo)

def _dp_metrics(rank, world, out_dir):
    from shallowspeed_amd.parallel import init_topology

    topo = init_topology(dp=world, pp=1, backend="gloo",
                         device=torch.device("cpu"))
    model = MLP(SIZES, 0, 1, GBS, loss="xent").materialize_device("cpu")
    opt = SGD(model.parameters(), lr=0.05)
    ds = Dataset(GBS, GBS // world // 2, n_samples=2 * GBS, in_dim=SIZES[0],
                 n_classes=SIZES[-1]).load(topo.dp_rank, world)
    w = Worker(topo, model, ds, opt, metrics=True)
    w.execute(GPipeSchedule(ds.num_mubatches(), 1, 0), 0)
    m = w.read_metrics()
    torch.save(m, os.path.join(out_dir, f"metrics_{rank}.pt"))
    torch.distributed.destroy_process_group()


def _dist_entry(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    _dp_metrics(rank, world, out_dir)


def test_dp2_totals_match_serial(tmp_path):
    mp.spawn(_dist_entry,
             args=(2, random.randint(20000, 45000), str(tmp_path)),
             nprocs=2, join=True)
    got = [torch.load(tmp_path / f"metrics_{r}.pt", weights_only=False)
           for r in range(2)]
    assert got[0] == got[1]  # every rank holds the reduced totals
    w, model, ds = make_worker("xent", mub=GBS // 4)
    w.execute(GPipeSchedule(4, 1, 0), 0)
    want = w.read_metrics()
    assert got[0]["rows"] == GBS == want["rows"]
    assert got[0]["correct"] == want["correct"]
    assert got[0]["nonfinite"] == 0
    assert got[0]["loss_sum"] == pytest.approx(want["loss_sum"], rel=1e-5)
    assert got[0]["loss"] == pytest.approx(want["loss"], rel=1e-5)


# ------------------------------------------------------------------- CLI

def _train(*extra):
    return subprocess.run(
        [sys.executable, "train.py", "--device", "cpu", "--loss", "xent",
         "--samples", "512", "--global-batch", "64", "--mubatches", "4",
         "--layer-sizes", "784,32,10", *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_cli_epoch_line():
    r = _train("--epochs", "4", "--lr", "0.1")
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert len(re.findall(r"val_acc=([0-9.]+)", out)) == 4 + 1
    lines = [l for l in out.splitlines() if l.startswith("epoch")]
    assert len(lines) == 4
    num = r"([-+0-9.eE]+|nan|inf)"
    tl, vl, ta = [], [], []
    for l in lines:
        m = re.search(rf"val_acc={num}\s+val_loss={num}\s+train_loss={num}"
                      rf"\s+train_acc={num}\s+time=", l)
        assert m, l
        vl.append(float(m.group(2)))
        tl.append(float(m.group(3)))
        ta.append(float(m.group(4)))
    assert all(v == v and abs(v) != float("inf") for v in tl + vl), out
    assert tl[-1] < tl[0], tl
    assert all(0.0 <= a <= 1.0 for a in ta)
    assert "WARNING" not in out


def test_cli_no_metrics_keeps_val_fields():
    r = _train("--epochs", "2", "--lr", "0.1", "--no-metrics")
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(re.findall(r"val_acc=([0-9.]+)", r.stdout)) == 2 + 1
    assert "val_loss=" in r.stdout and "train_loss=" not in r.stdout


def test_cli_halt_on_nonfinite():
    """A learning rate that overflows the weights in the first step: the
    epoch reports its non-finite rows and the run stops with status 3."""
    r = _train("--epochs", "3", "--lr", "1e30", "--halt-on-nonfinite")
    assert r.returncode == 3, r.stdout + r.stderr
    assert re.search(r"WARNING: \d+ non-finite rows", r.stdout), r.stdout
    assert len([l for l in r.stdout.splitlines()
                if l.startswith("epoch")]) == 1
