"""Dropout on the CPU path: the mask function, Linear with dropout
against a torch-autograd twin, serial equivalence under micro-batching,
DP and PP with dropout ON, checkpoint resume and the train.py flags.

The mask is a pure function of (seed, step, layer, sample, column)
(F.dropout_keep_mask, Philox4x32-10), so the serial-equivalence
comparisons run with the tolerances tests/test_distributed_cpu.py uses
for the same comparisons without dropout (rtol 1e-4, atol 1e-5), built
the same way: serial one-µbatch training is the reference."""

import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from shallowspeed_amd.checkpoint import load_checkpoint, save_checkpoint
from shallowspeed_amd.data import Dataset
from shallowspeed_amd.models import MLP, SGD
from shallowspeed_amd.models.layers import Linear
from shallowspeed_amd.ops import functional as F
from shallowspeed_amd.parallel import SCHEDULES, NaiveParallelSchedule, Topology, Worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ mask function

def _philox_hex(counter, key):
    return " ".join(f"{int(w):08x}" for w in F.philox4x32_10(counter, key))


def test_philox_known_answers():
    assert _philox_hex((0, 0, 0, 0), (0, 0)) == \
        "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _philox_hex((ones,) * 4, (ones,) * 2) == \
        "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _philox_hex((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                       (0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


@pytest.mark.parametrize("p, kept", [(0.1, 22097), (0.25, 18358),
                                      (0.5, 12198)])
def test_kept_counts(p, kept):
    m = F.dropout_keep_mask(0x5EED, 3, 1, torch.arange(96), 256, p)
    assert m.shape == (96, 256) and m.dtype == torch.bool
    assert int(m.sum()) == kept


def test_threshold_and_scale():
    assert F.dropout_params(0.0) == (0xFFFFFFFF, 1.0)
    assert F.dropout_params(0.5) == (1 << 31, 2.0)
    thr, scale = F.dropout_params(0.1)
    assert thr == round(0.9 * 2 ** 32)
    assert scale == float(np.float32(1 / 0.9))
    with pytest.raises(ValueError):
        F.dropout_params(1.0)


def test_mask_is_a_function_of_the_sample_only():
    """One block, four µbatch slices and a stride-2 shard give each
    sample the same bits; ragged column counts cut a 4-column group
    without changing the columns that remain."""
    seed, step, layer, p = 0x1234_5678_9ABC_DEF0, 7, 2, 0.25
    ids = torch.arange(64)
    whole = F.dropout_keep_mask(seed, step, layer, ids, 40, p)
    for k in range(4):
        part = F.dropout_keep_mask(seed, step, layer, ids[16 * k:16 * k + 16],
                                   40, p)
        assert torch.equal(part, whole[16 * k:16 * k + 16])
    for r in range(2):
        shard = F.dropout_keep_mask(seed, step, layer, ids[r::2], 40, p)
        assert torch.equal(shard, whole[r::2])
    ragged = F.dropout_keep_mask(seed, step, layer, ids, 33, p)
    assert torch.equal(ragged, whole[:, :33])
    # a high bit of the 64-bit seed is part of the key
    for other in ((seed ^ 1, step, layer), (seed ^ (1 << 40), step, layer),
                  (seed, step + 1, layer), (seed, step, layer + 1)):
        assert not torch.equal(F.dropout_keep_mask(*other, ids, 40, p), whole)
    with pytest.raises(AssertionError):
        F.dropout_keep_mask(seed, step, layer, torch.tensor([1 << 32]), 4, p)


# ------------------------------------------------------------------ Linear

def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_linear_dropout_matches_autograd_twin():
    """f32 forward/backward of Linear(48, 40, relu, dropout=0.25) against
    torch autograd multiplying by the oracle mask·scale (atol = rtol =
    1e-5, the fuzz test's tolerance).  Default state of a hand-driven
    Linear: seed 0, step 0, layer 0, samples 0..M-1."""
    M, p = 33, 0.25
    lin = Linear(48, 40, "relu", dropout=p)
    x = _rand(M, 48, seed=1)
    dout = _rand(M, 40, seed=2)
    y = lin.forward(x, 0)
    dx = lin.backward(dout, 0)

    keep = F.dropout_keep_mask(0, 0, 0, torch.arange(M), 40, p)
    scale = F.dropout_params(p)[1]
    assert 0 < int(keep.sum()) < keep.numel()
    xt = x.clone().requires_grad_(True)
    w = lin.weight.data.clone().requires_grad_(True)
    b = lin.bias.data.clone().requires_grad_(True)
    yt = torch.relu(xt @ w.t() + b) * keep.float() * scale
    yt.backward(dout)
    tol = dict(atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(y, yt.detach(), **tol)
    assert torch.equal(y == 0, ~keep | (yt.detach() == 0))
    torch.testing.assert_close(dx, xt.grad, **tol)
    torch.testing.assert_close(lin.weight.grad, w.grad, **tol)
    torch.testing.assert_close(lin.bias.grad, b.grad, **tol)


def test_linear_eval_and_p0_are_plain():
    x = _rand(17, 48, seed=3)
    dout = _rand(17, 40, seed=4)
    plain = Linear(48, 40, "relu")
    want_y = plain.forward(x, 0)
    want_dx = plain.backward(dout, 0)

    p0 = Linear(48, 40, "relu", dropout=0.0, layer_index=3)
    assert torch.equal(p0.forward(x, 0), want_y)
    assert torch.equal(p0.backward(dout, 0), want_dx)
    assert torch.equal(p0.weight.grad, plain.weight.grad)

    ev = Linear(48, 40, "relu", dropout=0.25)
    ev.eval()
    assert torch.equal(ev.forward(x, 0), want_y)
    ev.train()
    assert not torch.equal(ev.forward(x, 0), want_y)


@pytest.mark.parametrize("activation", [None, "gelu"])
def test_dropout_needs_relu(activation):
    with pytest.raises(ValueError):
        Linear(48, 40, activation, dropout=0.25)
    Linear(48, 40, activation, dropout=0.0)


def test_dropout_range():
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            Linear(48, 40, "relu", dropout=bad)


def test_mlp_places_dropout_and_global_layer_index():
    sizes = [48, 64, 64, 64, 64, 10]
    whole = MLP(sizes, 0, 1, 32, dropout=0.25, dropout_seed=9)
    assert [l.dropout for l in whole.layers[:-1]] == [0.25] * 4 + [0.0]
    assert [l.layer_index for l in whole.layers[:4]] == [0, 1, 2, 3]
    assert whole.dropout_seed == 9 and whole.dropout_step == 0
    assert whole.has_dropout()
    s1 = MLP(sizes, 1, 2, 32, dropout=0.25)
    assert [l.layer_index for l in s1.layers[:2]] == [3, 4]
    assert [l.dropout for l in s1.layers[:2]] == [0.25, 0.0]
    assert not MLP(sizes, 0, 1, 32).has_dropout()


def test_tpmlp_rejects_dropout():
    from shallowspeed_amd.parallel import TPMLP

    with pytest.raises(ValueError, match="dropout"):
        TPMLP([48, 64, 64, 10], None, 0, 1, 32, dropout=0.1)


# ------------------------------------------------------- serial equivalence

SIZES = [48, 64, 64, 64, 10]
# MLP cuts len(sizes) boundaries into equal stages, so two pipeline
# stages need an even count: the PP comparison adds one hidden layer
SIZES_PP = [48, 64, 64, 64, 64, 10]
GBS = 32
STEPS = 3
N = GBS * STEPS
LR = 0.05
P = 0.25
SEED = 0xD0D0_5EED_0000_0001
TOL = dict(rtol=1e-4, atol=1e-5)

_SERIAL = {}


def _train(model, topo, mub, dp_rank, dp, schedule, stage_id=0, pp=1):
    opt = SGD(model.parameters(), lr=LR)
    sizes = SIZES_PP if pp > 1 else SIZES
    ds = Dataset(GBS, mub, n_samples=N, in_dim=sizes[0], n_classes=sizes[-1])
    ds.load(dp_rank, dp)
    w = Worker(topo, model, ds, opt)
    assert ds.num_batches() == STEPS
    for b in range(STEPS):
        w.execute(SCHEDULES[schedule](ds.num_mubatches(), pp, stage_id), b)
    assert model.dropout_step == STEPS
    return [p.data.clone() for p in model.parameters()]


def _serial(sizes=None, dropout=P):
    """Serial reference: one µbatch of the whole batch, computed once
    per configuration and shared (never modified)."""
    sizes = sizes or SIZES
    key = (tuple(sizes), dropout)
    if key not in _SERIAL:
        model = MLP(sizes, 0, 1, GBS, loss="mse", dropout=dropout,
                    dropout_seed=SEED).materialize_device("cpu")
        opt = SGD(model.parameters(), lr=LR)
        ds = Dataset(GBS, GBS, n_samples=N, in_dim=sizes[0],
                     n_classes=sizes[-1]).load(0, 1)
        w = Worker(Topology(), model, ds, opt)
        for b in range(STEPS):
            w.execute(NaiveParallelSchedule(1, 1, 0), b)
        _SERIAL[key] = [p.data.clone() for p in model.parameters()]
    return _SERIAL[key]


def test_dropout_changes_training():
    """The comparisons below are not vacuous: dropout moves the weights
    well outside their tolerance."""
    a, b = _serial(), _serial(dropout=0.0)
    assert max((x - y).abs().max().item() for x, y in zip(a, b)) > 1e-3


@pytest.mark.parametrize("schedule", ["naive", "gpipe", "pipedream"])
def test_four_mubatches_match_serial(schedule):
    model = MLP(SIZES, 0, 1, GBS, loss="mse", dropout=P,
                dropout_seed=SEED).materialize_device("cpu")
    got = _train(model, Topology(), GBS // 4, 0, 1, schedule)
    for g, w in zip(got, _serial()):
        torch.testing.assert_close(g, w, **TOL)


def _dist_entry(rank, world, port, fn_name, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    globals()[fn_name](rank, world, out_dir)


def _run_dist(fn, world, tmp_path):
    port = random.randint(20000, 45000)
    mp.spawn(_dist_entry, args=(world, port, fn.__name__, str(tmp_path)),
             nprocs=world, join=True)


def _dp_train(rank, world, out_dir):
    from shallowspeed_amd.parallel import init_topology
    from shallowspeed_amd.utils import assert_sync, get_model_hash

    topo = init_topology(dp=world, pp=1, backend="gloo",
                         device=torch.device("cpu"))
    model = MLP(SIZES, 0, 1, GBS, loss="mse", dropout=P,
                dropout_seed=SEED).materialize_device("cpu")
    got = _train(model, topo, (GBS // world) // 2, topo.dp_rank, world,
                 "gpipe")
    assert_sync(topo.dp_group, get_model_hash(model))
    if rank == 0:
        torch.save(got, os.path.join(out_dir, "dp_params.pt"))
    torch.distributed.destroy_process_group()


def test_dp2_matches_serial(tmp_path):
    _run_dist(_dp_train, 2, tmp_path)
    got = torch.load(tmp_path / "dp_params.pt", weights_only=False)
    want = _serial()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, **TOL)


def _pp_train(rank, world, out_dir):
    from shallowspeed_amd.parallel import init_topology

    topo = init_topology(dp=1, pp=world, backend="gloo",
                         device=torch.device("cpu"))
    model = MLP(SIZES_PP, topo.stage_id, world, GBS, loss="mse", dropout=P,
                dropout_seed=SEED).materialize_device("cpu")
    got = _train(model, topo, GBS // 4, 0, 1, "gpipe", topo.stage_id, world)
    torch.save(got, os.path.join(out_dir, f"pp_stage{topo.stage_id}.pt"))
    torch.distributed.destroy_process_group()


def test_pp2_matches_serial(tmp_path):
    _run_dist(_pp_train, 2, tmp_path)
    got = []
    for s in range(2):
        got += torch.load(tmp_path / f"pp_stage{s}.pt", weights_only=False)
    want = _serial(SIZES_PP)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, **TOL)


# --------------------------------------------------------------- checkpoint

CK_SIZES = [24, 16, 12, 10]


def _ck_model():
    return MLP(CK_SIZES, 0, 1, 16, dropout=P,
               dropout_seed=77).materialize_device("cpu")


def _ck_ds():
    return Dataset(16, 8, n_samples=64, in_dim=CK_SIZES[0],
                   n_classes=CK_SIZES[-1]).load(0, 1)


def _ck_train(model, opt, ds, batches):
    w = Worker(Topology(), model, ds, opt)
    for b in batches:
        w.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), b)


def test_resume_continues_the_mask_sequence(tmp_path):
    """2 steps, save, resume, 2 steps == 4 straight steps, bit for bit
    (the tolerance of the momentum-resume test)."""
    straight = _ck_model()
    opt_s = SGD(straight.parameters(), lr=0.05, momentum=0.9)
    _ck_train(straight, opt_s, _ck_ds(), [0, 1, 2, 3])

    part1 = _ck_model()
    opt1 = SGD(part1.parameters(), lr=0.05, momentum=0.9)
    ds = _ck_ds()
    _ck_train(part1, opt1, ds, [0, 1])
    assert part1.dropout_step == 2
    save_checkpoint(tmp_path, part1, Topology(), step=2, optimizer=opt1)

    # the resumed model is built with ANOTHER seed: the shard's wins
    part2 = MLP(CK_SIZES, 0, 1, 16, dropout=P,
                dropout_seed=1).materialize_device("cpu")
    opt2 = SGD(part2.parameters(), lr=0.05, momentum=0.9)
    load_checkpoint(tmp_path, part2, Topology(), optimizer=opt2)
    assert (part2.dropout_step, part2.dropout_seed) == (2, 77)
    _ck_train(part2, opt2, ds, [2, 3])
    for a, b in zip(straight.parameters(), part2.parameters()):
        torch.testing.assert_close(a.data, b.data, rtol=0, atol=0)

    # without the counter the run would have replayed steps 0 and 1
    part3 = _ck_model()
    opt3 = SGD(part3.parameters(), lr=0.05, momentum=0.9)
    load_checkpoint(tmp_path, part3, Topology(), optimizer=opt3)
    part3.dropout_step = 0
    _ck_train(part3, opt3, ds, [2, 3])
    assert any((a.data != b.data).any()
               for a, b in zip(straight.parameters(), part3.parameters()))


def test_old_format_shard_loads_as_step_zero(tmp_path):
    model = _ck_model()
    model.dropout_step = 5
    save_checkpoint(tmp_path, model, Topology(), step=5)
    shard = os.path.join(tmp_path, "stage_00.pt")
    state = torch.load(shard, weights_only=False)
    assert state.pop("dropout") == {"seed": 77, "step": 5}
    torch.save(state, shard)
    fresh = _ck_model()
    fresh.dropout_step = 3
    load_checkpoint(tmp_path, fresh, Topology())
    assert (fresh.dropout_step, fresh.dropout_seed) == (0, 77)


# ---------------------------------------------------------------------- CLI

def _cli(*extra):
    return subprocess.run(
        [sys.executable, "train.py", "--device", "cpu", "--loss", "xent",
         "--samples", "256", "--global-batch", "64", "--mubatches", "2",
         "--layer-sizes", "784,32,32,10", *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_cli_dropout_runs_and_echoes():
    r = _cli("--dropout", "0.2", "--dropout-seed", "5", "--epochs", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"dropout=0\.2 dropout_seed=5", r.stdout), r.stdout
    assert "final val_acc=" in r.stdout


def test_cli_default_does_not_mention_dropout():
    r = _cli("--epochs", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dropout" not in r.stdout


def test_cli_rejects_dropout_with_tp():
    r = _cli("--tp", "2", "--dropout", "0.2", "--epochs", "1")
    assert r.returncode == 2, r.stdout + r.stderr
    assert "--dropout" in r.stderr and "usage" in r.stderr
