"""LoadMuBatchTarget hands the backward a zero-copy view of the dataset
slice when dtype and device already match (mirrors the input side); a
later receive into the same grad-in buffer index drops the view."""

import torch

from shallowspeed_amd.data import Dataset
from shallowspeed_amd.models import MLP, SGD
from shallowspeed_amd.parallel import NaiveParallelSchedule, Topology, Worker
from shallowspeed_amd.parallel import comm as comm_mod
from shallowspeed_amd.parallel.instructions import (
    BackwardGradAcc,
    Forward,
    LoadMuBatchInput,
    LoadMuBatchTarget,
    RecvOutputGrad,
)

SIZES = [20, 16, 12, 10]


def _worker():
    model = MLP(SIZES, 0, 1, 32, loss="xent").materialize_device("cpu")
    ds = Dataset(32, 8, n_samples=64, in_dim=SIZES[0], n_classes=SIZES[-1],
                 seed=3).load(0, 1)
    w = Worker(Topology(), model, ds, SGD(model.parameters(), lr=0.05))
    # one full step sets up buffers and the per-batch state
    w.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), 0)
    return w, model, ds


def _spy_backward(model):
    seen = []
    real = model.backward

    def spy(dout, mubatch_id=0):
        seen.append(dout)
        return real(dout, mubatch_id)

    model.backward = spy
    return seen


def test_load_target_is_zero_copy_view():
    w, model, ds = _worker()
    seen = _spy_backward(model)
    w._batch_id = 1
    w._load_input(LoadMuBatchInput(2, 0))
    w._load_target(LoadMuBatchTarget(2, 0))
    w._forward(Forward(2, 0, 0))
    w._backward_acc(BackwardGradAcc(2, 0, 0))
    want = ds.micro_batch_target(1, 2)
    assert len(seen) == 1
    assert seen[0].data_ptr() == want.data_ptr()
    assert seen[0].shape == want.shape
    assert torch.equal(seen[0], want)
    # no copy was made into the staging buffer's storage either
    assert seen[0].data_ptr() != w._gin_bufs[0].data_ptr()


def test_recv_output_grad_drops_the_view(monkeypatch):
    w, model, ds = _worker()
    seen = _spy_backward(model)
    w._batch_id = 0
    w._load_input(LoadMuBatchInput(1, 0))
    w._load_target(LoadMuBatchTarget(1, 0))
    assert 0 in w._gin_views

    incoming = ds.micro_batch_target(1, 3).clone()

    def fake_recv(buf, src):
        buf.copy_(incoming)

    monkeypatch.setattr(comm_mod, "recv_tensor", fake_recv)
    w._recv_output_grad(RecvOutputGrad(1, 0))
    w._forward(Forward(1, 0, 0))
    w._backward_acc(BackwardGradAcc(1, 0, 0))
    assert seen[0].data_ptr() == w._gin_bufs[0].data_ptr()
    assert torch.equal(seen[0], incoming)


def test_training_result_unchanged_by_the_view():
    """The view feeds the same values as the former staging copy: two
    workers, one forced through the copy path, end with equal weights."""
    wa, ma, ds = _worker()
    wb, mb, _ = _worker()

    def copy_load(cmd):
        y = wb.dataset.micro_batch_target(wb._batch_id, cmd.mubatch_id)
        wb._gin_views.pop(cmd.buffer_idx, None)
        wb._gin_bufs[cmd.buffer_idx].copy_(y)

    wb._DISPATCH[LoadMuBatchTarget] = copy_load
    for b in range(ds.num_batches()):
        wa.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), b)
        wb.execute(NaiveParallelSchedule(ds.num_mubatches(), 1, 0), b)
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p.data, q.data)
