"""Sequential._bwd_chain_plan: which layers the backward chain kernel
takes.  Pure layer configuration — runs without a GPU."""

import pytest
import torch

from shallowspeed_amd.models import MLP
from shallowspeed_amd.models.layers import (LayerNorm, Linear, Sequential,
                                            SoftmaxXent)
from shallowspeed_amd.ops import functional as F

FLAGSHIP = [784, 256, 256, 256, 10]


@pytest.fixture(autouse=True)
def flags():
    F.set_bwd_chain(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    yield
    F.set_bwd_chain(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)


def test_flagship_plan():
    """dgrad of L3 and L2 in the chain, L1 mask-only (stage 0 never
    needs dL/d(data))."""
    m = MLP(FLAGSHIP, 0, 1, 16384)
    assert m._bwd_chain_plan(16384) == [(2, True), (1, True), (0, False)]
    assert m._bwd_chain_plan(1) == [(2, True), (1, True), (0, False)]


def test_first_layer_dx_needed_ends_the_chain_the_same_way():
    m = MLP(FLAGSHIP, 0, 1, 64)
    m._skip_input_grad = False  # in_dims 784 != 256: still dz only
    assert m._bwd_chain_plan(64) == [(2, True), (1, True), (0, False)]


def test_pp2_stage_slices():
    """bench.py --pp 2 pads the sizes to an even count; stage 0 has no
    head, stage 1 is Linear(256,256,relu) -> head with its dx needed."""
    sizes = [784, 256, 256, 256, 256, 10]
    s0 = MLP(sizes, 0, 2, 64)
    s1 = MLP(sizes, 1, 2, 64)
    assert s0._bwd_chain_plan(64) is None
    assert [(l.in_dims, l.out_dims) for l in s1.layers[:-1]] == \
        [(256, 256), (256, 10)]
    assert s1._bwd_chain_plan(64) == [(0, True)]


def test_all_256_stage0_skips_the_input_grad():
    m = MLP([256, 256, 256, 10], 0, 1, 64)
    assert m._bwd_chain_plan(64) == [(1, True), (0, False)]


def test_mse_head_has_no_plan():
    assert MLP(FLAGSHIP, 0, 1, 64, loss="mse")._bwd_chain_plan(64) is None


def test_other_widths_have_no_plan():
    assert MLP([784, 1024, 1024, 1024, 10], 0, 1, 64)._bwd_chain_plan(64) \
        is None
    assert MLP([784, 128, 128, 10], 0, 1, 64)._bwd_chain_plan(64) is None
    # the head's input is 256 wide but the layer under it is not
    assert MLP([784, 512, 256, 10], 0, 1, 64)._bwd_chain_plan(64) == \
        [(1, False)]
    assert MLP([784, 256, 512, 10], 0, 1, 64)._bwd_chain_plan(64) is None


def test_gelu_or_layernorm_in_the_run_stops_the_chain_above_it():
    gelu = Sequential([Linear(48, 256, "gelu"), Linear(256, 256, "relu"),
                       Linear(256, 256, "relu"), Linear(256, 10),
                       SoftmaxXent(64)])
    assert gelu._bwd_chain_plan(64) == [(2, True), (1, True)]
    ln = Sequential([Linear(48, 256, "relu"), LayerNorm(256),
                     Linear(256, 256, "relu"), Linear(256, 10),
                     SoftmaxXent(64)])
    assert ln._bwd_chain_plan(64) == [(2, True)]
    under_head = Sequential([Linear(48, 256, "relu"),
                             Linear(256, 256, "gelu"), Linear(256, 10),
                             SoftmaxXent(64)])
    assert under_head._bwd_chain_plan(64) is None


def test_at_most_eight_layers():
    m = MLP([256] * 11 + [10], 0, 1, 64)
    plan = m._bwd_chain_plan(64)
    assert plan == [(i, True) for i in range(9, 1, -1)]


def test_switches():
    m = MLP(FLAGSHIP, 0, 1, 64)
    F.set_bwd_chain(False)
    assert m._bwd_chain_plan(64) is None
    F.set_bwd_chain(True)
    F.set_head_fused(False)
    assert m._bwd_chain_plan(64) is None
    F.set_head_fused(True)
    F.set_head_wgrad_fused(True)
    assert m._bwd_chain_plan(64) is None
    F.set_head_wgrad_fused(False)
    assert m._bwd_chain_plan(64) is not None

    class NoFuse(MLP):
        _fuse_head = False  # as TPMLP

    assert NoFuse(FLAGSHIP, 0, 1, 64)._bwd_chain_plan(64) is None


def test_without_dz_of_the_mask_only_layer(monkeypatch):
    """SS_BWD_CHAIN_DZ1=0, the measured alternative: the chain ends at
    dh of a layer whose dgrad it would not run, unless that layer is
    all the chain would hold."""
    monkeypatch.setattr(F, "_BWD_CHAIN_DZ_LAST", False)
    assert MLP(FLAGSHIP, 0, 1, 64)._bwd_chain_plan(64) == \
        [(2, True), (1, True)]
    assert MLP([784, 512, 256, 10], 0, 1, 64)._bwd_chain_plan(64) == \
        [(1, False)]


def test_cpu_backward_is_todays_path(monkeypatch):
    """On the CPU the plan exists but the chain op is never called."""
    def boom(*a, **k):
        raise AssertionError("bwd_chain called on the CPU")

    monkeypatch.setattr(F, "bwd_chain", boom)
    m = MLP([24, 256, 256, 10], 0, 1, 8).materialize_device("cpu")
    assert m._bwd_chain_plan(8) is not None
    x = torch.randn(8, 24, generator=torch.Generator().manual_seed(1))
    t = torch.zeros(8, 10)
    t[:, 3] = 1
    m.zero_grad()
    m.forward(x, 0)
    m.backward(t, 0)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
