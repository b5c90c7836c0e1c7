"""Sequential._fwd_stage_plan / _bwd_stage_plan: which layers of a
pipeline stage with no loss head the stage arms of the chain kernels
take.  Pure layer configuration — runs without a GPU."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.models.layers import Linear, Sequential
from shallowspeed_amd.ops import functional as F

PP2 = [784, 256, 256, 256, 256, 10]   # the flagship, padded for --pp 2


@pytest.fixture(autouse=True)
def flags():
    saved = (F._FWD_CHAIN, F._FWD_CHAIN_L1, F._BWD_CHAIN)
    F.set_fwd_chain(True)
    F.set_bwd_chain(True)
    F._FWD_CHAIN_L1 = True
    yield
    F._FWD_CHAIN, F._FWD_CHAIN_L1, F._BWD_CHAIN = saved


def plans(m):
    return m._fwd_stage_plan(), m._bwd_stage_plan()


def relu_stack(*dims, **kw):
    return Sequential([Linear(a, b, "relu", **kw)
                       for a, b in zip(dims[:-1], dims[1:])])


def test_pp2_stage0_of_the_padded_flagship():
    """Stage 0 streams its 784-wide input and skips the input gradient,
    so the backward chain ends at the first layer's dz."""
    m = MLP(PP2, 0, 2, 64)
    assert plans(m) == ([0, 1, 2], [(2, True), (1, True), (0, False)])
    F._FWD_CHAIN_L1 = False
    assert m._fwd_stage_plan() == [1, 2]


def test_middle_stage_returns_dx():
    m = MLP([256] * 8 + [10], 1, 3, 64)
    assert plans(m) == ([0, 1, 2], [(2, True), (1, True), (0, True)])


def test_the_headed_plans_keep_the_last_stage():
    for m in (MLP(PP2, 1, 2, 64), MLP(PP2[1:], 0, 1, 64)):
        assert m._head_pair() is not None and plans(m) == (None, None)
        assert m._fwd_chain_plan() and m._bwd_chain_plan()
    # and the stage plans change nothing about the headed ones
    assert MLP(PP2, 0, 2, 64)._fwd_chain_plan() is None
    assert MLP(PP2, 0, 2, 64)._bwd_chain_plan() is None


def test_at_most_eight_layers_from_the_top():
    m = relu_stack(*[256] * 11)   # ten layers
    assert m._fwd_stage_plan() == list(range(2, 10))
    assert m._bwd_stage_plan() == [(i, True) for i in range(9, 1, -1)]


def test_other_layers_in_or_under_the_run():
    # a 48-wide input under the run: streamed forward; backward the chain
    # ends at that layer's dz and its ordinary dgrad follows
    m = relu_stack(48, 256, 256)
    assert plans(m) == ([0, 1], [(1, True), (0, False)])
    # 300 is no multiple of 8, 512 is no chain width
    assert plans(relu_stack(300, 256, 256)) == ([1], [(1, True), (0, False)])
    assert plans(relu_stack(256, 512, 256)) == ([1], [(1, False)])
    # the run must end at the stage's last layer
    assert plans(relu_stack(256, 256, 128)) == (None, None)
    gelu_top = Sequential([Linear(256, 256, "relu"),
                           Linear(256, 256, "gelu")])
    assert plans(gelu_top) == (None, None)
    linear_top = Sequential([Linear(256, 256, "relu"), Linear(256, 256)])
    assert plans(linear_top) == (None, None)


def test_dropout_and_fp8():
    """No forward plan over a dropout layer; the backward takes one drop
    probability per launch, as the headed chain."""
    m = MLP(PP2, 0, 2, 64, dropout=0.25)
    assert m._fwd_stage_plan() is None
    assert m._bwd_stage_plan() == [(2, True), (1, True), (0, False)]
    mix = Sequential([Linear(256, 256, "relu", dropout=0.25),
                      Linear(256, 256, "relu", dropout=0.5)])
    assert plans(mix) == (None, None)
    m = MLP(PP2, 0, 2, 64)
    m.layers[1].fp8_fwd = True
    assert m._fwd_stage_plan() is None
    assert m._bwd_stage_plan() is not None


def test_switches_are_the_headed_ones():
    m = MLP(PP2, 0, 2, 64)
    F.set_fwd_chain(False)
    assert plans(m) == (None, [(2, True), (1, True), (0, False)])
    F.set_fwd_chain(True)
    F.set_bwd_chain(False)
    assert plans(m) == ([0, 1, 2], None)
    F.set_bwd_chain(True)
    # the head switches do not matter to a stage without a head
    F.set_head_fused(False)
    F.set_head_wgrad_fused(True)
    try:
        assert plans(m) == ([0, 1, 2], [(2, True), (1, True), (0, False)])
    finally:
        F.set_head_fused(True)
        F.set_head_wgrad_fused(False)
