"""Sequential._fwd_wide_stage_plan / _bwd_wide_stage_plan: which layers
the stage arms of the wide chain kernels (H = 128, 512) take in a pipeline
stage with no head.  Pure layer configuration: runs without a GPU."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.models.layers import Linear, Sequential
from shallowspeed_amd.ops import functional as F


@pytest.fixture(autouse=True)
def flags():
    saved = (F._CHAIN_WIDE, F._CHAIN_WIDE_DROPOUT)
    F.set_chain_wide(True)
    F.set_chain_wide_dropout(False)
    yield
    F._CHAIN_WIDE, F._CHAIN_WIDE_DROPOUT = saved


def plans(model, rows=64):
    return model._fwd_wide_stage_plan(rows), model._bwd_wide_stage_plan(rows)


def relu_stack(*dims, **kw):
    return Sequential([Linear(a, b, "relu", **kw)
                       for a, b in zip(dims[:-1], dims[1:])])


@pytest.mark.parametrize("make, fwd, bwd", [
    # stage 0 of --pp 2: the streamed first layer ends both chains
    (lambda: MLP([784, 512, 512, 512, 512, 10], 0, 2, 64), [0, 1, 2],
     [(2, True), (1, True), (0, False)]),
    # a middle stage: every dgrad in the chain, dx returned
    (lambda: MLP([128] * 8 + [10], 1, 3, 64), [0, 1, 2],
     [(2, True), (1, True), (0, True)]),
    (lambda: relu_stack(48, 128, 128), [0, 1], [(1, True), (0, False)]),
    # mixed widths: only the run that ends at the stage's last layer
    (lambda: relu_stack(784, 128, 512, 512), [1, 2], [(2, True), (1, False)]),
    # the eight-layer cap
    (lambda: relu_stack(*[128] * 11), list(range(2, 10)),
     [(i, True) for i in range(9, 1, -1)]),
])
def test_wide_stage_plans(make, fwd, bwd):
    m = make()
    assert plans(m) == (fwd, bwd)
    # the 256 stage plans and the headed wide plans keep these models out
    assert m._fwd_stage_plan() is None and m._bwd_stage_plan(64) is None
    assert m._fwd_wide_plan(64) is None and m._bwd_wide_plan(64) is None


def test_no_wide_stage_plan():
    # a head pair: the headed plans own that stage, and keep their results
    last = MLP([784, 512, 512, 512, 512, 10], 1, 2, 64)
    assert plans(last) == (None, None)
    assert last._fwd_wide_plan(64) == [0]
    assert last._bwd_wide_plan(64) == [(0, True)]
    # a GELU or plain top layer, other widths
    for top in ("gelu", None):
        assert plans(Sequential([Linear(128, 128, "relu"),
                                 Linear(128, 128, top)])) == (None, None)
    for width in (256, 1024):
        assert plans(relu_stack(width, width, width)) == (None, None)
    # an fp8 forward on a planned layer refuses the forward plan
    m = relu_stack(512, 512, 512)
    m.layers[0].fp8_fwd = True
    assert m._fwd_wide_stage_plan(64) is None


def test_dropout_follows_its_switch():
    m = relu_stack(784, 512, 512, dropout=0.25)
    assert plans(m) == (None, None)
    F.set_chain_wide_dropout(True)
    assert plans(m) == ([0, 1], [(1, True), (0, False)])
    # one dz_scale per launch: mixed p keeps the forward plan only
    m.layers[0].dropout = 0.5
    assert plans(m) == ([0, 1], None)


def test_row_threshold_in_auto_mode():
    m512, m128 = relu_stack(784, 512, 512), relu_stack(128, 128)
    F._CHAIN_WIDE = "auto"
    lo = F.CHAIN_WIDE_MIN_ROWS[512]
    assert plans(m512, lo - 1) == (None, None)
    assert plans(m512, lo) == ([0, 1], [(1, True), (0, False)])
    assert plans(m128, 1 << 20) == (None, None)   # 128: on request only
