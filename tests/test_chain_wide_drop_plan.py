"""Sequential._fwd_wide_plan / _bwd_wide_plan of a model with dropout:
the plain model's plans with F.set_chain_wide_dropout on, none with it
off.  Pure layer configuration: runs without a GPU."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.ops import functional as F


@pytest.fixture(autouse=True)
def flags():
    names = ("_CHAIN_WIDE", "_CHAIN_WIDE_DROPOUT", "_HEAD_FUSED",
             "_HEAD_WGRAD_FUSED")
    saved = [getattr(F, n) for n in names]
    F.set_chain_wide(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    yield
    for n, v in zip(names, saved):
        setattr(F, n, v)


def plans(model, rows=64):
    return model._fwd_wide_plan(), model._bwd_wide_plan(rows)


@pytest.mark.parametrize("sizes", [[784, 512, 512, 10],
                                   [40, 128, 128, 128, 10], [128, 128, 10]])
def test_dropout_model_plans_follow_the_switch(sizes):
    plain = MLP(sizes, 0, 1, 64)
    drop = MLP(sizes, 0, 1, 64, dropout=0.25)
    drop._skip_input_grad = plain._skip_input_grad = False
    F.set_chain_wide_dropout(True)
    assert F.chain_wide_dropout_enabled()
    assert plans(drop) == plans(plain) != (None, None)
    drop.eval()  # every dz_scale is 1: still one scale
    assert plans(drop) == plans(plain)
    F.set_chain_wide_dropout(False)
    assert plans(drop) == (None, None) != plans(plain)


def test_fp8_layer_and_mixed_p_have_no_plan():
    F.set_chain_wide_dropout(True)
    m = MLP([784, 512, 512, 10], 0, 1, 64, dropout=0.25)
    m._skip_input_grad = False
    m.layers[1].fp8_fwd = True
    assert m._fwd_wide_plan() is None
    m.layers[1].fp8_fwd = False
    # one dz scale per launch: planned layers whose p differ
    m.layers[0].dropout = 0.5
    assert m._fwd_wide_plan() == [0, 1]
    assert m._bwd_wide_plan(64) is None
