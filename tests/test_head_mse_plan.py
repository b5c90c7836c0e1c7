"""F.set_head_mse_fused: with the switch on, a model that ends in
Linear -> SoftmaxMSE gets every plan its SoftmaxXent twin gets; with it
off (the default), none.  Configuration only: no tensors, no device."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.ops import functional as F
from shallowspeed_amd.parallel.tp import TPMLP

FLAGSHIP = [784, 256, 256, 256, 10]


def plans(m):
    return (m._fwd_chain_plan(), m._fwd_drop_plan(), m._bwd_chain_plan(64),
            m._fwd_wide_plan(), m._bwd_wide_plan(64),
            m._head_pair() is not None)


@pytest.mark.parametrize("sizes,dropout", [
    (FLAGSHIP, 0.0), (FLAGSHIP, 0.25), ([784, 128, 128, 10], 0.0),
    ([784, 512, 512, 10], 0.0)], ids=str)
def test_mse_plans_follow_the_switch(monkeypatch, sizes, dropout):
    monkeypatch.setattr(F, "_HEAD_MSE_FUSED", False)
    monkeypatch.setattr(F, "_CHAIN_WIDE", True)
    monkeypatch.setattr(F, "_FWD_CHAIN_DROPOUT", True)
    xent = plans(MLP(sizes, 0, 1, 64, loss="xent", dropout=dropout))
    assert xent[5] and any(p is not None for p in xent[:5])
    mse = MLP(sizes, 0, 1, 64, loss="mse", dropout=dropout)
    assert plans(mse) == (None,) * 5 + (False,)
    F.set_head_mse_fused(True)
    assert F.head_mse_fused() is True
    assert plans(mse) == xent
    assert plans(TPMLP(sizes, None, 0, 1, 64, loss="mse")) == \
        (None,) * 5 + (False,)
    F.set_head_mse_fused(False)
    assert plans(mse) == (None,) * 5 + (False,)


def test_default_off_and_environment_read_once(monkeypatch):
    monkeypatch.setattr(F, "_HEAD_MSE_FUSED", None)
    monkeypatch.delenv("SS_HEAD_MSE_FUSED", raising=False)
    assert F.head_mse_fused() is False
    monkeypatch.setattr(F, "_HEAD_MSE_FUSED", None)
    monkeypatch.setenv("SS_HEAD_MSE_FUSED", "1")
    assert F.head_mse_fused() is True
    monkeypatch.setenv("SS_HEAD_MSE_FUSED", "0")
    assert F.head_mse_fused() is True
