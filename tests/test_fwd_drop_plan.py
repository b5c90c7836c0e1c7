"""Sequential._fwd_drop_plan: which layers the forward chain under
dropout takes.  Pure layer configuration — runs without a GPU."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.ops import functional as F

# headed, first layer from a stored tile, and a headless pipeline stage
MODELS = [([784, 256, 256, 256, 10], 1), ([256, 256, 256, 10], 1),
          ([784, 256, 256, 256, 256, 10], 2), ([784, 300, 256, 10], 1)]


@pytest.fixture(autouse=True)
def flags():
    saved = (F._FWD_CHAIN, F._FWD_CHAIN_L1, F._FWD_CHAIN_DROPOUT)
    F.set_fwd_chain(True)
    F._FWD_CHAIN_L1 = True
    F.set_head_fused(True)
    yield
    F._FWD_CHAIN, F._FWD_CHAIN_L1, F._FWD_CHAIN_DROPOUT = saved


@pytest.mark.parametrize("sizes,n_stages", MODELS)
def test_plan_is_the_plain_models_when_switched_on(sizes, n_stages):
    plain = MLP(sizes, 0, n_stages, 64)
    want = plain._fwd_chain_plan() if n_stages == 1 \
        else plain._fwd_stage_plan()
    assert (want is None) == (sizes[1] == 300)
    drop = MLP(sizes, 0, n_stages, 64, dropout=0.25)
    for on in (False, True):
        F.set_fwd_chain_dropout(on)
        assert drop._fwd_drop_plan() == (want if on else None)
        assert drop._fwd_chain_plan() is None
        assert drop._fwd_stage_plan() is None


def test_no_plan_with_an_fp8_layer_or_the_chain_off():
    F.set_fwd_chain_dropout(True)
    m = MLP(MODELS[0][0], 0, 1, 64, dropout=0.25)
    assert m._fwd_drop_plan() == [0, 1, 2]
    m.layers[1].fp8_fwd = True
    assert m._fwd_drop_plan() is None
    m.layers[1].fp8_fwd = False
    F.set_fwd_chain(False)
    assert m._fwd_drop_plan() is None
