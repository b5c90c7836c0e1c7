"""Sequential._fwd_wide_plan / _bwd_wide_plan: which layers the wide chain
kernels (H = 128, 512) take.  Pure layer configuration: runs without a
GPU."""

import pytest

from shallowspeed_amd.models import MLP
from shallowspeed_amd.ops import functional as F
from shallowspeed_amd.parallel.tp import TPMLP


@pytest.fixture(autouse=True)
def flags():
    saved = (F._CHAIN_WIDE, F._HEAD_FUSED, F._HEAD_WGRAD_FUSED)
    F.set_chain_wide(True)
    F.set_head_fused(True)
    F.set_head_wgrad_fused(False)
    yield
    F._CHAIN_WIDE, F._HEAD_FUSED, F._HEAD_WGRAD_FUSED = saved


def plans(model, rows=64):
    return model._fwd_wide_plan(), model._bwd_wide_plan(rows)


@pytest.mark.parametrize("sizes, fwd, bwd", [
    # the streamed first layer ends both chains: its dgrad is not in
    ([784, 512, 512, 10], [0, 1], [(1, True), (0, False)]),
    ([40, 128, 128, 128, 10], [0, 1, 2], [(2, True), (1, True), (0, False)]),
    # a first layer of the width itself
    ([128, 128, 10], [0], [(0, True)]),
    # mixed widths: only the run under the head
    ([784, 512, 128, 10], [1], [(1, False)]),
    ([784, 128, 512, 512, 10], [1, 2], [(2, True), (1, False)]),
    # 36 % 8 != 0 is not streamed forward; the backward, which reads no
    # x, still ends with that layer's dz
    ([36, 128, 128, 10], [1], [(1, True), (0, False)]),
])
def test_wide_plans(sizes, fwd, bwd):
    m = MLP(sizes, 0, 1, 64)
    m._skip_input_grad = False
    assert plans(m) == (fwd, bwd)
    # the 256 plans keep these models out
    assert m._fwd_chain_plan() is None and m._bwd_chain_plan(64) is None


def test_skipped_input_grad_ends_the_chain_at_dz():
    m = MLP([128, 128, 10], 0, 1, 64)
    m._skip_input_grad = True
    assert m._bwd_wide_plan(64) == [(0, False)]


@pytest.mark.parametrize("width", [256, 1024, 320])
def test_other_widths_have_no_wide_plan(width):
    assert plans(MLP([784, width, width, 10], 0, 1, 64)) == (None, None)


def test_no_wide_plan():
    sizes = [784, 512, 512, 10]
    assert plans(MLP(sizes, 0, 1, 64, dropout=0.1)) == (None, None)
    assert plans(MLP(sizes, 0, 1, 64, loss="mse")) == (None, None)
    assert plans(TPMLP(sizes, None, 0, 1, 64)) == (None, None)
    m = MLP(sizes, 0, 1, 64)
    assert m._bwd_wide_plan(0) is None
    for switch_off in (lambda: F.set_head_fused(False),
                       lambda: F.set_head_wgrad_fused(True),
                       lambda: F.set_chain_wide(False)):
        F.set_head_fused(True)
        F.set_head_wgrad_fused(False)
        F.set_chain_wide(True)
        assert plans(m) != (None, None)
        switch_off()
        assert plans(m) == (None, None)
