"""Sequential._fwd_chain_plan: which layers the forward chain kernel
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
    saved = (F._FWD_CHAIN, F._FWD_CHAIN_L1)
    F.set_fwd_chain(True)
    F._FWD_CHAIN_L1 = False
    F.set_head_fused(True)
    yield
    F._FWD_CHAIN, F._FWD_CHAIN_L1 = saved
    F.set_head_fused(True)


def test_flagship_plan():
    """The 784-wide first layer stays its own launch; with the streamed
    first layer switched on the chain takes it too."""
    m = MLP(FLAGSHIP, 0, 1, 16384)
    assert m._fwd_chain_plan() == [1, 2]
    F._FWD_CHAIN_L1 = True
    assert m._fwd_chain_plan() == [0, 1, 2]


def test_chain_covers_only_the_layers_above_another_width():
    m = MLP([784, 300, 256, 10], 0, 1, 64)
    assert m._fwd_chain_plan() is None  # 300 -> 256 is not in the chain
    F._FWD_CHAIN_L1 = True
    # 300 % 8 != 0: still not streamed
    assert m._fwd_chain_plan() is None
    m = MLP([784, 304, 256, 256, 10], 0, 1, 64)
    assert m._fwd_chain_plan() == [1, 2]    # 304 -> 256 streamed
    F._FWD_CHAIN_L1 = False
    assert m._fwd_chain_plan() == [2]
    m = MLP([784, 300, 256, 256, 10], 0, 1, 64)
    assert m._fwd_chain_plan() == [2]
    # the head's input is 256 wide but the layer under it is not
    assert MLP([784, 256, 512, 10], 0, 1, 64)._fwd_chain_plan() is None
    assert MLP([784, 128, 128, 10], 0, 1, 64)._fwd_chain_plan() is None


def test_dropout_model_has_no_plan():
    assert MLP(FLAGSHIP, 0, 1, 64, dropout=0.1)._fwd_chain_plan() is None
    # dropout on a layer below the chain does not matter
    below = Sequential([Linear(784, 512, "relu", dropout=0.1),
                        Linear(512, 256, "relu"), Linear(256, 256, "relu"),
                        Linear(256, 10), SoftmaxXent(64)])
    assert below._fwd_chain_plan() == [2]


def test_gelu_or_layernorm_under_the_head():
    under_head = Sequential([Linear(48, 256, "relu"),
                             Linear(256, 256, "gelu"), Linear(256, 10),
                             SoftmaxXent(64)])
    assert under_head._fwd_chain_plan() is None
    gelu = Sequential([Linear(48, 256, "gelu"), Linear(256, 256, "relu"),
                       Linear(256, 256, "relu"), Linear(256, 10),
                       SoftmaxXent(64)])
    assert gelu._fwd_chain_plan() == [1, 2]
    ln = Sequential([Linear(48, 256, "relu"), LayerNorm(256),
                     Linear(256, 256, "relu"), Linear(256, 10),
                     SoftmaxXent(64)])
    assert ln._fwd_chain_plan() == [2]


def test_mse_head_has_no_plan():
    assert MLP(FLAGSHIP, 0, 1, 64, loss="mse")._fwd_chain_plan() is None


def test_pp2_stage_slices():
    """bench.py --pp 2 pads the sizes to an even count; stage 0 has no
    head, stage 1 is Linear(256,256,relu) -> head."""
    sizes = [784, 256, 256, 256, 256, 10]
    assert MLP(sizes, 0, 2, 64)._fwd_chain_plan() is None
    assert MLP(sizes, 1, 2, 64)._fwd_chain_plan() == [0]


def test_at_most_eight_layers():
    m = MLP([256] * 10 + [10], 0, 1, 64)  # nine 256-wide ReLU layers
    assert m._fwd_chain_plan() == list(range(1, 9))


def test_switches():
    m = MLP(FLAGSHIP, 0, 1, 64)
    F.set_fwd_chain(False)
    assert m._fwd_chain_plan() is None
    F.set_fwd_chain(True)
    F.set_head_fused(False)
    assert m._fwd_chain_plan() is None
    F.set_head_fused(True)
    m.layers[2].fp8_fwd = True
    assert m._fwd_chain_plan() is None
    m.layers[2].fp8_fwd = False
    assert m._fwd_chain_plan() == [1, 2]

    class NoFuse(MLP):
        _fuse_head = False  # as TPMLP

    assert NoFuse(FLAGSHIP, 0, 1, 64)._fwd_chain_plan() is None


def test_cpu_forward_is_unchanged(monkeypatch):
    """On the CPU the plan exists but the chain op is never called, and
    the forward is the per-layer torch path."""
    def boom(*a, **k):
        raise AssertionError("fwd_chain called on the CPU")

    x = torch.zeros(8, 256)
    assert F.fwd_chain(x, [x], [x[0]], x, x[0]) is None  # CPU tensors
    monkeypatch.setattr(F, "fwd_chain", boom)
    m = MLP([24, 256, 256, 10], 0, 1, 8).materialize_device("cpu")
    assert m._fwd_chain_plan() == [1]
    x = torch.randn(8, 24, generator=torch.Generator().manual_seed(1))
    probs = m.forward(x, 0)
    h = x
    for lin in m.layers[:2]:
        h = torch.clamp(h @ lin.weight.data.t() + lin.bias.data, min=0)
    z = h @ m.layers[2].weight.data.t() + m.layers[2].bias.data
    assert torch.equal(probs, F.softmax_fwd(z))
    assert [sorted(k for k, _ in l._cache) for l in m.layers] == \
        [["x", "y"], ["x", "y"], ["x"], ["s"]]
    F.set_fwd_chain(False)
    assert torch.equal(m.forward(x, 0), probs)
