"""wgrad_tn with two LDS staging sets (stages=2): the loads of K-step
t+1 are issued into the other set under the MFMAs of step t, with one
block barrier per step.

The staging depth changes WHEN loads are issued, never what is summed
or in which order, so:

* on small-integer operands (every partial sum exact in f32) the result
  is BITWISE equal to the f64 reference whatever the split — a K-step
  read from the wrong set, read before it landed or overwritten while it
  was still being read cannot hide in rounding noise;
* on normal data the single-owner path (split_k = 1, one K-group, K
  summed in order) is BITWISE equal to the one-set kernel.

Operands and references are those of test_wgrad_onchip_reduce (computed
once, shared, never modified), plus shapes whose K-step counts hit the
two-set loop's edges.
"""

import pytest
import torch

from test_wgrad_onchip_reduce import SHAPES, SPLITS, _int_case, _normal_case

pytestmark = pytest.mark.gpu

# (Kb, Mo, N) beyond SHAPES
EXTRA_SHAPES = [
    (128, 64, 80),       # one K-step per group at KG = 2: nothing to prefetch
    (328, 256, 256),     # six steps, the last a K tail, in the 64-tile form
    (264, 10, 256),      # head: Mo no multiple of 8, odd step count
    (448, 256, 528),     # 128-tile form, seven steps: the groups' trip
                         # counts differ and every set is reused
]


def _ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_two_sets_exact_integer_cases(gpu_device, shape, masked, split_k):
    c = _int_case(gpu_device, shape, masked)
    gw, gb = c["w0"].clone(), c["b0"].clone()
    _ext().wgrad_tn(c["dy"], c["x"], gw, gb, c["mask"], split_k, 2)
    assert torch.equal(gw, c["w0"] + c["ref_w"])
    assert torch.equal(gb, c["b0"] + c["ref_b"])


@pytest.mark.parametrize("shape", [(200, 64, 80), (192, 256, 528),
                                   (4096, 256, 784)],
                         ids=lambda s: "x".join(map(str, s)))
def test_two_sets_accumulate_into_the_same_buffers(gpu_device, shape):
    c = _int_case(gpu_device, shape, False)
    gw, gb = c["w0"].clone(), c["b0"].clone()
    for _ in range(2):
        _ext().wgrad_tn(c["dy"], c["x"], gw, gb, c["mask"], 0, 2)
    assert torch.equal(gw, c["w0"] + 2 * c["ref_w"])
    assert torch.equal(gb, c["b0"] + 2 * c["ref_b"])


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", [(192, 256, 528), (200, 64, 80),
                                   (1000, 100, 123), (4096, 256, 256)],
                         ids=lambda s: "x".join(map(str, s)))
def test_split_k_1_bitwise_equal_to_one_set(gpu_device, shape, masked):
    dy, x, mk = _normal_case(gpu_device, shape, 23)
    mask = mk if masked else torch.Tensor()
    outs = []
    for stages in (1, 2):
        gw = torch.zeros(shape[1], shape[2], device=gpu_device)
        gb = torch.zeros(shape[1], device=gpu_device)
        _ext().wgrad_tn(dy, x, gw, gb, mask, 1, stages)
        outs.append((gw, gb))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


def test_stages_argument_is_checked(gpu_device):
    c = _int_case(gpu_device, (64, 64, 64), False)
    gw, gb = c["w0"].clone(), c["b0"].clone()
    with pytest.raises(RuntimeError):
        _ext().wgrad_tn(c["dy"], c["x"], gw, gb, c["mask"], 0, 3)
    assert torch.equal(gw, c["w0"]) and torch.equal(gb, c["b0"])
