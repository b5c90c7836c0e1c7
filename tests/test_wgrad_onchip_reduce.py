"""wgrad_tn with K-groups inside the block: the groups' partial tiles
are summed through LDS and each block issues one set of f32 atomics.

The exact cases use small-integer operands, so every partial sum is
exactly representable in f32 and the result must be BITWISE equal to the
reference whatever the summation order: a dropped or doubled K-slice,
K-group, fragment or chunk cannot hide in rounding noise.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

# (Kb, Mo, N)
SHAPES = [
    (64, 64, 64),        # one K-step: every K-group but one is empty
    (200, 64, 80),       # K tail + N remainder on the 64-tile path
    (192, 256, 528),     # 128-tile path, N = 4*128 + 16 (the 784 pattern);
                         # unmasked: glds tiles plus a remainder tile
    (1000, 100, 123),    # nothing aligned: element-wise staging
    (4096, 256, 784),    # auto split, flagship first layer at 1/4 batch
    (4096, 256, 256),    # hidden layer
    (4096, 10, 256),     # head
]
SPLITS = [0, 1, 4, 7]

_cache = {}


def _ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def _int_case(dev, shape, masked):
    """Seeded integer operands, integer initial gW/gb and the exact f32
    reference (computed once in f64, shared, never modified)."""
    key = (shape, masked)
    if key not in _cache:
        Kb, Mo, N = shape
        g = torch.Generator().manual_seed(1000 * Kb + 10 * Mo + N + masked)
        dy = torch.randint(-2, 3, (Kb, Mo), generator=g).to(dev)
        x = torch.randint(-2, 3, (Kb, N), generator=g).to(dev)
        mk = torch.randint(-1, 2, (Kb, Mo), generator=g).to(dev)
        w0 = torch.randint(-3, 4, (Mo, N), generator=g).to(dev)
        b0 = torch.randint(-3, 4, (Mo,), generator=g).to(dev)
        dz = dy.double() * (mk > 0) if masked else dy.double()
        ref_w = (dz.t() @ x.double())
        ref_b = dz.sum(0)
        # everything below 2^24: exactly representable in f32
        assert (w0.abs().max() + 2 * ref_w.abs().max()) < 2 ** 24
        _cache[key] = dict(
            dy=dy.bfloat16(), x=x.bfloat16(),
            mask=mk.bfloat16() if masked else torch.Tensor(),
            w0=w0.float(), b0=b0.float(),
            ref_w=ref_w.float(), ref_b=ref_b.float())
    return _cache[key]


@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_cases(gpu_device, shape, masked, split_k):
    c = _int_case(gpu_device, shape, masked)
    gw, gb = c["w0"].clone(), c["b0"].clone()
    _ext().wgrad_tn(c["dy"], c["x"], gw, gb, c["mask"], split_k)
    assert torch.equal(gw, c["w0"] + c["ref_w"])
    assert torch.equal(gb, c["b0"] + c["ref_b"])


@pytest.mark.parametrize("split_k", [0, 1])
@pytest.mark.parametrize("shape", [(200, 64, 80), (192, 256, 528),
                                   (4096, 256, 784)],
                         ids=lambda s: "x".join(map(str, s)))
def test_accumulates_into_the_same_buffers(gpu_device, shape, split_k):
    c = _int_case(gpu_device, shape, True)
    gw, gb = c["w0"].clone(), c["b0"].clone()
    for _ in range(2):
        _ext().wgrad_tn(c["dy"], c["x"], gw, gb, c["mask"], split_k)
    assert torch.equal(gw, c["w0"] + 2 * c["ref_w"])
    assert torch.equal(gb, c["b0"] + 2 * c["ref_b"])


@pytest.mark.parametrize("shape", [(128, 64, 80), (256, 256, 528)],
                         ids=lambda s: "x".join(map(str, s)))
def test_chunk_table_sums_over_chunks(gpu_device, shape):
    from shallowspeed_amd.ops import functional as F

    Kb, Mo, N = shape
    g = torch.Generator().manual_seed(7 + Kb)
    chunks, ref_w, ref_b = [], 0, 0
    for _ in range(3):
        dy = torch.randint(-2, 3, (Kb, Mo), generator=g).to(gpu_device)
        x = torch.randint(-2, 3, (Kb, N), generator=g).to(gpu_device)
        mk = torch.randint(-1, 2, (Kb, Mo), generator=g).to(gpu_device)
        dz = dy.double() * (mk > 0)
        ref_w = ref_w + dz.t() @ x.double()
        ref_b = ref_b + dz.sum(0)
        chunks.append((dy.bfloat16(), x.bfloat16(), mk.bfloat16()))
    w0 = torch.randint(-3, 4, (Mo, N), generator=g).float().to(gpu_device)
    b0 = torch.randint(-3, 4, (Mo,), generator=g).float().to(gpu_device)
    gw, gb = w0.clone(), b0.clone()
    F.linear_wgrad_multi(chunks, gw, gb)
    assert torch.equal(gw, w0 + ref_w.float())
    assert torch.equal(gb, b0 + ref_b.float())


def _normal_case(dev, shape, seed):
    Kb, Mo, N = shape
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(Kb, Mo, generator=g).to(dev).bfloat16()
    x = torch.randn(Kb, N, generator=g).to(dev).bfloat16()
    mk = torch.randn(Kb, Mo, generator=g).to(dev).bfloat16()
    return dy, x, mk


def test_random_normal_matches_f32_reference(gpu_device):
    shape = (4096, 256, 784)
    dy, x, mk = _normal_case(gpu_device, shape, 11)
    dz = dy.float() * (mk.float() > 0)
    ref_w = dz.t() @ x.float()
    ref_b = dz.sum(0)
    gw = torch.zeros(shape[1], shape[2], device=gpu_device)
    gb = torch.zeros(shape[1], device=gpu_device)
    _ext().wgrad_tn(dy, x, gw, gb, mk, 0)
    for got, ref in ((gw, ref_w), (gb, ref_b)):
        torch.testing.assert_close(
            got, ref, atol=1e-2 + 1e-3 * ref.abs().max().item(), rtol=2e-2)


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", [(192, 256, 528), (200, 64, 80)],
                         ids=lambda s: "x".join(map(str, s)))
def test_split_k_1_is_bitwise_reproducible(gpu_device, shape, masked):
    dy, x, mk = _normal_case(gpu_device, shape, 23)
    mask = mk if masked else torch.Tensor()
    outs = []
    for _ in range(2):
        gw = torch.zeros(shape[1], shape[2], device=gpu_device)
        gb = torch.zeros(shape[1], device=gpu_device)
        _ext().wgrad_tn(dy, x, gw, gb, mask, 1)
        outs.append((gw, gb))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
