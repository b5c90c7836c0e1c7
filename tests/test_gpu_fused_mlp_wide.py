"""The wide fused serving forward (csrc/fused_mlp_wide.hip through
F.fused_mlp_forward) against float64 on the CPU, from the same bf16
tensors:

    h = bf16(relu(h W^T + b)) per hidden layer ;  logits = h W^T + b

    |logits - ref| <= (H + 16) 2^-24 (|h_ref| |W|^T + |b|) + F

The first term is an f32 sum of H products in any order.  F covers
isolated one-step differences in the bf16 rounding of a hidden activation
(f32 and f64 on different sides of a tie); it is measured on the eager
chain, not derived: profiles/r19_fused_mlp_wide.md.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# twice the eager chain's (F.linear_fwd) largest deviation from ref over
# CASES, at (512, 130, 36, 8, 16): profiles/r19_fused_mlp_wide.md, "F"
F_TIE = 2 * 0.002469250001013279

# (H, M, in_dim, nhidden, cout)
CASES = [(128, 1, 16, 1, 1), (128, 65, 100, 2, 10), (256, 63, 784, 3, 10),
         (256, 64, 100, 1, 16), (512, 64, 784, 2, 10), (512, 130, 36, 8, 16),
         (1024, 33, 784, 2, 10), (1024, 129, 1024, 1, 3)]


@functools.lru_cache(maxsize=None)
def inputs(H, M, in_dim, nhidden, cout):
    """Seeded CPU bf16 (x, ws, bs): weights N(0,1)/sqrt(in), biases of
    scale 0.5."""
    g = torch.Generator().manual_seed(H + M + in_dim + nhidden + cout)
    dims = [in_dim] + [H] * nhidden + [cout]
    x = torch.randn(M, in_dim, generator=g).bfloat16()
    ws = [(torch.randn(o, i, generator=g) / i ** 0.5).bfloat16()
          for i, o in zip(dims, dims[1:])]
    bs = [(0.5 * torch.randn(o, generator=g)).bfloat16() for o in dims[1:]]
    return x, ws, bs


@functools.lru_cache(maxsize=None)
def reference(*case):
    """(float64 logits, |h_ref| |W|^T + |b| of the head)."""
    x, ws, bs = inputs(*case)
    h = x.double()
    for w, b in zip(ws[:-1], bs[:-1]):
        h = torch.relu(h @ w.double().t() + b.double()).bfloat16().double()
    w, b = ws[-1].double(), bs[-1].double()
    return h @ w.t() + b, h.abs() @ w.abs().t() + b.abs()


def on(dev, case):
    x, ws, bs = inputs(*case)
    return x.to(dev), [w.to(dev) for w in ws], [b.to(dev) for b in bs]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_logits_and_argmax(gpu_device, case):
    from shallowspeed_amd.ops import functional as F

    ref, mag = reference(*case)
    bound = (case[0] + 16) * 2.0 ** -24 * mag + F_TIE
    # the shipped arm, then every arm built for this width
    for rows, waves in ((0, 0),) + F.FUSED_MLP_ARMS[case[0]]:
        amax, z = F.fused_mlp_forward(*on(gpu_device, case), logits=True,
                                      rows=rows, waves=waves)
        amax, z = amax.cpu(), z.cpu()
        assert amax.dtype == torch.int32 and z.dtype == torch.float32
        assert z.shape == (case[1], case[4])
        assert torch.equal(amax.long(), z.argmax(1))  # the first maximum
        err = (z.double() - ref).abs()
        print(case, rows, waves, "max err", err.max().item(),
              "max excess over the derived term",
              (err - bound + F_TIE).max().item())
        assert (err <= bound).all()
    amax = F.fused_mlp_forward(*on(gpu_device, case), logits=True)[0].cpu()
    # without logits: the same argmax (H = 256, M % 64 == 0: the old kernel)
    only = F.fused_mlp_forward(*on(gpu_device, case))
    if not (case[0] == 256 and case[1] % 64 == 0):
        assert torch.equal(only.cpu(), amax)


def test_argmax_takes_lowest_of_equal_maxima(gpu_device):
    from shallowspeed_amd.ops import functional as F

    x, ws, bs = on(gpu_device, (128, 37, 16, 1, 16))
    ws[-1].zero_()                      # logits = head bias alone
    bs[-1].copy_(torch.tensor([1., 3, 3, 0, 3] + [2.] * 11))
    amax, z = F.fused_mlp_forward(x, ws, bs, logits=True)
    assert (amax == 1).all() and (z[:, 1] == 3).all()


@pytest.mark.parametrize("bad", ["H320", "cout17", "cpu", "nhidden9"])
def test_refusals(gpu_device, bad):
    from shallowspeed_amd.ops import functional as F
    from shallowspeed_amd.ops import load_ext

    case = {"H320": (320, 8, 16, 1, 10), "cout17": (128, 8, 16, 1, 17),
            "cpu": (128, 8, 16, 1, 10), "nhidden9": (128, 8, 16, 9, 10)}[bad]
    x, ws, bs = on("cpu" if bad == "cpu" else gpu_device, case)
    assert F.fused_mlp_forward(x, ws, bs) is None
    assert F.fused_mlp_forward(x, ws, bs, logits=True) is None
    with pytest.raises(RuntimeError):
        load_ext(required=True).fused_mlp_fwd(x, ws, bs, True)


@pytest.mark.parametrize("sizes,batch", [([784, 512, 512, 10], 96),
                                         ([100, 128, 10], 96),
                                         ([784, 256, 256, 256, 10], 128)])
def test_infer_wiring(gpu_device, sizes, batch):
    import infer
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.ops import functional as F
    from shallowspeed_amd.ops import load_ext

    model = MLP(sizes, 0, 1, batch, loss="xent").materialize_device(gpu_device)
    model.eval()
    fn = infer.fused_forward_fn(model, batch)
    assert fn is not None
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, sizes[0], generator=g).bfloat16().to(gpu_device)
    plan = infer.build_fused_plan(model, batch)
    if sizes[1] == 256:
        want = load_ext(required=True).fused_mlp_argmax(x, *plan)
    else:
        assert plan is None
        ls = [l for l in model.layers if hasattr(l, "weight")]
        want = F.fused_mlp_forward(x, [l.weight.compute() for l in ls],
                                   [l.bias.compute() for l in ls])
    assert torch.equal(fn(x), want)
    _, z = infer.fused_forward_fn(model, batch, scores=True)(x)
    assert z.shape == (batch, sizes[-1]) and z.dtype == torch.float32
