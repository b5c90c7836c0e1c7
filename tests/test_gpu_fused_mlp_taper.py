"""The fused serving forward for hidden widths that differ from layer to
layer (csrc/fused_mlp_taper.hip through F.fused_mlp_forward) against
float64 on the CPU, from the same bf16 tensors:

    h = bf16(relu(h W^T + b)) per hidden layer ;  logits = h W^T + b

    |logits - ref| <= (K_head + 16) 2^-24 (|h_ref| |W|^T + |b|) + F

as tests/test_gpu_fused_mlp_wide.py has it, whose input recipe this file
reuses; and bit for bit against csrc/fused_mlp_wide.hip where the widths
are equal.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# twice the eager per-layer chain's (F.linear_fwd) largest deviation from
# the float64 reference over CASES, at ([256, 1024, 256, 128], 130, 784,
# 10): profiles/r21_fused_mlp_taper.md, "F"
F_TIE_TAPER = 2 * 0.0013570189476013184

# (hidden widths, M, in_dim, cout)
CASES = [((512, 256, 128), 65, 784, 10), ((128, 512, 128), 33, 100, 16),
         ((512, 128, 512), 63, 36, 3), ((1024, 128), 1, 20, 1),
         ((256, 1024, 256, 128), 130, 784, 10),
         ((128, 256, 512, 1024, 512, 256, 128, 128), 64, 16, 16)]
# (H, M, in_dim, nhidden, cout) of test_gpu_fused_mlp_wide.py's CASES
EQUAL = [(256, 63, 784, 3, 10), (512, 130, 36, 2, 16)]


@functools.lru_cache(maxsize=None)
def inputs(widths, M, in_dim, cout):
    """Seeded CPU bf16 (x, ws, bs): weights N(0,1)/sqrt(in), biases of
    scale 0.5."""
    g = torch.Generator().manual_seed(sum(widths) + M + in_dim + cout)
    dims = [in_dim, *widths, cout]
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

    widths = case[0]
    ref, mag = reference(*case)
    bound = (widths[-1] + 16) * 2.0 ** -24 * mag + F_TIE_TAPER
    arms = [a for a in F.FUSED_MLP_TAPER_ARMS[max(widths)]
            if min(widths) // a[1] >= 16]
    assert arms
    # the shipped arm, then every arm these widths can take
    for rows, waves in [(0, 0)] + arms:
        amax, z = F.fused_mlp_forward(*on(gpu_device, case), logits=True,
                                      rows=rows, waves=waves)
        amax, z = amax.cpu(), z.cpu()
        assert amax.dtype == torch.int32 and z.dtype == torch.float32
        assert z.shape == (case[1], case[3])
        assert torch.equal(amax.long(), z.argmax(1))  # the first maximum
        err = (z.double() - ref).abs()
        print(case, rows, waves, "max err", err.max().item(),
              "max excess over the derived term",
              (err - bound + F_TIE_TAPER).max().item())
        assert (err <= bound).all()
        only = F.fused_mlp_forward(*on(gpu_device, case), rows=rows,
                                   waves=waves)
        assert torch.equal(only.cpu(), amax)


@pytest.mark.parametrize("case", EQUAL, ids=lambda c: "-".join(map(str, c)))
def test_equal_widths_give_the_uniform_kernels_bits(gpu_device, case):
    from shallowspeed_amd.ops import functional as F
    from shallowspeed_amd.ops import load_ext

    ext = load_ext(required=True)
    H, M, in_dim, nhidden, cout = case
    x, ws, bs = on(gpu_device, ((H,) * nhidden, M, in_dim, cout))
    amax, z = ext.fused_mlp_fwd(x, ws, bs, True)
    for rows, waves in ((0, 0),) + F.FUSED_MLP_TAPER_ARMS[H]:
        got_amax, got_z = ext.fused_mlp_taper_fwd(x, ws, bs, True, rows, waves)
        assert torch.equal(got_z, z), (rows, waves)
        assert torch.equal(got_amax, amax), (rows, waves)


@pytest.mark.parametrize("bad", ["N320", "N64", "cout17", "nhidden9", "cpu",
                                 "waves16"])
def test_refusals(gpu_device, bad):
    from shallowspeed_amd.ops import functional as F
    from shallowspeed_amd.ops import load_ext

    case = {"N320": ((256, 320, 128), 8, 16, 10),
            "N64": ((256, 64), 8, 16, 10),
            "cout17": ((256, 128), 8, 16, 17),
            "nhidden9": ((256,) + (128,) * 8, 8, 16, 10),
            "cpu": ((256, 128), 8, 16, 10),
            "waves16": ((512, 128), 8, 16, 10)}[bad]
    arm = (64, 16) if bad == "waves16" else (0, 0)
    x, ws, bs = on("cpu" if bad == "cpu" else gpu_device, case)
    assert F.fused_mlp_forward(x, ws, bs, rows=arm[0], waves=arm[1]) is None
    assert F.fused_mlp_forward(x, ws, bs, logits=True, rows=arm[0],
                               waves=arm[1]) is None
    with pytest.raises(RuntimeError):
        load_ext(required=True).fused_mlp_taper_fwd(x, ws, bs, True, *arm)


def test_infer_wiring(gpu_device):
    import infer
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.ops import functional as F

    sizes, batch = [784, 512, 256, 128, 10], 96
    model = MLP(sizes, 0, 1, batch, loss="xent").materialize_device(gpu_device)
    model.eval()
    fn = infer.fused_forward_fn(model, batch)
    assert fn is not None and infer.build_fused_plan(model, batch) is None
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, sizes[0], generator=g).bfloat16().to(gpu_device)
    ls = [l for l in model.layers if hasattr(l, "weight")]
    ws = [l.weight.compute() for l in ls]
    bs = [l.bias.compute() for l in ls]
    assert torch.equal(fn(x), F.fused_mlp_forward(x, ws, bs))
    amax, z = infer.fused_forward_fn(model, batch, scores=True)(x)
    want = F.fused_mlp_forward(x, ws, bs, logits=True)
    assert torch.equal(amax, want[0]) and torch.equal(z, want[1])
