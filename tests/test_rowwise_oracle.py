"""Every case of tests/test_gpu_rowwise.py through the CPU paths of
ops/functional.py and through plain torch, against the float64 oracle of
tests/rowwise_oracle.py.

This proves without a GPU that the reference path alone stays inside every
bound on every input the GPU tests use, and that the exact cases are exact
before any kernel is involved.  The CPU paths compute in f32; where the
kernel emits bf16 the f32 result is rounded once, as the kernel does."""

import pytest
import torch

import rowwise_oracle as O
from rowwise_oracle import BF


def _functional():
    from shallowspeed_amd.ops import functional as F

    def f(t):
        return t.float()

    def ln_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta):
        dgamma, dbeta = dgamma.clone(), dbeta.clone()
        dx = F.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta)
        return dx, dgamma, dbeta

    return O.Backend(
        softmax_fwd=lambda x: F.softmax_fwd(f(x)).to(BF),
        softmax_bwd=lambda dy, s: F.softmax_bwd(f(dy), f(s)).to(BF),
        head_mse_bwd=lambda s, t, gb:
            F.head_softmax_mse_bwd(f(s), f(t), gb).to(BF),
        head_xent_bwd=lambda s, t, gb:
            F.head_softmax_xent_bwd(f(s), f(t), gb).to(BF),
        row_argmax=F.row_argmax,
        ln_fwd=lambda x, g, b: F.layernorm_fwd(x, g, b, eps=1e-5),
        ln_bwd=ln_bwd,
        relu_fwd=F.relu_fwd,
        relu_bwd=lambda dy, y, scale:
            F.relu_bwd(f(dy), f(y), scale).to(BF),
        gelu_fwd=F.gelu_fwd,
        gelu_bwd=F.gelu_bwd,
    )


def _plain_torch():
    """The same operations spelled with torch's own functions (autograd
    for the backwards) in f32: a second, independent reference path."""
    nnf = torch.nn.functional

    def f(t):
        return t.float()

    def softmax_bwd(dy, s):
        # the Jacobian-vector product of softmax at output s
        sf, dyf = f(s), f(dy)
        return (sf * (dyf - (sf * dyf).sum(dim=1, keepdim=True))).to(BF)

    def head_mse_bwd(s, t, gb):
        sf = f(s).requires_grad_(True)
        # d/ds of sum (t - s)^2 / GB, chained through softmax's Jacobian
        loss = ((f(t) - sf) ** 2).sum() / gb
        g, = torch.autograd.grad(loss, sf)
        sf = sf.detach()
        return (sf * (g - (sf * g).sum(dim=1, keepdim=True))).to(BF)

    def ln_fwd(x, gamma, beta):
        xf = f(x)
        y = nnf.layer_norm(xf, (x.shape[1],), f(gamma), f(beta), eps=1e-5)
        var, mean = torch.var_mean(xf, dim=1, unbiased=False)
        return y.to(BF), mean, torch.rsqrt(var + 1e-5)

    def ln_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta):
        # autograd through the definition with the GIVEN statistics held
        # fixed would not be LayerNorm's gradient; differentiate the op
        # itself and accumulate
        xf = f(x).requires_grad_(True)
        gf = f(gamma).requires_grad_(True)
        bf = torch.zeros(x.shape[1], requires_grad=True)
        y = nnf.layer_norm(xf, (x.shape[1],), gf, bf, eps=1e-5)
        dx, dg, db = torch.autograd.grad(y, (xf, gf, bf), f(dy))
        return dx.to(BF), dgamma + dg, dbeta + db

    def gelu_bwd(dy, z):
        zf = f(z).requires_grad_(True)
        g, = torch.autograd.grad(nnf.gelu(zf, approximate="tanh"), zf, f(dy))
        return g.to(BF)

    return O.Backend(
        softmax_fwd=lambda x: torch.softmax(f(x), dim=1).to(BF),
        softmax_bwd=softmax_bwd,
        head_mse_bwd=head_mse_bwd,
        head_xent_bwd=lambda s, t, gb: ((f(s) - f(t)) / gb).to(BF),
        row_argmax=lambda x: torch.argmax(x, dim=1),
        ln_fwd=ln_fwd,
        ln_bwd=ln_bwd,
        relu_fwd=lambda x: torch.where(x > 0, x, torch.zeros_like(x)),
        relu_bwd=lambda dy, y, scale: torch.where(
            y > 0, (f(dy) * scale).to(BF), torch.zeros_like(dy)),
        gelu_fwd=lambda z: nnf.gelu(f(z), approximate="tanh").to(BF),
        gelu_bwd=gelu_bwd,
    )


_BACKENDS = {"functional": _functional, "torch": _plain_torch}


@pytest.fixture(scope="module", params=sorted(_BACKENDS))
def be(request):
    return _BACKENDS[request.param]()


# ----------------------------------------------------------------- rowwise

@pytest.mark.parametrize("kind,B,C", O.SOFTMAX_CASES)
def test_softmax_fwd(be, kind, B, C):
    O.check_softmax_fwd(be, kind, B, C)


@pytest.mark.parametrize("B,C", O.ROW_GRID)
def test_softmax_bwd(be, B, C):
    O.check_softmax_bwd(be, B, C)


@pytest.mark.parametrize("B,C", O.ROW_GRID)
def test_head_mse_bwd(be, B, C):
    O.check_head_mse_bwd(be, B, C)


@pytest.mark.parametrize("B,C", O.ROW_GRID)
def test_row_argmax(be, B, C):
    O.check_row_argmax(be, O.softmax_input("normal", B, C), f"B{B} C{C}")


@pytest.mark.parametrize("C", O.ARGMAX_TIE_C)
def test_row_argmax_ties(be, C):
    x, what = O.argmax_tie_input(C)
    assert "equal" in what and "across lanes" in what \
        and "last column" in what and (C < 65 or "one lane" in what)
    O.check_row_argmax(be, x, f"ties C{C}")
    assert int(be.row_argmax(x)[0]) == 0  # the all-equal row


@pytest.mark.parametrize("kind,B,C", O.LN_FWD_CASES)
def test_ln_fwd(be, kind, B, C):
    O.check_ln_fwd(be, kind, B, C)


@pytest.mark.parametrize("B,C", O.ROW_GRID)
def test_ln_bwd_dx(be, B, C):
    O.check_ln_bwd_dx(be, B, C)


@pytest.mark.parametrize("B,C", O.LN_DPARAM_SHAPES)
def test_ln_bwd_dparam(be, B, C):
    O.check_ln_bwd_dparam(be, B, C)


# ------------------------------------------------------------------ 8-wide

@pytest.mark.parametrize("n", O.EW_N)
def test_relu_fwd(be, n):
    O.check_relu_fwd(be, n)


@pytest.mark.parametrize("scale", O.RELU_SCALES)
@pytest.mark.parametrize("n", O.EW_N)
def test_relu_bwd(be, n, scale):
    O.check_relu_bwd(be, n, scale)


@pytest.mark.parametrize("n", O.EW_N)
def test_gelu_fwd(be, n):
    O.check_gelu_fwd(be, n)


@pytest.mark.parametrize("n", O.EW_N)
def test_gelu_bwd(be, n):
    O.check_gelu_bwd(be, n)


@pytest.mark.parametrize("n", O.EW_N)
def test_head_xent_bwd(be, n):
    s, t = O.xent_flat_input(n)
    O.check_head_xent_bwd(be, s, t, 3 * n, f"n={n}")


def test_head_xent_bwd_rows(be):
    B, C = O.XENT_ROWS
    assert (B * C) % 8 == 2
    s, t, gb = O.head_input(B, C)
    O.check_head_xent_bwd(be, s, t, gb, f"B{B} C{C}")


# ------------------------------------------------- the oracle's own cases

def test_special_values_are_what_they_say():
    """The bit patterns of the special values, and that the planted cases
    hold them where the 8-wide kernels' vector and tail paths read."""
    m = O.bf16_from_bits(O.RELU_MASK_SPECIALS).float()
    assert m[0] == 0 and m[1] == 0 and torch.signbit(m[1])
    assert m[2] == 2.0 ** -133 and m[3] == -2.0 ** -133   # subnormals
    assert m[4] == 2.0 ** -126 and m[5] == -2.0 ** -126   # normals
    assert m[6] == float("inf") and m[7] == -float("inf")
    assert torch.isnan(m[8]) and m[9] == 1 and m[10] == -1
    x = O.bf16_from_bits(O.RELU_FWD_SPECIALS).float()
    assert not torch.isnan(x).any() and x[4] == 2.0 ** -126 - 2.0 ** -133
    n = O.EW_N[-1]
    assert n % 8 == 5 and n > 2048 * 2048 and O.EW_N[-2] % 8 == 5
    y = O.ew_input("relu_mask", n)
    k = len(O.RELU_MASK_SPECIALS)
    assert torch.isnan(y[:k].float()).sum() == 1
    # the scalar tail (n % 8 elements) holds the last specials, NaN among
    # them; n = 7 is all tail and holds the first seven
    assert torch.isnan(y[n - 5:].float()).sum() == 1
    assert torch.equal(O.bits(y[n - k:]),
                       O.bits(O.bf16_from_bits(O.RELU_MASK_SPECIALS)))
    assert torch.equal(O.bits(O.ew_input("relu_mask", 7)),
                       O.bits(O.bf16_from_bits(O.RELU_MASK_SPECIALS)[:7]))
    z = O.ew_input("gelu_z", n).float()
    assert z[n - 1] == -(2.0 ** 15) and z.abs().max() == 2.0 ** 15


def test_constant_rows_are_constant():
    for C in (777, 3000):
        x = O.ln_input("const", 200, C)
        assert (x == x[:, :1]).all() and (x >= 1).all() and (x < 1024).all()
        s = O.ln_input("step", 200, C)
        d = O.bits(s).int() - O.bits(x).int()
        assert (d.sum(dim=1) == 1).all() and ((d == 0) | (d == 1)).all()
    assert len(torch.unique(O.ln_input("const", 200, 777)[:, 0])) > 100


def test_one_pass_variance_is_outside_the_rstd_bound():
    """The bound must separate the two definitions: E[x^2] - mean^2 in
    f32 (emulated here with plain f32 sums, so a kernel's exact values may
    differ) misses the rstd bound on the large-mean and constant rows."""
    missed = 0
    for kind, B, C in O.LN_SPECIAL:
        x = O.ln_input(kind, B, C)
        xf = x.float()
        mu = xf.sum(dim=1) / C
        var = (xf * xf).sum(dim=1) / C - mu * mu
        rstd = torch.rsqrt(var + 1e-5).double()
        ref = O.ln_fwd_ref(x, *O.ln_params(C))
        bad = ~((rstd - ref["rstd"]).abs() <= ref["rstd_bound"])
        print(f"{kind} B{B} C{C}: one-pass rstd outside the bound on "
              f"{int(bad.sum())} of {B} rows")
        missed += int(bad.sum())
    assert missed > 0
