"""The rowwise kernels (softmax fwd / bwd, head_mse_bwd, row_argmax,
LayerNorm) and the 8-wide elementwise kernels (relu_*, gelu_*,
head_xent_bwd) against the float64 oracle of tests/rowwise_oracle.py, at
the shapes where their structure shows: one wave per row and four rows
per block (B = 1, a partial last block, many blocks; C = 1, below, at and
above the 64 lanes, many strides), the scalar tail and the second
grid-stride pass of the 8-wide kernels, row splits of ln_bwd_dparam that
are unequal or empty, tied maxima, signed zeros, subnormals, Inf and NaN
in the ReLU mask.

The same cases, references and bounds run through the CPU paths in
tests/test_rowwise_oracle.py; the bounds are derived there, not tuned."""

import pytest
import torch

import rowwise_oracle as O
from rowwise_oracle import BF

pytestmark = pytest.mark.gpu


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


@pytest.fixture(scope="module")
def be(gpu_device):
    from shallowspeed_amd.ops import functional as F

    ext()

    def d(t):
        return t.to(gpu_device)

    def ln_fwd(x, gamma, beta):
        return tuple(t.cpu() for t in
                     F.layernorm_fwd(d(x), d(gamma), d(beta), eps=1e-5))

    def ln_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta):
        dgamma, dbeta = d(dgamma.clone()), d(dbeta.clone())
        dx = F.layernorm_bwd(d(dy), d(x), d(gamma), d(mean), d(rstd),
                             dgamma, dbeta)
        return dx.cpu(), dgamma.cpu(), dbeta.cpu()

    return O.Backend(
        softmax_fwd=lambda x: F.softmax_fwd(d(x)).cpu(),
        softmax_bwd=lambda dy, s: F.softmax_bwd(d(dy), d(s)).cpu(),
        head_mse_bwd=lambda s, t, gb:
            F.head_softmax_mse_bwd(d(s), d(t), gb).cpu(),
        head_xent_bwd=lambda s, t, gb:
            F.head_softmax_xent_bwd(d(s), d(t), gb).cpu(),
        row_argmax=lambda x: F.row_argmax(d(x)).cpu(),
        ln_fwd=ln_fwd,
        ln_bwd=ln_bwd,
        relu_fwd=lambda x: F.relu_fwd(d(x)).cpu(),
        relu_bwd=lambda dy, y, scale: F.relu_bwd(d(dy), d(y), scale).cpu(),
        gelu_fwd=lambda z: F.gelu_fwd(d(z)).cpu(),
        gelu_bwd=lambda dy, z: F.gelu_bwd(d(dy), d(z)).cpu(),
    )


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
    """Lowest index wins: all-equal rows, ties inside one lane's stride,
    across lanes (the lower index in the higher and in the lower lane) and
    with the last column.  NaN rows are outside the contract."""
    x, _ = O.argmax_tie_input(C)
    O.check_row_argmax(be, x, f"ties C{C}")
    assert int(be.row_argmax(x)[0]) == 0  # the all-equal row


@pytest.mark.parametrize("kind,B,C", O.LN_FWD_CASES)
def test_ln_fwd(be, kind, B, C):
    """y, mean and rstd each against float64 and its own bound.

    The constant rows, the rows one bf16 step from constant and rstd on
    the large-mean rows fail against a one-pass variance
    (E[x^2] - mean^2 in f32: NaN or an rstd off by up to 100 % there);
    the kernel takes the variance about the mean."""
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
    """Bitwise: x where x > 0 (subnormals and +Inf kept), else +0."""
    O.check_relu_fwd(be, n)


@pytest.mark.parametrize("scale", O.RELU_SCALES)
@pytest.mark.parametrize("n", O.EW_N)
def test_relu_bwd(be, n, scale):
    """Bitwise against the CPU rule with +0, -0.0, subnormals, the
    smallest normals, +-Inf and NaN in the mask source."""
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
    s, t, gb = O.head_input(B, C)
    O.check_head_xent_bwd(be, s, t, gb, f"B{B} C{C}")


# --------------------------------------------- nothing behind the last one

_PAD = 64
_SENTINEL = -7.5


def _ew_ops(n, dev):
    """name -> (call(out), expected bf16 on the CPU or None) for every
    8-wide kernel at n elements."""
    e = ext()
    x = O.ew_input("relu_x", n)
    dy, y = O.ew_input("dy", n), O.ew_input("relu_mask", n)
    z = O.ew_input("gelu_z", n)
    s, t = O.xent_flat_input(n)
    xd, dyd, yd, zd, sd, td = (v.to(dev) for v in (x, dy, y, z, s, t))
    return {
        "relu_fwd": (lambda out: e.relu_fwd(xd, out=out),
                     O.relu_fwd_ref(x)),
        "relu_bwd": (lambda out: e.relu_bwd(dyd, yd, out=out),
                     O.relu_bwd_ref(dy, y, 1.0)),
        "relu_bwd_scaled": (
            lambda out: e.relu_bwd_scaled(dyd, yd, 1.25, out=out),
            O.relu_bwd_ref(dy, y, 1.25)),
        "gelu_fwd": (lambda out: e.gelu_fwd(zd, out=out), None),
        "gelu_bwd": (lambda out: e.gelu_bwd(dyd, zd, out=out), None),
        "head_xent_bwd": (
            lambda out: e.head_xent_bwd(sd, td, float(3 * n), out=out),
            None),
    }


@pytest.mark.parametrize("n", O.EW_N)
def test_ew_writes_exactly_n(gpu_device, n):
    """Each 8-wide kernel writes its n outputs and nothing behind them:
    the output is a view of a buffer whose elements past n hold a
    sentinel before the call and must hold it afterwards.  The written
    part equals the op's ordinary result bit for bit."""
    e = ext()
    for name, (call, want) in _ew_ops(n, gpu_device).items():
        buf = torch.full((n + _PAD,), _SENTINEL, dtype=BF, device=gpu_device)
        fresh = call(None)
        got = call(buf[:n])
        assert got.data_ptr() == buf.data_ptr(), name
        tail = buf[n:].cpu()
        assert torch.equal(O.bits(tail), O.bits(torch.full_like(
            tail, _SENTINEL))), f"{name} n={n} wrote past its output"
        O.check_bits(buf[:n].cpu(), fresh.cpu(), f"{name} n={n} out= vs fresh")
        if want is not None:
            O.check_bits(fresh.cpu(), want, f"{name} n={n}")
    with pytest.raises(RuntimeError):
        e.relu_fwd(O.ew_input("relu_x", n).to(gpu_device),
                   out=torch.empty(n + 1, dtype=BF, device=gpu_device))
