"""Float64 references, derived error bounds and the shared cases for the
rowwise kernels (csrc/elementwise.hip: softmax fwd / bwd, head_mse_bwd,
row_argmax; csrc/norm.hip: LayerNorm) and the 8-wide elementwise kernels
(relu_*, gelu_*, head_xent_bwd).

A plain helper module (no tests, no fixtures).  tests/test_rowwise_oracle.py
runs every case through the CPU paths of ops/functional.py,
tests/test_gpu_rowwise.py through the HIP kernels; both hand this module a
`Backend` of callables that take and return CPU tensors, so the two suites
see the same tensors, the same references and the same bounds.

References are float64, computed on the CPU from the SAME bf16 tensors the
kernel reads.  No bound below comes from the code under test:

  u   = 2^-24  unit roundoff of f32 (one rounding: |fl(a) - a| <= u |a|)
  2^-8         half a bf16 grid step, relative, at worst

* A bf16 output that is ONE rounding of an f32 value v:
      |got - ref| <= 2^-8 |ref| + slack,
  slack = the error of v itself, written out per operation below.
* An f32 sum of n terms taken in ANY order (lane-strided partials, a xor
  tree, atomics): at most n - 1 roundings, each of a partial sum that is
  <= sum|term|, so to first order
      |fl(sum) - sum| <= (n + 16) u sum|term| ;
  the 16 pays for the roundings inside each term and of the few
  operations around the sum (every use below needs fewer).
* f32 results below the smallest normal 2^-126 may be flushed to zero, so
  every bound carries an absolute floor of that size.
* Exact outputs (relu, argmax, integer sums, softmax of equal rows) are
  compared bit for bit.
"""

import functools
from collections import namedtuple

import torch

BF = torch.bfloat16
U = 2.0 ** -24
HALF_BF = 2.0 ** -8
FLOOR = 2.0 ** -126

# eps as the f32 the kernel receives
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))

ROW_B = (1, 5, 257)
ROW_C = (1, 9, 63, 64, 65, 777)
EW_N = (1, 7, 8, 9, 2048 * 3 + 5, 2048 * 2048 + 2048 * 3 + 13)

# Callables on CPU tensors (bf16 unless said otherwise), returning CPU
# tensors:
#   softmax_fwd(x) softmax_bwd(dy, s) head_mse_bwd(s, t, gb)
#   head_xent_bwd(s, t, gb) row_argmax(x) -> int64
#   ln_fwd(x, gamma, beta) -> (y, mean f32, rstd f32)
#   ln_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta) -> dx, accumulating
#       into copies of dgamma / dbeta that it returns: (dx, dgamma, dbeta)
#   relu_fwd(x) relu_bwd(dy, y, scale) gelu_fwd(z) gelu_bwd(dy, z)
Backend = namedtuple("Backend", [
    "softmax_fwd", "softmax_bwd", "head_mse_bwd", "head_xent_bwd",
    "row_argmax", "ln_fwd", "ln_bwd", "relu_fwd", "relu_bwd", "gelu_fwd",
    "gelu_bwd"])


# ------------------------------------------------------------ comparison

def bf16_bound(ref, slack):
    """Bound on a bf16 output that is one rounding of an f32 value whose
    own error is `slack`."""
    return HALF_BF * ref.abs() + slack


def sum_bound(n, abs_sum):
    """f32 sum of n terms in any order; abs_sum = sum|term|."""
    return (n + 16) * U * abs_sum


def check(got, ref, bound, what):
    """Every element of `got` finite and within `bound` of `ref`; prints
    the worst error and the worst error / bound before it asserts."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    finite = torch.isfinite(got)
    err = torch.where(finite, (got - ref).abs(),
                      torch.full_like(ref, float("inf")))
    ok = err <= bound
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    print(f"{what}: max err {err.max().item():.3e}  worst err/bound "
          f"{ratio.max().item():.3f}  non-finite {int((~finite).sum())}  "
          f"outside {int((~ok).sum())} of {ok.numel()}")
    assert finite.all(), f"{what}: {int((~finite).sum())} non-finite outputs"
    if not ok.all():
        i = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(
            f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound; "
            f"worst at flat index {i}: got {got.flatten()[i].item()!r} ref "
            f"{ref.flatten()[i].item()!r} err {err.flatten()[i].item():.3e} "
            f"bound {bound.flatten()[i].item():.3e}")


def bits(t):
    """The raw bits of a bf16 / f32 tensor, for sign-of-zero comparisons."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def check_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (what, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = bits(got), bits(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.numel()} of {gb.numel()} elements differ in bits; "
            f"first at flat index {i}: got {got.flatten()[i].item()!r} "
            f"(0x{int(gb.flatten()[i]) & 0xffff:04x}) want "
            f"{want.flatten()[i].item()!r} "
            f"(0x{int(wb.flatten()[i]) & 0xffff:04x})")


def bf16_from_bits(words):
    """bf16 tensor from 16-bit patterns given as ints in [0, 0xffff]."""
    w = [v - 0x10000 if v >= 0x8000 else v for v in words]
    return torch.tensor(w, dtype=torch.int16).view(BF)


def gen(*key):
    """A generator seeded by the case's name and shape (hash() of a str
    is salted per process, so names are spelled out as integers)."""
    seed = 0
    for k in key:
        if isinstance(k, str):
            k = sum((i + 1) * ord(ch) for i, ch in enumerate(k))
        seed = (seed * 1000003 + int(k)) % (1 << 31)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- softmax

SOFTMAX_KINDS = ("normal", "pm300", "dominant", "equal", "below_-1e30")


@functools.lru_cache(maxsize=None)
def softmax_input(kind, B, C):
    g = gen("softmax", kind, B, C)
    if kind == "normal":
        x = torch.randn(B, C, generator=g) * 2.0
    elif kind == "pm300":
        # exp(300) overflows f32: only the row-max subtraction saves it
        sign = (torch.rand(B, C, generator=g) < 0.5).float() * 2 - 1
        x = 300.0 * sign + torch.randn(B, C, generator=g)
    elif kind == "dominant":
        x = torch.randn(B, C, generator=g)
        col = torch.randint(0, C, (B,), generator=g)
        x[torch.arange(B), col] += 60.0
    elif kind == "equal":
        x = (torch.randn(B, 1, generator=g) * 8.0).expand(B, C).contiguous()
    elif kind == "below_-1e30":
        # finite rows wholly below -1e30: a running max that starts at a
        # finite floor never sees them (a bf16 step here is 2^93 and more,
        # so the softmax is one-hot, or shared among exact ties)
        x = -2e30 * (1.0 + 1e6 * torch.rand(B, C, generator=g))
    else:
        raise KeyError(kind)
    return x.to(BF)


def softmax_ref(x):
    """softmax in f64 and its bound.

    The kernel takes e_c = __expf(x_c - m), S = sum e_c, out = e_c / S.
    x_c - m is one f32 rounding, u|x_c - m|.  __expf(a) is
    exp2(fl(a * log2e)): log2e in f32 (2^-25 relative) and the product's
    rounding put 1.5u|a| on the argument, which is 1.5u|a| relative on the
    result; with the subtraction's u|a| that is 2.5u|a| <= 220u for
    |a| <= 88 (beyond which e_c < 2^-126 and falls under the floor), plus
    one ulp (2u) of the hardware exp2: below 2^-16 = 256u.  S is a sum of
    positive terms each within 2^-16 relative, so S is within 2^-16
    relative of the true sum plus the summation error (C + 16)u; the
    reciprocal and the product are two of those 16 roundings.  In all:
        slack = (2 * 2^-16 + (C + 16) u) |ref| + 2^-125
    (two floors: e_c and the quotient may each be flushed)."""
    ref = torch.softmax(x.double(), dim=1)
    C = x.shape[1]
    slack = (2 * 2.0 ** -16 + (C + 16) * U) * ref + 2 * FLOOR
    return ref, bf16_bound(ref, slack)


def check_softmax_fwd(be, kind, B, C):
    x = softmax_input(kind, B, C)
    got = be.softmax_fwd(x)
    assert got.dtype == BF
    ref, bound = softmax_ref(x)
    check(got, ref, bound, f"softmax_fwd {kind} B{B} C{C}")
    # each output is within 2^-8 relative of a value whose row sums to 1
    # within 2^-15: |rowsum - 1| <= 2^-8 + 2^-15 < C * 2^-9 for C >= 3;
    # C = 1 and equal rows are exact below
    rs = got.double().sum(dim=1)
    print(f"  row sums: max |sum - 1| {(rs - 1).abs().max().item():.3e} "
          f"limit {C * 2.0 ** -9:.3e}")
    assert ((rs - 1).abs() <= C * 2.0 ** -9).all()
    if C == 1:
        check_bits(got, torch.ones(B, 1, dtype=BF), "softmax C=1 is 1.0")
    elif kind == "equal":
        # exp(0) = 1 exactly, S = C exactly, 1 / C correctly rounded in
        # f32, then one rounding to bf16
        want = torch.tensor(1.0 / C, dtype=torch.float64).float().to(BF)
        assert want.item() == torch.tensor(1.0 / C,
                                           dtype=torch.float64).to(BF).item()
        check_bits(got, want.expand(B, C).contiguous(),
                   f"softmax equal rows are bf16(1/{C})")


@functools.lru_cache(maxsize=None)
def softmax_bwd_input(B, C):
    """(dy, s): s the bf16 softmax of the 'normal' logits; rows 1.. of
    B >= 5 take the dominant-column probabilities."""
    g = gen("softmax_bwd", B, C)
    s = torch.softmax(softmax_input("normal", B, C).double(), dim=1)
    if B >= 5:
        s[1] = torch.softmax(softmax_input("dominant", B, C).double(),
                             dim=1)[1]
    dy = torch.randn(B, C, generator=g)
    return dy.to(BF), s.to(BF)


def softmax_bwd_ref(dy, s):
    """dx = s (dy - dot), dot = sum_c s dy.

    s dy is exact in f32 (8 x 8 significant bits).  dot: sum_bound.
    dy - dot and the product with s are one rounding each, u(|dy| + |dot|)
    |s| each; 4 covers both with room.
        slack = |s| ((C + 16) u sum|s dy| + 4u (|dy| + |dot|)) + 2^-126"""
    sd, dyd = s.double(), dy.double()
    C = s.shape[1]
    terms = sd * dyd
    dot = terms.sum(dim=1, keepdim=True)
    ref = sd * (dyd - dot)
    dot_err = sum_bound(C, terms.abs().sum(dim=1, keepdim=True))
    slack = sd.abs() * (dot_err + 4 * U * (dyd.abs() + dot.abs())) + FLOOR
    return ref, bf16_bound(ref, slack)


def check_softmax_bwd(be, B, C):
    dy, s = softmax_bwd_input(B, C)
    got = be.softmax_bwd(dy, s)
    assert got.dtype == BF
    ref, bound = softmax_bwd_ref(dy, s)
    check(got, ref, bound, f"softmax_bwd B{B} C{C}")


@functools.lru_cache(maxsize=None)
def head_input(B, C):
    """(probs, one-hot target, global batch): GB = 3B is no power of two,
    so 1/GB rounds in f32."""
    g = gen("head", B, C)
    _, s = softmax_bwd_input(B, C)
    lab = torch.randint(0, C, (B,), generator=g)
    t = torch.zeros(B, C)
    t[torch.arange(B), lab] = 1
    return s, t.to(BF), 3 * B


def head_mse_bwd_ref(s, t, gb):
    """g = -2 (t - s) / GB ; dz = s (g - dot), dot = sum_c s g.

    g in f32: t - s rounds once, 1/GB is rounded when passed and the
    product rounds: |g_err| <= 4u|g|.  Each term s g adds its own
    rounding (5u in all, inside the 16 of sum_bound).  g - dot and the
    product with s round once each.
        slack = |s| ((C + 16) u sum|s g| + 4u|g| + 4u (|g| + |dot|))
                + 2^-126"""
    sd, td = s.double(), t.double()
    C = s.shape[1]
    g = -2.0 * (td - sd) / gb
    terms = sd * g
    dot = terms.sum(dim=1, keepdim=True)
    ref = sd * (g - dot)
    dot_err = sum_bound(C, terms.abs().sum(dim=1, keepdim=True))
    slack = sd.abs() * (dot_err + 4 * U * g.abs()
                        + 4 * U * (g.abs() + dot.abs())) + FLOOR
    return ref, bf16_bound(ref, slack)


def check_head_mse_bwd(be, B, C):
    s, t, gb = head_input(B, C)
    got = be.head_mse_bwd(s, t, gb)
    assert got.dtype == BF
    ref, bound = head_mse_bwd_ref(s, t, gb)
    check(got, ref, bound, f"head_mse_bwd B{B} C{C}")


def head_xent_bwd_ref(s, t, gb):
    """dz = (s - t) / GB: the subtraction, the rounding of 1/GB and the
    product are three roundings; slack = 4u|ref| + 2^-126."""
    ref = (s.double() - t.double()) / gb
    return ref, bf16_bound(ref, 4 * U * ref.abs() + FLOOR)


# ------------------------------------------------------------- row_argmax

ARGMAX_TIE_C = (10, 65, 777)


@functools.lru_cache(maxsize=None)
def argmax_tie_input(C):
    """Rows of values below 3 with the maximum 5 planted twice (or in
    every column); returns (x, what each row is)."""
    g = gen("argmax", C)
    pairs = [("equal", None)]
    if C > 64:
        pairs += [("one lane", (c, c + 64))
                  for c in (0, 5, C - 65) if c + 64 < C]
        pairs += [("one lane, 3 apart", (c, c + 192))
                  for c in (7,) if c + 192 < C]
    # different lanes, both orders of (lane, index): the lower index in
    # the higher lane and in the lower lane
    pairs += [("across lanes", (2, 9)), ("across lanes", (3, 4))]
    if C > 130:
        pairs += [("across lanes", (67, 130)), ("across lanes", (63, 64)),
                  ("across lanes", (129, 700))]
    pairs += [("last column", (1, C - 1)), ("last column", (C - 2, C - 1)),
              ("last column", (0, C - 1))]
    x = torch.randn(len(pairs), C, generator=g).clamp(max=3.0)
    for r, (_, cols) in enumerate(pairs):
        if cols is None:
            x[r, :] = -1.5
        else:
            x[r, list(cols)] = 5.0
    # rows wholly below -1e30 (finite, the maximum not in column 0), all
    # -Inf (index 0) and -Inf but for one column: a running maximum must
    # start at -Inf, not at a finite floor
    low = -2e30 * (2.0 + torch.rand(3, C, generator=g))
    low[0, C // 2] = -1.5e30
    low[1, :] = -float("inf")
    low[2, :] = -float("inf")
    low[2, C - 3] = -3e38
    what = [p[0] for p in pairs] + ["below -1e30", "all -inf", "one finite"]
    return torch.cat([x, low]).to(BF), what


def check_row_argmax(be, x, what):
    got = be.row_argmax(x)
    want = torch.argmax(x.float(), dim=1)
    assert got.dtype == torch.int64 and got.shape == want.shape
    bad = (got != want).nonzero().flatten()
    print(f"row_argmax {what}: {bad.numel()} of {want.numel()} rows differ")
    assert bad.numel() == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(),
                              want[bad[:8]].tolist())


# -------------------------------------------------------------- layernorm

@functools.lru_cache(maxsize=None)
def ln_params(C):
    g = gen("ln_params", C)
    gamma = 1.0 + 0.25 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    return gamma.to(BF), beta.to(BF)


def _const_values(n, g):
    """u * 2^k, u in [1, 2), k in 0..9, rounded to bf16."""
    u = 1.0 + torch.rand(n, generator=g)
    k = torch.randint(0, 10, (n,), generator=g)
    return (u * 2.0 ** k).to(BF)


# the inputs beyond zero-mean normals: (kind, B, C)
LN_SPECIAL = (
    ("mean100", 5, 777), ("mean300", 5, 777), ("mean1000", 5, 777),
    ("const", 200, 777), ("const", 200, 3000),
    ("step", 200, 777), ("step", 200, 3000),
)
# both sides of the widths at which ln_fwd changes from 4 to 16 registers
# a lane and from registers to re-reading the row
LN_TIER_EDGES = tuple((kind, 5, C) for C in (256, 257, 1024, 1025)
                      for kind in ("zero_mean", "mean1000", "const", "step"))
LN_LARGE_MEAN = {"mean100": (100.0, 0.5), "mean300": (300.0, 2.0),
                 "mean1000": (1000.0, 8.0)}


@functools.lru_cache(maxsize=None)
def ln_input(kind, B, C):
    """x (bf16, B x C) of one LayerNorm case."""
    if kind in ("const", "step"):
        # ONE seeded generator for all constant rows of a width; "step"
        # is the same rows with one element one bf16 step higher
        g = gen("ln_const", C)
        v = _const_values(B, g)
        x = v.reshape(B, 1).expand(B, C).contiguous()
        if kind == "step":
            col = torch.randint(0, C, (B,), generator=g)
            w = x.view(torch.int16)
            w[torch.arange(B), col] += 1  # positive values: next bf16 up
        return x
    g = gen("ln", kind, B, C)
    if kind == "zero_mean":
        x = torch.randn(B, C, generator=g) * 1.5
    else:
        m, sd = LN_LARGE_MEAN[kind]
        x = m + sd * torch.randn(B, C, generator=g)
    return x.to(BF)


def ln_stats_ref(x):
    xd = x.double()
    mu = xd.mean(dim=1)
    var = ((xd - mu[:, None]) ** 2).mean(dim=1)
    return mu, (var + LN_EPS) ** -0.5


def ln_fwd_ref(x, gamma, beta):
    """y = (x - mu) rstd gamma + beta with the two-pass f64 statistics.

    mean: an f32 sum of C terms and one division,
        |mean - mu| <= (C + 16) u sum|x| / C.
    rstd = (var + eps)^-1/2 with var = sum (x - mean)^2 / C about the
    computed mean: a sum of C NON-NEGATIVE terms, each (x - mean)^2 within
    4u relative (the subtraction and the square), so var is within
    (C + 16) u relative; the error of the mean itself moves var by its
    square only (the cross term sums to zero), which is of second order.
    rstd moves by half the relative change of var + eps; rsqrt and the
    additions take the rest of the factor 4 the bound leaves:
        |rstd - ref| <= (C + 16) 2^-23 ref.
    A one-pass var = E[x^2] - mean^2 has an ABSOLUTE error near
    C u mean^2 instead, which this bound refuses once mean^2 is large
    against var + eps.
    y: x_hat gamma + beta takes four f32 roundings on top of rstd's
    error, paid by 2^-20 (|x_hat gamma| + |beta|); the error of the mean,
    held to 2^-21 max|x| (eight f32 ulps of the largest element), enters
    y multiplied by rstd |gamma|:
        slack = 2^-20 (|x_hat gamma| + |beta|)
                + max_c|x| 2^-21 rstd |gamma| + 2^-126."""
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    C = x.shape[1]
    mu, rstd = ln_stats_ref(x)
    xh = (xd - mu[:, None]) * rstd[:, None]
    y = xh * gd + bd
    slack = (2.0 ** -20 * ((xh * gd).abs() + bd.abs())
             + xd.abs().amax(dim=1, keepdim=True) * 2.0 ** -21
             * rstd[:, None] * gd.abs() + FLOOR)
    return dict(
        y=y, y_bound=bf16_bound(y, slack),
        mean=mu, mean_bound=sum_bound(C, xd.abs().sum(dim=1)) / C + FLOOR,
        rstd=rstd, rstd_bound=(C + 16) * 2.0 ** -23 * rstd)


def check_ln_fwd(be, kind, B, C):
    x = ln_input(kind, B, C)
    gamma, beta = ln_params(C)
    y, mean, rstd = be.ln_fwd(x, gamma, beta)
    assert y.dtype == BF and mean.dtype == torch.float32 \
        and rstd.dtype == torch.float32
    assert y.shape == x.shape and mean.shape == (B,) and rstd.shape == (B,)
    ref = ln_fwd_ref(x, gamma, beta)
    if kind == "const" or C == 1:
        # a constant row normalises to zero: the reference y is beta
        assert torch.equal(ref["y"], beta.double().expand(B, C))
    what = f"ln_fwd {kind} B{B} C{C}"
    errors = []
    for name, got in (("mean", mean), ("rstd", rstd), ("y", y)):
        try:
            check(got, ref[name], ref[name + "_bound"], f"{what} {name}")
        except AssertionError as e:  # report all three before failing
            errors.append(str(e))
    assert not errors, "\n".join(errors)


def ln_stats_f32(x):
    """The f64 statistics rounded to f32: what the backward is fed, so a
    forward error can neither mask a backward one nor be blamed on it."""
    mu, rstd = ln_stats_ref(x)
    return mu.float(), rstd.float()


@functools.lru_cache(maxsize=None)
def ln_bwd_dy(B, C):
    return torch.randn(B, C, generator=gen("ln_dy", B, C)).to(BF)


def ln_bwd_dx_ref(dy, x, gamma, mean, rstd):
    """dx = rstd (g - mean_c g - x_hat mean_c (g x_hat)), g = dy gamma,
    x_hat = (x - mean) rstd, from the f32 statistics it is given.

    g is exact in f32.  x_hat: two roundings.  sg = sum g / C and
    sgx = sum g x_hat / C: sum_bound over C (the roundings of x_hat, of
    the product and of the division are inside its 16).  The bracket adds
    x_hat's own error on its third term and two subtractions and one
    product, the factor rstd one more: 8u of the magnitudes covers them.
        slack = rstd ((C + 16) u (sum|g| + |x_hat| sum|g x_hat|) / C
                      + 8u (|g| + |sg| + |x_hat sgx|)) + 2^-126"""
    C = x.shape[1]
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    g = dy.double() * gamma.double()
    xh = (x.double() - mu) * rs
    sg = g.mean(dim=1, keepdim=True)
    sgx = (g * xh).mean(dim=1, keepdim=True)
    ref = rs * (g - sg - xh * sgx)
    sg_err = sum_bound(C, g.abs().sum(dim=1, keepdim=True)) / C
    sgx_err = sum_bound(C, (g * xh).abs().sum(dim=1, keepdim=True)) / C
    slack = rs * (sg_err + xh.abs() * sgx_err
                  + 8 * U * (g.abs() + sg.abs() + (xh * sgx).abs())) + FLOOR
    return ref, bf16_bound(ref, slack)


def check_ln_bwd_dx(be, B, C):
    x = ln_input("zero_mean", B, C)
    gamma, _ = ln_params(C)
    dy = ln_bwd_dy(B, C)
    mean, rstd = ln_stats_f32(x)
    dx, _, _ = be.ln_bwd(dy, x, gamma, mean, rstd,
                         torch.zeros(C), torch.zeros(C))
    assert dx.dtype == BF
    ref, bound = ln_bwd_dx_ref(dy, x, gamma, mean, rstd)
    check(dx, ref, bound, f"ln_bwd_dx B{B} C{C}")


# (B, C): two row splits of unequal length around the 256-column tile,
# one row, and a row split whose trailing blocks own no row
LN_DPARAM_SHAPES = ((65, 255), (65, 256), (65, 257), (1, 257), (32769, 8))


@functools.lru_cache(maxsize=None)
def ln_dparam_input(B, C):
    """(dy with small-integer values, x, dgamma seed, integer dbeta
    seed)."""
    g = gen("ln_dparam", B, C)
    dy = torch.randint(-4, 5, (B, C), generator=g).float().to(BF)
    x = (torch.randn(B, C, generator=g) * 1.5 + 0.5).to(BF)
    dgamma0 = torch.randn(C, generator=g) * 3.0
    dbeta0 = torch.randint(-8, 9, (C,), generator=g).float()
    return dy, x, dgamma0, dbeta0


def check_ln_bwd_dparam(be, B, C):
    """dgamma += sum_r dy x_hat, dbeta += sum_r dy, into accumulators
    that already hold something.

    dbeta: integers of magnitude <= 4 B + 8 < 2^24 are exact in f32 in
    any order: bitwise.  dgamma: an f32 sum of the B terms and the seed in
    any order (partial sums, atomics), each term with x_hat's two
    roundings and the product's inside the 16:
        |got - ref| <= (B + 1 + 16) u (|seed| + sum_r |dy x_hat|)."""
    dy, x, dgamma0, dbeta0 = ln_dparam_input(B, C)
    gamma, _ = ln_params(C)
    mean, rstd = ln_stats_f32(x)
    _, dgamma, dbeta = be.ln_bwd(dy, x, gamma, mean, rstd, dgamma0, dbeta0)
    assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    terms = dy.double() * xh
    ref = dgamma0.double() + terms.sum(dim=0)
    bound = sum_bound(B + 1, dgamma0.double().abs() + terms.abs().sum(dim=0))
    check(dgamma, ref, bound + FLOOR, f"ln_bwd_dparam dgamma B{B} C{C}")
    want = (dbeta0.double() + dy.double().sum(dim=0)).float()
    assert want.abs().max() < 2 ** 24
    check_bits(dbeta, want, f"ln_bwd_dparam dbeta B{B} C{C}")


# ------------------------------------------------------- 8-wide kernels

# mask source of the ReLU backward: +0, -0.0, the smallest subnormal
# (both signs), the smallest normal (both signs), +-Inf, NaN, +-1
RELU_MASK_SPECIALS = (0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080,
                      0x7f80, 0xff80, 0x7fc0, 0x3f80, 0xbf80)
# relu_fwd: the same without NaN (the GPU maps it to +0, the CPU path
# propagates it: documented, not asserted), plus the largest subnormal
RELU_FWD_SPECIALS = (0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f,
                     0x0080, 0x8080, 0x7f80, 0xff80, 0x3f80, 0xbf80)
GELU_SPECIALS = (0.0, -0.0, 1e-3, -1e-3, 6.0, -6.0, 10.0, -10.0, 40.0,
                 -40.0, 300.0, -300.0, 2.0 ** 15, -(2.0 ** 15))


def _plant(x, spec):
    """Specials at the END of x (the scalar tail of an 8-wide kernel when
    n % 8 != 0) and, where there is room, at the start (the vector
    path)."""
    n, k = x.numel(), min(x.numel(), spec.numel())
    x[n - k:] = spec[:k]
    if n >= 2 * spec.numel():
        x[:spec.numel()] = spec
    return x


@functools.lru_cache(maxsize=None)
def ew_input(name, n):
    """bf16 vectors of n elements for the 8-wide kernels."""
    g = gen("ew", name, n)
    x = (torch.randn(n, generator=g) * 2.0).to(BF)
    if name == "relu_x":
        return _plant(x, bf16_from_bits(RELU_FWD_SPECIALS))
    if name == "relu_mask":
        return _plant(x, bf16_from_bits(RELU_MASK_SPECIALS))
    if name == "gelu_z":
        return _plant(x, torch.tensor(GELU_SPECIALS).to(BF))
    if name == "dy":
        if n >= 4:
            x[n // 2] = -0.0  # a kept -0.0 passes through with its sign
        return x
    raise KeyError(name)


def relu_fwd_ref(x):
    """x where x > 0, else +0 (so -0.0 gives +0); NaN is out of scope."""
    return torch.where(x.float() > 0, x, torch.zeros_like(x))


def relu_bwd_ref(dy, y, scale):
    """The CPU rule: dy where y > 0, otherwise +0 — NaN, -0.0 and every
    negative in y mask to +0.  Kept values are dy's own bits, or with a
    scale bf16(f32(dy) * f32(scale)): one IEEE f32 product (the same on
    every machine) rounded once to bf16."""
    kept = dy if scale == 1.0 else \
        (dy.float() * torch.tensor(scale, dtype=torch.float32)).to(BF)
    return torch.where(y.float() > 0, kept, torch.zeros_like(dy))


def check_relu_fwd(be, n):
    x = ew_input("relu_x", n)
    check_bits(be.relu_fwd(x), relu_fwd_ref(x), f"relu_fwd n={n}")


def check_relu_bwd(be, n, scale):
    dy, y = ew_input("dy", n), ew_input("relu_mask", n)
    check_bits(be.relu_bwd(dy, y, scale), relu_bwd_ref(dy, y, scale),
               f"relu_bwd scale={scale} n={n}")


_GELU_C = 0.7978845608028654
_GELU_A = 0.044715
# |tanhf(u_f32) - tanh(u)|: u = c (z + a z^3) takes five f32 roundings
# and two rounded constants, 6u relative, and |u| tanh'(u) <= 0.45 for
# every u, so the argument costs 2.7u; tanhf itself is within 2 ulp of a
# value <= 1 (HIP math API accuracy table).  4.7u, held to 8u.
_TANH_ERR = 8 * U


def gelu_fwd_ref(z):
    """0.5 z (1 + tanh(u)).  1 + tanh cancels for negative z, so the
    error of tanh is ABSOLUTE in the result, 0.5 |z| 8u: that is the
    floor below which values compare absolutely.  The sum and the two
    products round once each, inside the 2^-16 |ref| term.
        slack = 2^-16 |ref| + 0.5 |z| 8u + 2^-126"""
    zd = z.double()
    t = torch.tanh(_GELU_C * (zd + _GELU_A * zd ** 3))
    ref = 0.5 * zd * (1.0 + t)
    slack = 2.0 ** -16 * ref.abs() + 0.5 * zd.abs() * _TANH_ERR + FLOOR
    return ref, bf16_bound(ref, slack)


def gelu_bwd_ref(dy, z):
    """dz = dy grad, grad = 0.5 (1 + t) + 0.5 z (1 - t^2) u'(z),
    u' = c (1 + 3 a z^2).

    With tau the error of t: 0.5 (1 + t) moves by 0.5 tau, 1 - t^2 by
    2 |t| tau + tau^2, so the second term by 0.5 |z| |u'| (2|t| + tau)
    tau; the products and sums of both terms round a handful of times,
    8u of their magnitudes.  Where tanh saturates this is loose (u' is
    huge while the computed 1 - t^2 is 0): it still demands a finite
    value of the right size there.
        slack = |dy| (0.5 tau + 0.5 |z u'| (2|t| + tau) tau
                      + 8u (0.5 (1 + t) + 0.5 |z| (1 - t^2) |u'|))
                + 2^-16 |ref| + 2^-126"""
    zd, dyd = z.double(), dy.double()
    t = torch.tanh(_GELU_C * (zd + _GELU_A * zd ** 3))
    du = _GELU_C * (1.0 + 3.0 * _GELU_A * zd ** 2)
    a, b = 0.5 * (1.0 + t), 0.5 * zd * (1.0 - t * t) * du
    ref = dyd * (a + b)
    tau = _TANH_ERR
    grad_err = (0.5 * tau + 0.5 * (zd * du).abs() * (2 * t.abs() + tau) * tau
                + 8 * U * (a.abs() + b.abs()))
    slack = dyd.abs() * grad_err + 2.0 ** -16 * ref.abs() + FLOOR
    return ref, bf16_bound(ref, slack)


def check_gelu_fwd(be, n):
    z = ew_input("gelu_z", n)
    got = be.gelu_fwd(z)
    assert got.dtype == BF
    ref, bound = gelu_fwd_ref(z)
    check(got, ref, bound, f"gelu_fwd n={n}")


def check_gelu_bwd(be, n):
    dy, z = ew_input("dy", n), ew_input("gelu_z", n)
    got = be.gelu_bwd(dy, z)
    assert got.dtype == BF
    ref, bound = gelu_bwd_ref(dy, z)
    check(got, ref, bound, f"gelu_bwd n={n}")


@functools.lru_cache(maxsize=None)
def xent_flat_input(n):
    """(probs, target) as flat vectors of n elements: head_xent_bwd is
    elementwise, only the element count reaches the kernel."""
    g = gen("xent", n)
    s = torch.rand(n, generator=g).to(BF)
    t = (torch.rand(n, generator=g) < 0.1).to(BF)
    return s, t


def check_head_xent_bwd(be, s, t, gb, what):
    got = be.head_xent_bwd(s, t, gb)
    assert got.dtype == BF and got.shape == s.shape
    ref, bound = head_xent_bwd_ref(s, t, gb)
    check(got, ref, bound, f"head_xent_bwd {what}")


# ------------------------------------------------- the cases of both suites

ROW_GRID = [(B, C) for B in ROW_B for C in ROW_C]
SOFTMAX_CASES = [(k, B, C) for k in SOFTMAX_KINDS for (B, C) in ROW_GRID]
LN_FWD_CASES = [("zero_mean", B, C) for (B, C) in ROW_GRID] \
    + list(LN_SPECIAL) + list(LN_TIER_EDGES)
RELU_SCALES = (1.0, 1.25, 1.0 / 0.7)  # 1 / (1 - p) for p = 0, 0.2, 0.3
XENT_ROWS = (129, 10)                 # n % 8 == 2
