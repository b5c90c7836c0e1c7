"""Forward chain kernel (csrc/fwd_chain.hip): every way to start the
chain and both K loops against the per-layer ops.

Every h_l and probs must be BIT-identical (int16 views) to
F.linear_fwd(relu=True) per layer followed by F.head_fwd_fused, for

  start   l1 = 2 (x streamed through the register-staged LDS stage) with
          kloop = 1 (B fragments one K-step ahead) and kloop = 2 (three
          K-steps ahead in named register sets, loads unguarded and the
          pieces past K0 zeroed at their use)
  arms    (64, 8), (32, 8) and the shipped choice (0, 0)
  depth   1, 3;  C 1, 10
  M       1, 63, 64, 65, 129: one to three tiles, ragged last tile
  K0      a chunk of x is 128 columns = four K-steps = one turn of the
          B ring.  8, 40: less than a chunk (the ring is never turned);
          128: exactly one; 136: one and a piece; 384, 512, 640: whole
          chunks only; 520: four and one piece; 784: six and half a
          K-step; 1160: nine and one piece

The inputs are built as tests/test_gpu_fwd_chain.py builds them (an
all-zero row, -0.0, a NaN, a column driven negative, a pre-activation
that rounds to bf16 inf).  No tolerance anywhere: the kernel promises
the bits.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H = 256
ARMS = [(64, 8), (32, 8), (0, 0)]
STARTS = [(2, 1), (2, 2)]  # (l1, kloop)
DEPTHS = (1, 3)
CS = (1, 10)
MS = [1, 63, 64, 65, 129]
K0S = [8, 40, 128, 136, 384, 512, 520, 640, 784, 1160]


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


_CASES = {}


def reference(c):
    """The per-layer chain of a case's inputs: ([h_l], {C: probs after
    layer `depth`}) for every depth in DEPTHS."""
    from shallowspeed_amd.ops import functional as F

    hs, h = [], c["x"]
    for w, b in zip(c["ws"], c["bs"]):
        h = F.linear_fwd(h, w, b, relu=True)
        hs.append(h)
    probs = {(d, C): F.head_fwd_fused(hs[d - 1], *c["head"][C])
             for d in DEPTHS for C in CS}
    return hs, probs


def chain_case(M, K0, device):
    """Seeded inputs for max(DEPTHS) layers and both heads, and the
    reference outputs; computed once per (M, K0), shared, never
    modified."""
    key = (M, K0)
    if key not in _CASES:
        depth = max(DEPTHS)
        x = randn(M, K0, seed=100 + M + K0)
        x[0, 3] = -0.0
        if M > 1:
            x[M // 2, :] = 0.0
        if M > 2:
            x[M - 1, 5] = float("nan")
        ws = [randn(H, K0, seed=50) / K0 ** 0.5]
        ws += [randn(H, H, seed=50 + l) / H ** 0.5 for l in range(1, depth)]
        bs = [randn(H, seed=60 + l) * 0.1 for l in range(depth)]
        for b in bs:
            b[7] = -1e4
        if M > 3:
            # row 1: 2^127 * (2 - 2^-7) + 2^119 * 1 = bf16_max + ulp/2
            x[1, :] = 0.0
            x[1, 0], x[1, 1] = 2.0 ** 127, 2.0 ** 119
            ws[0][9, 0], ws[0][9, 1] = 2.0 - 2.0 ** -7, 1.0
            bs[0][9] = 0.0
        head = {C: (randn(C, H, seed=30 + C) / H ** 0.5,
                    randn(C, seed=31 + C) * 0.1) for C in CS}

        def dev(t):
            return t.to(device=device, dtype=BF)

        c = dict(x=dev(x), ws=[dev(w) for w in ws], bs=[dev(b) for b in bs],
                 head={C: (dev(w), dev(b)) for C, (w, b) in head.items()})
        c["hs"], c["probs"] = reference(c)
        _CASES[key] = c
    return _CASES[key]


def run_chain(c, depth, C, arm, start, x=None):
    from shallowspeed_amd.ops import functional as F

    l1, kloop = start
    res = F.fwd_chain(c["x"] if x is None else x, c["ws"][:depth],
                      c["bs"][:depth], *c["head"][C], *arm, l1=l1,
                      kloop=kloop)
    assert res is not None, (arm, start)
    return res


@pytest.mark.parametrize("K0", K0S)
@pytest.mark.parametrize("M", MS)
def test_every_start_bit_identical(gpu_device, M, K0):
    c = chain_case(M, K0, gpu_device)
    for depth in DEPTHS:
        for C in CS:
            for arm in ARMS:
                for start in STARTS:
                    hs, probs = run_chain(c, depth, C, arm, start)
                    tag = (depth, C, arm, start)
                    assert len(hs) == depth
                    for l, h in enumerate(hs):
                        assert same_bits(h, c["hs"][l]), (tag, l)
                    assert same_bits(probs, c["probs"][depth, C]), tag


def test_ahead_loop_refused_with_four_waves(gpu_device):
    """kloop = 2 is built for the eight-wave arms only."""
    c = chain_case(64, 136, gpu_device)
    from shallowspeed_amd.ops import functional as F

    for rows in (32, 64):
        assert F.fwd_chain(c["x"], c["ws"], c["bs"], *c["head"][10], rows, 4,
                           l1=2, kloop=2) is None
        assert F.fwd_chain(c["x"], c["ws"], c["bs"], *c["head"][10], rows, 4,
                           l1=2, kloop=1) is not None
    assert F.fwd_chain(c["x"], c["ws"], c["bs"], *c["head"][10], kloop=3) \
        is None


@pytest.mark.parametrize("K0", [40, 520, 784])
def test_non_finite_inputs_stay_in_their_rows(gpu_device, K0):
    """NaN and +-Inf in the last valid 8 columns of x (rows 2 and 5) and
    all over row M-1: the chain is row-local and a piece past K0 is a
    zero whatever lies beside it, so every other row keeps its bits."""
    M = 129
    c = chain_case(M, K0, gpu_device)
    x = c["x"].clone()
    bad = [float("nan"), float("inf"), float("-inf")]
    pat = torch.tensor([bad[k % 3] for k in range(K0 + 1)],
                       device=gpu_device, dtype=BF)
    x[2, K0 - 8:] = pat[:8]
    x[5, K0 - 8:] = pat[1:9]
    x[M - 1, :] = pat[:K0]
    clean = torch.ones(M, dtype=torch.bool, device=gpu_device)
    clean[[2, 5, M - 1]] = False
    # rows that were clean before are clean now: the reference of the
    # unchanged x holds for them
    for arm in ARMS:
        for start in STARTS:
            hs, probs = run_chain(c, 3, 10, arm, start, x=x)
            for l, h in enumerate(hs):
                assert same_bits(h[clean], c["hs"][l][clean]), (arm, start, l)
            assert same_bits(probs[clean], c["probs"][3, 10][clean]), \
                (arm, start)


@pytest.mark.parametrize("arm", ARMS)
def test_twenty_launches_back_to_back(gpu_device, arm):
    """The same launch 20 times on one stream with the same inputs: the
    last result is the reference (stage reuse across launches)."""
    c = chain_case(129, 784, gpu_device)
    for start in STARTS:
        for _ in range(20):
            hs, probs = run_chain(c, 3, 10, arm, start)
        for l, h in enumerate(hs):
            assert same_bits(h, c["hs"][l]), (arm, start, l)
        assert same_bits(probs, c["probs"][3, 10]), (arm, start)
