"""Backward chain kernels under the softmax-MSE head
(csrc/bwd_chain_mse.hip, csrc/bwd_chain_wide_mse.hip) against the
per-layer ops they replace: head_mse_bwd -> gemm_nt(dz, W_head^T) ->
relu_bwd -> gemm_nt(dz_l, W_l^T) -> ...  Every dz_l and dx must be
bit-identical, at every built arm.  At model level the switch
F.set_head_mse_fused must not change probs at all, and the parameter
gradients only by f32 summation order (the weight gradients meet in f32
atomics), held to test_gpu_head_fused.py's model tolerance.

M: one row; 72 = a full 64-row tile and a partial one (two full 32-row
tiles and a partial one); 200 = several tiles, the last partial.
"""

import pytest
import torch

from test_gpu_head_fused import BF, EMPTY, ext, one_hot, rand_bf16, tol

pytestmark = pytest.mark.gpu

# (hidden width, head classes, whether the lowest layer's dgrad is in the
# chain): the layer sizes [40, H, H, 10] and [256, 256, 16]
SHAPES = [(256, 10, False), (256, 16, True), (128, 10, False),
          (512, 10, False)]
_CASES = {}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


def chain_case(M, H, C, dx_in, device):
    """Seeded operands and the per-layer chain's outputs, built once per
    shape and shared, never modified."""
    key = (M, H, C, dx_in)
    if key not in _CASES:
        e = ext()
        n = 1 if dx_in else 2
        probs = torch.softmax(rand_bf16(M, C, device=device, seed=M).float(),
                              dim=1).to(BF)
        t = one_hot(M, C, device, seed=M + 1)
        w_head_t = rand_bf16(H, C, device=device, scale=H ** -0.5, seed=C)
        # mask sources, top first: negatives, zeros and positives
        hs = [rand_bf16(M, H, device=device, seed=H + l).relu()
              for l in range(n)]
        w_ts = [rand_bf16(H, H, device=device, scale=H ** -0.5, seed=7 + l)
                for l in range(n if dx_in else n - 1)]
        gb = 3 * M
        dz_head = e.head_mse_bwd(probs, t, float(gb))
        dh = e.gemm_nt(dz_head, w_head_t, EMPTY, EMPTY, False)
        dzs = []
        for l in range(n):
            dzs.append(e.relu_bwd(dh, hs[l]))
            dh = e.gemm_nt(dzs[-1], w_ts[l], EMPTY, EMPTY, False) \
                if l < len(w_ts) else None
        _CASES[key] = dict(args=(probs, t, w_head_t, gb, hs, w_ts),
                           dz_head=dz_head, dzs=dzs, dx=dh)
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("M", [1, 72, 200])
def test_chain_bit_identical(gpu_device, M, shape):
    from shallowspeed_amd.ops import functional as F

    H, C, dx_in = shape
    c = chain_case(M, H, C, dx_in, gpu_device)
    if H == 256:
        op = F.bwd_chain
        arms = [(0, 0), (32, 4), (32, 8), (64, 4), (64, 8)]
    else:
        op = F.bwd_chain_wide
        arms = [(0, 0)] + list(F.CHAIN_WIDE_ARMS[H])
    for arm in arms:
        res = op(*c["args"], *arm, loss="mse")
        assert res is not None, arm
        dz_head, dzs, dx = res
        assert same_bits(dz_head, c["dz_head"]), arm
        assert len(dzs) == len(c["dzs"])
        for got, want in zip(dzs, c["dzs"]):
            assert same_bits(got, want), arm
        assert (dx is None) == (c["dx"] is None)
        assert dx is None or same_bits(dx, c["dx"]), arm


@pytest.mark.parametrize("M", [72, 200])
def test_chain_scaled_bit_identical(gpu_device, M):
    """The dropout-scaled form of the shipped arm: dz_head is unscaled,
    every kept dz_l element is bf16(dh * dz_scale)."""
    from shallowspeed_amd.ops import functional as F

    e = ext()
    c = chain_case(M, 256, 16, True, gpu_device)
    probs, t, w_head_t, gb, hs, w_ts = c["args"]
    dz_head, dzs, dx = F.bwd_chain(*c["args"], dz_scale=1.25, loss="mse")
    assert same_bits(dz_head, c["dz_head"])
    dh = e.gemm_nt(dz_head, w_head_t, EMPTY, EMPTY, False)
    want = F.relu_bwd(dh, hs[0], scale=1.25)
    assert same_bits(dzs[0], want)
    assert same_bits(dx, e.gemm_nt(want, w_ts[0], EMPTY, EMPTY, False))
    # no W-through-LDS arm under this loss: refused, nothing launched
    assert F.bwd_chain(*c["args"], 64, 8, 1, loss="mse") is None


@pytest.mark.parametrize("H", [256, 128, 512])
def test_model_switch_on_vs_off(gpu_device, monkeypatch, H):
    from shallowspeed_amd.models import MLP
    from shallowspeed_amd.ops import functional as F

    B = 72
    monkeypatch.setattr(F, "_CHAIN_WIDE", True)  # plan 128 / 512 at any B
    x = rand_bf16(B, 40, device=gpu_device, seed=5)
    t = one_hot(B, 10, gpu_device, seed=6)
    calls = []
    for name in ("head_softmax_mse_bwd", "bwd_chain", "bwd_chain_wide"):
        real = getattr(F, name)
        monkeypatch.setattr(
            F, name, lambda *a, _n=name, _r=real, **k: (
                calls.append((_n, k.get("loss"))), _r(*a, **k))[1])

    def run(on):
        monkeypatch.setattr(F, "_HEAD_MSE_FUSED", on)
        del calls[:]
        model = MLP([40, H, H, 10], 0, 1, B, loss="mse")
        model.materialize_device(gpu_device)
        model.zero_grad()
        p = model.forward(x, 0)
        model.backward(t, 0)
        torch.cuda.synchronize()
        return p, [q.grad.float().cpu() for q in model.parameters()], \
            list(calls)

    p_on, g_on, c_on = run(True)
    p_off, g_off, c_off = run(False)
    assert c_on == [("bwd_chain" if H == 256 else "bwd_chain_wide", "mse")]
    assert c_off == [("head_softmax_mse_bwd", None)]
    assert torch.equal(p_on, p_off)
    for g, r in zip(g_on, g_off):
        torch.testing.assert_close(g, r, **tol(r))
