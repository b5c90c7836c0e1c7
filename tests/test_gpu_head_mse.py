"""Squared-error arm of the fused head backward (csrc/head_mse.hip)
against the unfused ops it replaces and against float64.

dz must have the bits of head_mse_bwd (the row sum is the same tree over
the same partials) and lie inside rowwise_oracle's float64 bound; dx must
have the bits of gemm_nt(dz, W^T); gW / gb are held to the f32 reordering
bound test_gpu_head_fused.py derives, from the same dz bits; the metrics
arm counts what head_metrics(kind="mse") counts and its loss_sum, an f32
sum of n = M*C squared errors in some order, is within n * 2^-24 *
sum|term| of the float64 sum over the same bf16 probs.

Shapes: K = 288 crosses the 256-column chunk and K = 256 the 128-row
arm's 128-column one; C = 16 leaves no idle lane among a row's 16, C = 1
makes dz identically zero; M = 1 and 33 leave tiles mostly past M.
"""

import pytest
import torch

import rowwise_oracle as O
from test_gpu_head_fused import (EMPTY, assert_within, ext,
                                 grad_ref_and_bound, head_case, rand_bf16)

pytestmark = pytest.mark.gpu

MSE = 1  # the ops' `loss` argument


@pytest.mark.parametrize("rb", [32, 64, 128])
@pytest.mark.parametrize("KC", [(32, 1), (64, 10), (256, 16), (288, 10)],
                         ids=lambda kc: f"K{kc[0]}C{kc[1]}")
@pytest.mark.parametrize("M", [1, 33, 200])
def test_mse_arm(gpu_device, M, KC, rb):
    from shallowspeed_amd.ops import functional as F

    K, C = KC
    e = ext()
    c = head_case(M, K, C, gpu_device)
    probs, t, x, w_t = c["probs"], c["t"], c["x"], c["w_t"]
    gb = 3 * M  # no power of two: 1/GB rounds in f32
    want_dz = e.head_mse_bwd(probs, t, float(gb))
    want_dx = e.gemm_nt(want_dz, w_t, EMPTY, EMPTY, False)

    dz, dx = e.head_bwd_fused(probs, t, x, w_t, float(gb), EMPTY, EMPTY, rb,
                              None, 0, MSE)
    assert torch.equal(dz.view(torch.int16), want_dz.view(torch.int16))
    assert torch.equal(dx.view(torch.int16), want_dx.view(torch.int16))
    ref, bound = O.head_mse_bwd_ref(probs.cpu(), t.cpu(), gb)
    O.check(dz, ref, bound, f"fused mse dz M{M} K{K} C{C} rb{rb}")

    # gW / gb accumulate from a non-zero start, twice; the first call
    # also counts
    g0w = rand_bf16(C, K, device=gpu_device, seed=7).float() * 1.37
    g0b = rand_bf16(C, device=gpu_device, seed=8).float() * 0.73
    ref_w, ref_b, bnd_w, bnd_b = grad_ref_and_bound(want_dz, x, g0w, g0b, M)
    gw, gbias = g0w.clone(), g0b.clone()
    acc = F.new_metrics_acc(gpu_device)
    for n in (1, 2):
        dz, dx = e.head_bwd_fused(probs, t, x, w_t, float(gb), gw, gbias, rb,
                                  acc if n == 1 else None, 0, MSE)
        assert torch.equal(dz.view(torch.int16), want_dz.view(torch.int16))
        assert torch.equal(dx.view(torch.int16), want_dx.view(torch.int16))
        g0w64, g0b64 = g0w.double().cpu(), g0b.double().cpu()
        assert_within(gw, g0w64 + n * (ref_w - g0w64), bnd_w, f"gW x{n}")
        assert_within(gbias, g0b64 + n * (ref_b - g0b64), bnd_b, f"gb x{n}")

    got = F.read_metrics_acc(acc)
    alone = F.new_metrics_acc(gpu_device)
    F.head_metrics(probs, t, alone, "mse")
    want = F.read_metrics_acc(alone)
    for k in ("correct", "rows", "nonfinite"):
        assert got[k] == want[k], (k, got[k], want[k])
    terms = (t.double().cpu() - probs.double().cpu()) ** 2
    loss = terms.sum().item()
    loss_bound = M * C * 2.0 ** -24 * terms.abs().sum().item()
    print(f"loss_sum {got['loss_sum']!r} ref {loss!r} bound {loss_bound:.3e}")
    assert abs(got["loss_sum"] - loss) <= loss_bound


def test_loss_argument_is_checked(gpu_device):
    e = ext()
    c = head_case(33, 64, 10, gpu_device)
    with pytest.raises(RuntimeError):
        e.head_bwd_fused(c["probs"], c["t"], c["x"], c["w_t"], 33.0, EMPTY,
                         EMPTY, 0, None, 0, 2)
