"""Deterministic-mode wgrad plumbing: "single" | "ordered", its
SS_DET_WGRAD default, and the CPU path of linear_wgrad_acc(ordered=True).
"""

import pytest
import torch

from shallowspeed_amd.ops import functional as F


@pytest.fixture
def fresh(monkeypatch):
    """functional's mode state as at import; restored afterwards."""
    for name in ("_DETERMINISTIC", "_DET_WGRAD", "_DET_WGRAD_ENV"):
        monkeypatch.setattr(F, name, False if name == "_DETERMINISTIC"
                            else None)
    return monkeypatch


def test_default_and_keyword(fresh):
    fresh.delenv("SS_DET_WGRAD", raising=False)
    assert F.deterministic() is False
    assert F.deterministic_wgrad() == "single"
    F.set_deterministic(True, wgrad="ordered")
    assert F.deterministic() is True
    assert F.deterministic_wgrad() == "ordered"
    F.set_deterministic(True)  # no keyword: back to the default
    assert F.deterministic() is True
    assert F.deterministic_wgrad() == "single"
    with pytest.raises(ValueError):
        F.set_deterministic(True, wgrad="fast")


def test_environment_default_is_read_once(fresh):
    fresh.setenv("SS_DET_WGRAD", "ordered")
    F.set_deterministic(True)
    assert F.deterministic() is True
    assert F.deterministic_wgrad() == "ordered"
    fresh.setenv("SS_DET_WGRAD", "single")
    assert F.deterministic_wgrad() == "ordered"
    F.set_deterministic(True, wgrad="single")
    assert F.deterministic_wgrad() == "single"


@pytest.mark.parametrize("masked", [False, True])
def test_cpu_ordered_equals_plain(masked):
    g = torch.Generator().manual_seed(5)
    dy, x = torch.randn(33, 7, generator=g), torch.randn(33, 12, generator=g)
    mask = torch.randn(33, 7, generator=g) if masked else None
    out = []
    for ordered in (False, True):
        gw, gb = torch.ones(7, 12), torch.ones(7)
        F.linear_wgrad_acc(dy, x, gw, gb, mask, split_k=3, ordered=ordered)
        out.append((gw, gb))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
