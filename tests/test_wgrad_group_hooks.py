"""Grad hooks around the grouped weight-gradient call
(Sequential._wgrad_group), on the CPU path of F.linear_wgrad_group.

The DP overlap hangs on the hooks: each parameter's hook fires once, in
the per-layer path's order (head, then top to bottom), and only after
the parameter's own gradient is complete.
"""

import torch

from shallowspeed_amd.models import MLP
from shallowspeed_amd.models.layers import Linear
from shallowspeed_amd.ops import functional as F

SIZES = [48, 256, 256, 256, 10]
B = 24


def _model():
    model = MLP(SIZES, 0, 1, B, loss="xent").materialize_device("cpu")
    model.zero_grad()
    return model


def _record_hooks(model):
    seen = []
    index = {id(p): k for k, p in enumerate(model.parameters())}
    model.register_grad_hook(
        lambda p: seen.append((index[id(p)], p.grad.clone())))
    return seen


def _per_layer(monkeypatch):
    """One backward on the per-layer path: the hook record, the final
    grads, and every layer's (dz, x) as its wgrad call saw them."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, SIZES[0], generator=g)
    t = torch.zeros(B, SIZES[-1])
    t[torch.arange(B), torch.randint(0, SIZES[-1], (B,), generator=g)] = 1
    model = _model()
    seen = _record_hooks(model)
    calls, real = {}, F.linear_wgrad_acc

    def rec(dy, xx, gw, gb=None, mask_src=None, split_k=0):
        dz = dy if mask_src is None else dy * (mask_src > 0).to(dy.dtype)
        calls[gw.data_ptr()] = (dz.clone(), xx.clone())
        return real(dy, xx, gw, gb, mask_src, split_k)

    monkeypatch.setattr(F, "linear_wgrad_acc", rec)
    model.forward(x, 0)
    model.backward(t, 0)
    monkeypatch.setattr(F, "linear_wgrad_acc", real)
    lins = [l for l in model.layers if isinstance(l, Linear)]
    ops = [calls[l.weight.grad.data_ptr()] for l in lins]
    return seen, [p.grad.clone() for p in model.parameters()], ops


def _grouped(ops):
    model = _model()
    seen = _record_hooks(model)
    lins = [l for l in model.layers if isinstance(l, Linear)]
    head = model.layers[-1]
    items = [(lins[-1], *ops[-1], (head, lins[-1]))]
    for l, (dz, x) in reversed(list(zip(lins[:-1], ops[:-1]))):
        items.append((l, dz, x, (l,)))
    model._wgrad_group(items)
    return seen, [p.grad.clone() for p in model.parameters()]


def test_hooks_fire_once_per_parameter_in_the_per_layer_order(monkeypatch):
    ref_seen, ref_grads, ops = _per_layer(monkeypatch)
    seen, grads = _grouped(ops)
    order = [k for k, _ in seen]
    assert sorted(order) == list(range(len(grads)))  # once each
    assert order == [k for k, _ in ref_seen]
    for g, r in zip(grads, ref_grads):
        assert torch.equal(g, r)


def test_each_hook_sees_its_complete_gradient(monkeypatch):
    _, _, ops = _per_layer(monkeypatch)
    seen, grads = _grouped(ops)
    for k, g in seen:
        assert g.abs().max() > 0
        assert torch.equal(g, grads[k])


def test_without_hooks_the_list_is_one_call(monkeypatch):
    _, ref_grads, ops = _per_layer(monkeypatch)
    calls, real = [], F.linear_wgrad_group

    def rec(problems, splits=None):
        calls.append(len(list(problems)))
        return real(problems, splits)

    monkeypatch.setattr(F, "linear_wgrad_group", rec)
    model = _model()
    lins = [l for l in model.layers if isinstance(l, Linear)]
    items = [(l, *ops[k], (l,)) for k, l in reversed(list(enumerate(lins)))]
    model._wgrad_group(items)
    assert calls == [4]
    for g, r in zip([p.grad for p in model.parameters()], ref_grads):
        assert torch.equal(g, r)
